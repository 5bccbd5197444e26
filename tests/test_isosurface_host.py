"""CPU: the isosurface specification as tests/isosurface_ref.py restates it (closed, oriented, welded meshes of analytic fields), the
library's derived case table against the restatement's, the entry points' refusals without a device, and nerf.write_mesh."""
import ctypes
import math
import struct

import numpy as np
import pytest

from tests import isosurface_ref as R

FIELDS = {"sphere": (2, 4.0 / 3.0 * math.pi * 0.7 ** 3), "torus": (0, 2.0 * math.pi ** 2 * 0.55 * 0.22 ** 2), "two_spheres": (4, None),
          "noise": (None, None)}
_MESHES = {}


def _mesh(name):
    if name not in _MESHES:
        if name == "noise":
            v, lo, hi = R.noise_field(), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
        else:
            v, lo, hi = getattr(R, name)(*R.grid_points(R.BOX_LO, R.BOX_HI, R.BOX_N)), R.BOX_LO, R.BOX_HI
        _MESHES[name] = R.isosurface(v, 0.0, lo, hi, normals=True)
    return _MESHES[name]


@pytest.mark.parametrize("name", list(FIELDS))
def test_restatement_gives_closed_oriented_welded_meshes(name):
    """Every directed edge once and its reverse once, no zero-area triangle, every vertex referenced, positive signed volume (normals
    point outward), the Euler characteristic of the analytic surface; the sphere's volume within 5 % of 4/3 pi r^3."""
    chi, volume = FIELDS[name]
    verts, faces, normals = _mesh(name)
    rep = R.mesh_report(verts, faces)
    print(name, verts.shape[0], faces.shape[0], rep)
    assert faces.shape[0] > 0 and faces.min() >= 0 and faces.max() < verts.shape[0]
    assert rep["closed"] and rep["zero_area"] == 0 and rep["unreferenced"] == 0 and rep["volume"] > 0
    assert np.isfinite(verts).all() and np.isfinite(normals).all()
    if chi is not None:
        assert rep["chi"] == chi
    if name == "sphere":
        assert abs(rep["volume"] / volume - 1.0) < 0.05, rep["volume"] / volume
    if name == "torus":
        assert 0.85 < rep["volume"] / volume < 1.0          # an inscribed polyhedron of a coarse grid: below the analytic volume
    if name in ("sphere", "torus"):
        length = np.linalg.norm(normals.astype(np.float64), axis=1)
        assert np.abs(length - 1.0).max() < 1e-6


def test_vertices_lie_on_their_edges_and_follow_the_scan_order():
    """Every vertex of the sphere lies inside the box on a segment between two grid points of opposite sides; the ids follow the
    (k, j, i, e) order, so the z of the owner never decreases."""
    verts, faces, _ = _mesh("sphere")
    lo, hi = np.float32(R.BOX_LO), np.float32(R.BOX_HI)
    assert (verts >= lo).all() and (verts <= hi).all()
    hz = (hi[2] - lo[2]) / np.float32(R.BOX_N[2] - 1)
    owner_k = np.floor((verts[:, 2].astype(np.float64) - lo[2]) / hz + 1e-4).astype(int)
    r = np.linalg.norm(verts.astype(np.float64), axis=1)
    assert np.abs(r - 0.7).max() < 0.01                      # linear interpolation of r^2 - |p|^2 along an edge of length <= 0.19
    assert (np.diff(owner_k) >= -1).all() and owner_k[0] <= owner_k[-1]


def test_library_table_is_the_derived_table(hip_lib):
    """nf_isosurface_table == the restatement's derivation, entry for entry; 14 live entries per tetrahedron; a quad's two triangles
    share the inside -> outside side (the derivation asserts it) and the flip bit is set exactly where the restatement flips."""
    out = (ctypes.c_uint32 * 96)()
    assert hip_lib.nf_isosurface_table(out) == 0
    got, want = np.array(out, dtype=np.uint32).reshape(6, 16), R.derive_table()
    assert np.array_equal(got, want)
    assert hip_lib.nf_isosurface_table(None) == -22
    for tet in range(6):
        assert got[tet, 0] == 0 and got[tet, 15] == 0 and np.count_nonzero(got[tet]) == 14
        for mask in range(1, 15):
            tris, flip = R.case_triangles(tet, mask)
            assert (got[tet, mask] >> 24) & 3 == len(tris) == (2 if bin(mask).count("1") == 2 else 1)
            assert bool(got[tet, mask] >> 26 & 1) == flip
            # the complementary mask cuts the same edges with the opposite orientation
            other, _ = R.case_triangles(tet, 15 - mask)
            assert sorted(sorted(t) for t in tris) == sorted(sorted(t) for t in other)
    assert [R.tet_corners(t) for t in range(6)] == [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]


def test_entry_points_refuse_before_touching_the_device(hip_lib):
    """NF_EINVAL (-22) for NULL pointers, an axis below 2, a workspace that is too small, lo >= hi on an axis, a negative capacity and
    a grid past the plan (7 * points or 12 * cells above 2^31 - 1); the size query answers 0 for what it does not serve.  The
    pointers handed over are never dereferenced on these paths, so small integers stand in for device memory."""
    ws_bytes = hip_lib.nf_isosurface_workspace_bytes
    assert ws_bytes(1, 4, 4) == 0 and ws_bytes(4, 1, 4) == 0 and ws_bytes(4, 4, 1) == 0 and ws_bytes(-3, 4, 4) == 0
    assert ws_bytes(675, 675, 675) == 0 and ws_bytes(2 ** 16, 2 ** 16, 2) == 0 and ws_bytes(2 ** 30, 2 ** 30, 2 ** 30) == 0
    assert ws_bytes(564, 564, 564) > 0 and ws_bytes(565, 565, 565) == 0   # 12 * 563^3 < 2^31 <= 12 * 564^3
    assert ws_bytes(2, 2, 2 ** 26) > 0 and ws_bytes(2, 2, 2 ** 27) == 0   # 7 * 2^28 < 2^31 <= 7 * 2^29
    n = ws_bytes(23, 19, 21)
    points = 23 * 19 * 21
    assert n >= 256 + 6 * points and n % 256 == 0 and n < 256 * 6 + 6 * points + 8 * 256
    assert ws_bytes(512, 512, 512) >= 6 * 512 ** 3
    P = 4096                                                              # a non-NULL stand-in
    lo, hi = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(1, 1, 1)
    a = ctypes.addressof
    count, emit = hip_lib.nf_isosurface_count, hip_lib.nf_isosurface_emit
    assert count(None, 4, 4, 4, 0.0, P, n, P, None) == -22
    assert count(P, 4, 4, 4, 0.0, None, n, P, None) == -22
    assert count(P, 4, 4, 4, 0.0, P, n, None, None) == -22
    assert count(P, 1, 4, 4, 0.0, P, n, P, None) == -22
    assert count(P, 23, 19, 21, 0.0, P, n - 1, P, None) == -22
    assert count(P, 675, 675, 675, 0.0, P, 1 << 40, P, None) == -22
    ok = dict(grid=P, nx=23, ny=19, nz=21, level=0.0, lo=a(lo), hi=a(hi), ws=P, ws_bytes=n, verts=P, n_verts=10, faces=P, n_faces=10, normals=None,
              stream=None)
    for change in (dict(grid=None), dict(ws=None), dict(lo=None), dict(hi=None), dict(verts=None), dict(faces=None), dict(nx=1), dict(nz=0),
                   dict(ws_bytes=n - 1), dict(n_verts=-1), dict(n_faces=-1), dict(n_verts=2 ** 31), dict(nx=675, ny=675, nz=675, ws_bytes=1 << 40)):
        assert emit(*{**ok, **change}.values()) == -22, change
    for axis in range(3):
        for bad in (1.0, 2.0, float("nan")):
            lo_bad = (ctypes.c_float * 3)(-1, -1, -1)
            lo_bad[axis] = bad
            assert emit(*{**ok, "lo": a(lo_bad)}.values()) == -22, (axis, bad)


@pytest.mark.parametrize("with_normals", [True, False])
def test_write_mesh_round_trips(tmp_path, with_normals):
    """.off, .obj and .ply parse back to the same arrays (float32 exactly: nine significant digits); the .ply bytes are exactly the
    header, V rows of little-endian floats and F rows of (uchar 3, three int32)."""
    import nerf
    import torch
    verts, faces, normals = _mesh("two_spheres")
    mesh = nerf.Mesh(torch.from_numpy(verts), torch.from_numpy(faces), torch.from_numpy(normals) if with_normals else None)
    # .off
    p = str(tmp_path / "m.off")
    nerf.write_mesh(p, mesh)
    lines = open(p).read().split("\n")
    assert lines[0] == "OFF" and lines[1].split() == [str(len(verts)), str(len(faces)), "0"]
    got_v = np.array([l.split() for l in lines[2:2 + len(verts)]], dtype=np.float64).astype(np.float32)
    got_f = np.array([l.split() for l in lines[2 + len(verts):2 + len(verts) + len(faces)]], dtype=np.int64)
    assert np.array_equal(got_v, verts) and (got_f[:, 0] == 3).all() and np.array_equal(got_f[:, 1:], faces)
    # .obj
    p = str(tmp_path / "m.obj")
    nerf.write_mesh(p, mesh)
    rows = [l.split() for l in open(p).read().split("\n") if l]
    got_v = np.array([r[1:] for r in rows if r[0] == "v"], dtype=np.float64).astype(np.float32)
    got_n = [r[1:] for r in rows if r[0] == "vn"]
    got_f = np.array([[int(x.split("/")[0]) for x in r[1:]] for r in rows if r[0] == "f"])
    assert np.array_equal(got_v, verts) and np.array_equal(got_f - 1, faces)
    if with_normals:
        assert np.array_equal(np.array(got_n, dtype=np.float64).astype(np.float32), normals)
        assert all(x.split("/") == [x.split("/")[0], "", x.split("/")[0]] for r in rows if r[0] == "f" for x in r[1:])
    else:
        assert not got_n
    # .ply
    p = str(tmp_path / "m.ply")
    nerf.write_mesh(p, (mesh.vertices, mesh.faces) if not with_normals else mesh)
    vert, got_f, props, head, body = R.read_ply(p)
    assert props == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else [])
    assert np.array_equal(vert[:, :3], verts) and np.array_equal(got_f, faces)
    want = (np.concatenate([verts, normals], axis=1) if with_normals else verts).astype("<f4").tobytes()
    want += b"".join(struct.pack("<B3i", 3, *row) for row in faces.tolist())
    assert body == want
    with pytest.raises(ValueError):
        nerf.write_mesh(str(tmp_path / "m.stl"), mesh)


def test_python_layer_refuses_what_it_cannot_serve():
    """ops.isosurface and nerf.density_grid on host tensors raise (no CPU path); a box with lo >= hi and a resolution below 2 are
    ValueErrors before anything is evaluated."""
    import nerf
    import torch
    from nerf import ops
    with pytest.raises(RuntimeError):
        ops.isosurface(torch.zeros(4, 4, 4), 0.0, (-1, -1, -1), (1, 1, 1))
    with pytest.raises(ValueError):
        ops.isosurface(torch.zeros(4, 4), 0.0, (-1, -1, -1), (1, 1, 1))
    m = nerf.models.ConditionalBlendshapePaperNeRFModel(num_encoding_fn_xyz=10, num_encoding_fn_dir=4, include_input_dir=False)
    with pytest.raises(RuntimeError):
        nerf.density_grid(m, torch.zeros(76), torch.zeros(32), lo=(-1, -1, -1), hi=(1, 1, 1), resolution=4)
    with pytest.raises(ValueError):
        nerf.mesh.grid_axes((0, 0, 0), (1, 0, 1), 4)
    with pytest.raises(ValueError):
        nerf.mesh.grid_axes((0, 0, 0), (1, 1, 1), (4, 1, 4))
    with pytest.raises(TypeError):
        nerf.extract_mesh(m, torch.zeros(76), torch.zeros(32), lo=(0, 0, 0), hi=(1, 1, 1), resolution=4)      # level has no default
    xs, ys, zs = nerf.mesh.grid_axes(R.BOX_LO, R.BOX_HI, R.BOX_N)
    x, y, z = R.grid_points(R.BOX_LO, R.BOX_HI, R.BOX_N)
    assert np.array_equal(xs, x[0, 0]) and np.array_equal(ys, y[0, :, 0]) and np.array_equal(zs, z[:, 0, 0])
