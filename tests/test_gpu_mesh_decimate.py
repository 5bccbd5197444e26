"""Mesh decimation on the GPU: ops.decimate_mesh and the C entry points against tests/mesh_decimate_ref.py.  Every float32 and float64
operation of the specification is one NumPy operation there, so every comparison is array_equal on the bit patterns.  Every mesh
goes through both layers: the entry points with the workspace 256 bytes inside its allocation and pre-filled (0xFF, 0x00, seeded
random bytes), every output PAD entries longer than needed and filled with 0xFF, the guards and the padding untouched; then ops.
Empty and tiny inputs, hand meshes for the coincidence rule, invalid inputs, cluster sizes round a wave and a workgroup, tables at
load 0.5, block and scan-round edges, isosurfaces of known fields, and the model-level functions.  GPU only."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from oracle import cases as C
from tests import isosurface_ref as R
from tests import mesh_colour_ref as K
from tests import mesh_decimate_ref as D
from tests import mesh_smooth_ref as S
from tests import util as U
from tests.test_gpu_mesh_smooth import GRID_HI, GRID_LO, GRID_N

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 40                       # entries every output buffer is longer than it needs to be
FILLS = (0xFF, 0x00, (1,))     # the workspace arrives with: every byte 0xFF, every byte 0, seeded random bytes
STATS = ("kept_vertices", "kept_faces", "degenerate_faces", "coincident_faces", "invalid_faces", "unclustered_vertices", "largest_cluster")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _faces(faces):
    return np.ascontiguousarray(np.asarray(faces, dtype=np.int32).reshape(-1, 3))


def _three(x):
    import ctypes
    return (ctypes.c_float * 3)(*D._three(x).tolist())


def _entry_points(gpu, vertices, faces, cell, origin, ws_fill=0xFF, wrong_sizes=False):
    """count and emit through the C ABI; returns host copies: counts (int64, one guard entry on either side), out_vertices (as int32),
    out_faces, vertex_map, each with its padding."""
    import ctypes
    from nerf import _hip as H
    lib = H.lib()
    n_vertices, n_faces = vertices.shape[0], faces.shape[0]
    poison = lambda n, dtype=torch.int32: torch.full((n,), -1, dtype=dtype, device=gpu)       # -1: every byte 0xFF
    ws_bytes = lib.nf_mesh_decimate_workspace_bytes(n_vertices, n_faces)
    assert ws_bytes >= 256
    if isinstance(ws_fill, tuple):
        ws = torch.from_numpy(np.random.default_rng(ws_fill[0]).integers(0, 256, size=ws_bytes + 512, dtype=np.uint8)).to(gpu)
    else:
        ws = torch.full((ws_bytes + 512,), ws_fill, dtype=torch.uint8, device=gpu)
    guard = (ws[:256].clone(), ws[256 + ws_bytes:].clone())
    assert ws.data_ptr() % 256 == 0
    d_v, d_f = torch.from_numpy(np.ascontiguousarray(vertices)).to(gpu), torch.from_numpy(faces).to(gpu)
    c_origin, c_cell = _three(origin), _three(cell)
    counts = poison(8 + 2, torch.int64)
    stream = H.stream_ptr(gpu)
    H.check(lib.nf_mesh_decimate_count(H.ptr(d_v), H.ptr(d_f), n_vertices, n_faces, ctypes.addressof(c_origin), ctypes.addressof(c_cell), ws.data_ptr() + 256,
                                       ws_bytes, counts.data_ptr() + 8, stream), "count")
    kept_v, kept_f = counts[1:3].tolist()
    out_v, out_f, vertex_map = poison(3 * kept_v + PAD), poison(3 * kept_f + PAD), poison(n_vertices + PAD)
    emit = lambda nv, nf: lib.nf_mesh_decimate_emit(H.ptr(d_v), H.ptr(d_f), n_vertices, n_faces, ctypes.addressof(c_origin), ctypes.addressof(c_cell),
                                                    ws.data_ptr() + 256, ws_bytes, H.ptr(out_v), nv, H.ptr(out_f), nf, H.ptr(vertex_map), stream)
    if wrong_sizes and n_vertices:                                  # sizes that count did not find: refused, and nothing is written
        for nv, nf in ((kept_v + 1, kept_f), (kept_v, kept_f + 1), (kept_v - 1, kept_f), (kept_v, kept_f - 1)):
            if 0 <= nv <= n_vertices and 0 <= nf <= n_faces:
                assert emit(nv, nf) == -22
        torch.cuda.synchronize()
        assert bool((out_v == -1).all()) and bool((out_f == -1).all()) and bool((vertex_map == -1).all())
    H.check(emit(kept_v, kept_f), "emit")
    torch.cuda.synchronize()
    assert torch.equal(ws[:256], guard[0]) and torch.equal(ws[256 + ws_bytes:], guard[1])
    return [t.cpu().numpy() for t in (counts, out_v, out_f, vertex_map)]


class _Reference:
    """The restatement's result of one mesh on one lattice, computed once."""

    def __init__(self, vertices, faces, cell, origin=(0.0, 0.0, 0.0)):
        self.vertices, self.faces = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3), _faces(faces)
        self.cell, self.origin = cell, origin
        self.out_v, self.out_f, _, self.vertex_map, self.stats = D.decimate(self.vertices, self.faces, cell, origin)
        self._normals = None

    @property
    def normals(self):
        if self._normals is None:
            self._normals = S.vertex_normals(self.out_v, self.out_f)
        return self._normals


def _check_entry_points(gpu, ref, what, **kw):
    got = _entry_points(gpu, ref.vertices, ref.faces, ref.cell, ref.origin, **kw)
    counts, out_v, out_f, vertex_map = got
    st = ref.stats
    assert counts.tolist() == [-1] + [st[k] for k in STATS] + [0, -1], (what, counts, st)
    nv, nf, n = 3 * st["kept_vertices"], 3 * st["kept_faces"], st["vertices"]
    assert np.array_equal(out_v[:nv].view(np.uint32), _bits(ref.out_v).reshape(-1)) and (out_v[nv:] == -1).all() and len(out_v) - nv == PAD, what
    assert np.array_equal(out_f[:nf], ref.out_f.reshape(-1)) and (out_f[nf:] == -1).all() and len(out_f) - nf == PAD, what
    assert np.array_equal(vertex_map[:n], ref.vertex_map) and (vertex_map[n:] == -1).all(), what
    return got


def _check_ops(gpu, ref, what, with_normals=True, strided=False):
    from nerf import ops
    d_v, d_f = torch.from_numpy(ref.vertices).to(gpu), torch.from_numpy(ref.faces).to(gpu)
    if strided:
        wide_v, wide_f = torch.full((len(d_v), 6), 9.0, device=gpu), torch.full((3, len(d_f) + 2), -5, dtype=torch.int32, device=gpu)
        wide_v[:, ::2], wide_f[:, 1:-1] = d_v, d_f.t()
        d_v, d_f = wide_v[:, ::2], wide_f[:, 1:-1].t()
        assert (len(d_v) < 2 or not d_v.is_contiguous()) and (len(d_f) < 2 or not d_f.is_contiguous())
    got = ops.decimate_mesh(d_v, d_f, torch.full_like(d_v, 7.0) if with_normals else None, cell=ref.cell, origin=ref.origin)
    out_v, out_f, out_n, vertex_map, stats = got
    st = ref.stats
    assert isinstance(stats, ops.MeshDecimateStats) and stats._asdict() == st, (what, stats, st)
    assert out_v.is_cuda and out_v.dtype == torch.float32 and tuple(out_v.shape) == (st["kept_vertices"], 3), what
    assert out_f.is_cuda and out_f.dtype == torch.int32 and tuple(out_f.shape) == (st["kept_faces"], 3), what
    assert vertex_map.is_cuda and vertex_map.dtype == torch.int32 and tuple(vertex_map.shape) == (st["vertices"],), what
    assert np.array_equal(_bits(out_v.cpu().numpy()), _bits(ref.out_v)) and np.array_equal(out_f.cpu().numpy(), ref.out_f), what
    assert np.array_equal(vertex_map.cpu().numpy(), ref.vertex_map), what
    if with_normals:
        assert out_n.dtype == torch.float32 and tuple(out_n.shape) == (st["kept_vertices"], 3), what
        assert np.array_equal(_bits(out_n.cpu().numpy()), _bits(ref.normals)), what
    else:
        assert out_n is None
    return got


def _check_mesh(gpu, vertices, faces, cell, origin=(0.0, 0.0, 0.0), what="", fills=FILLS, ops_normals=(True, False)):
    ref = _Reference(vertices, faces, cell, origin)
    for k, fill in enumerate(fills):
        _check_entry_points(gpu, ref, what, ws_fill=fill, wrong_sizes=k == 0)
    for with_normals in ops_normals:
        _check_ops(gpu, ref, what, with_normals=with_normals)
    return ref


# ---- 1. empty and tiny inputs
def test_no_vertices_and_no_faces(hip_lib, gpu):
    ref = _check_mesh(gpu, np.zeros((0, 3), np.float32), [], 1.0, what="nothing")
    assert ref.stats == dict(vertices=0, kept_vertices=0, faces=0, kept_faces=0, degenerate_faces=0, coincident_faces=0, invalid_faces=0,
                             unclustered_vertices=0, largest_cluster=0)
    ref = _check_mesh(gpu, np.zeros((0, 3), np.float32), [(0, 0, 0), (0, 1, 2)], 1.0, what="faces over no vertex")
    assert ref.stats["invalid_faces"] == 2 and ref.stats["kept_faces"] == 0
    ref = _check_mesh(gpu, S.positions(5, seed=1), [], 0.25, what="five vertices, no face")
    assert ref.stats["kept_vertices"] == 0 and ref.vertex_map.tolist() == [-1] * 5 and ref.out_v.shape == (0, 3) and ref.out_f.shape == (0, 3)


def test_one_triangle(hip_lib, gpu):
    from nerf import ops
    v = np.array([[0.5, 0.25, 0.125], [1.5, 0.25, 0.125], [0.5, 1.75, -0.125]], dtype=np.float32)
    ref = _check_mesh(gpu, v, [(2, 0, 1)], 1.0, what="corners in three cells")
    assert np.array_equal(_bits(ref.out_v), _bits(v)) and ref.out_f.tolist() == [[2, 0, 1]] and ref.vertex_map.tolist() == [0, 1, 2]
    assert ref.stats["largest_cluster"] == 1
    ref = _check_mesh(gpu, v, [(2, 0, 1)], (2.0, 1.0, 1.0), what="two corners in one cell")
    assert ref.out_v.shape == (0, 3) and ref.out_f.shape == (0, 3) and ref.vertex_map.tolist() == [-1, -1, -1]
    assert ref.stats["degenerate_faces"] == 1 and ref.stats["largest_cluster"] == 2
    out = ops.decimate_mesh(torch.from_numpy(v).to(gpu), torch.tensor([[2, 0, 1]], dtype=torch.int32, device=gpu), torch.zeros(3, 3, device=gpu),
                            cell=(2.0, 1.0, 1.0))
    assert all(tuple(t.shape) == (0, 3) for t in out[:3]) and out[0].dtype == out[2].dtype == torch.float32 and out[1].dtype == torch.int32


# ---- 2. hand meshes for the coincidence rule
CORNERS = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5], [0.625, 0.75, 0.25], [1.25, 0.125, 0.875]], dtype=np.float32)


def test_the_coincidence_rule_by_hand(hip_lib, gpu):
    """Vertices 0 and 4 share a cell, 1 and 5 another."""
    ref = _check_mesh(gpu, CORNERS, [(0, 1, 2), (4, 2, 5)], 1.0, what="an opposite pair")
    assert ref.out_f.shape == (0, 3) and ref.stats["coincident_faces"] == 2 and (ref.vertex_map == -1).all()
    ref = _check_mesh(gpu, CORNERS, [(5, 2, 4), (0, 1, 2)], 1.0, what="a same-orientation pair")
    assert ref.out_f.tolist() == [[1, 2, 0]] and ref.stats["coincident_faces"] == 1 and ref.vertex_map.tolist() == [0, 1, 2, -1, 0, 1]
    ref = _check_mesh(gpu, CORNERS, [(0, 2, 1), (3, 1, 2), (1, 2, 4), (2, 0, 5), (2, 3, 1)], 1.0, what="two even and one odd")
    assert ref.out_f.tolist() == [[3, 1, 2], [1, 2, 0]] and ref.stats["coincident_faces"] == 3       # {1, 2, 3} twice the same way; {0, 1, 2} once odd, twice even
    # a closed strip of tetrahedra-like rings: apex, ring, ring, apex; the two rings fall pairwise into one cell each, so the band
    # between them collapses and a closed bipyramid is left
    ring = lambda z: [[np.cos(a), np.sin(a), z] for a in (0.1, 2.2, 4.3)]
    v = np.array([[0, 0, -1.5]] + ring(-0.2) + ring(0.2) + [[0, 0, 1.5]], dtype=np.float32)
    faces = [(0, 2, 1), (0, 3, 2), (0, 1, 3)] + [(1, 2, 4), (2, 5, 4), (2, 3, 5), (3, 6, 5), (3, 1, 6), (1, 4, 6)] + [(7, 4, 5), (7, 5, 6), (7, 6, 4)]
    assert R.mesh_report(v, _faces(faces))["closed"]
    ref = _check_mesh(gpu, v, faces, 1.0, (-3.5, -3.5, -0.5), what="a strip whose middle collapses")
    after = R.mesh_report(ref.out_v, ref.out_f)
    assert ref.stats["degenerate_faces"] == 6 and ref.out_v.shape == (5, 3) and ref.out_f.shape == (6, 3) and after["closed"] and after["chi"] == 2


# ---- 3. invalid inputs
def test_invalid_faces_and_unclustered_vertices(hip_lib, gpu):
    big = np.float32(2 ** 20)
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [big, 0.5, 0.5],
                  [-big, 0.5, 0.5], [np.nextafter(big, np.float32(0)), 0.5, 0.5], [np.nextafter(-big, -np.float32(np.inf)), 0.5, 0.5], [np.nan, 0.5, 0.5],
                  [0.5, 0.5, 3e38], [-0.5, -0.25, -1e-30], [-0.75, -0.5, -0.5], [-1.5, -1.0, -1.0], [-0.0, 0.0, 1.0]], dtype=np.float32)
    n = len(v)
    faces = [(0, 1, 2), (2, -1, 1), (0, 1, n), (-1, -1, -1), (0, 3, 1), (3, 10, 1), (4, 5, 0), (6, 7, 8), (9, 11, 2), (12, 13, 1), (12, 14, 15), (13, 14, 15),
             (2 ** 31 - 1, 0, 1), (-2 ** 31, 0, 1)]
    ref = _check_mesh(gpu, v, faces, 1.0, what="invalid and unclustered")
    st = ref.stats
    assert st["invalid_faces"] == 5 and st["unclustered_vertices"] == 7 and st["degenerate_faces"] == 1 and st["largest_cluster"] == 2
    assert st["kept_faces"] == 7 and st["coincident_faces"] == 1 and ref.vertex_map[12] == ref.vertex_map[13] >= 0                    # two negative corners in the cell (-1, -1, -1)
    kept_nan = ref.out_v[ref.vertex_map[3]]
    assert np.isnan(kept_nan[0]) and np.array_equal(_bits(kept_nan), _bits(v[3])) and ref.vertex_map[3] != ref.vertex_map[10]       # each NaN its own cluster
    _check_mesh(gpu, v, faces, (0.5, 2.0, 1e-3), (0.25, -0.125, 1e-4), what="invalid and unclustered, another lattice", fills=(0xFF,))


def test_negative_coordinates_with_the_default_origin(hip_lib, gpu):
    rng = np.random.default_rng(31)
    v = -np.abs(S.positions(400, seed=32)) * np.float32(2.0)
    faces = rng.integers(0, 400, size=(900, 3)).astype(np.int32)
    ref = _check_mesh(gpu, v, faces, 0.5, what="all negative")
    assert ref.stats["largest_cluster"] > 3 and 0 < ref.stats["kept_vertices"] < 400 and (v < 0).all()


# ---- 4. cluster sizes
def _one_cluster(n, seed):
    """n vertices in the cell (0, 0, 0) of the unit lattice behind three vertices in cells of their own; a fan of faces over the
    members -- they all become one triple, in one orientation -- and one more face, so that all four clusters are used."""
    rng = np.random.default_rng(seed)
    outside = np.array([[1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5]], dtype=np.float32)
    members = rng.random((n, 3), dtype=np.float32)
    if n > 3:
        members[1], members[2], members[3] = (0.0, 0.0, 0.0), np.nextafter(np.float32(1), np.float32(0)), (-0.0, 0.5, 0.25)
    k = np.arange(n, dtype=np.int32) + 3
    faces = np.concatenate([np.stack([np.zeros(n, np.int32), k, np.ones(n, np.int32)], axis=1), [[0, 1, 2]]]).astype(np.int32)
    return np.concatenate([outside, members]), faces[rng.permutation(len(faces))]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 256, 257])
def test_clusters_on_both_sides_of_a_wave_and_of_a_workgroup(hip_lib, gpu, n):
    v, f = _one_cluster(n, seed=n)
    ref = _check_mesh(gpu, v, f, 1.0, what=f"a cluster of {n}")
    assert ref.stats["largest_cluster"] == n and ref.stats["kept_vertices"] == 4 and ref.stats["kept_faces"] == 2 and ref.stats["coincident_faces"] == n - 1
    if n == 1:
        assert np.array_equal(_bits(ref.out_v[3]), _bits(v[3]))


def test_5000_vertices_in_one_cell(hip_lib, gpu):
    v, f = _one_cluster(5000, seed=50)
    ref = _check_mesh(gpu, v, f, 1.0, what="5000 in one cell")
    assert ref.stats["largest_cluster"] == 5000 and ref.stats["kept_vertices"] == 4 and ref.stats["coincident_faces"] == 4999
    assert np.abs(ref.out_v[3] - 0.5).max() < 0.02                   # the mean of uniform positions
    ref = _check_mesh(gpu, v * np.float32(0.37) - np.float32(3.0), f, 0.37, (-3.0, -3.0, -3.0), what="5000 in one cell, scaled", fills=(0xFF,))
    assert ref.stats["largest_cluster"] >= 4990


# ---- 5. table load 0.5
@pytest.mark.parametrize("n", [4096, 65536])
def test_tables_at_load_one_half(hip_lib, gpu, n):
    """n vertices, each in a cell of its own, and n faces with n distinct vertex sets: both tables hold 2 n slots."""
    ids = np.arange(n)
    v = np.stack([ids % 64, ids // 64 % 64, ids // 4096], axis=1).astype(np.float32) + np.float32(0.5)
    faces = np.stack([ids, (ids + 1) % n, (ids + 2) % n], axis=1).astype(np.int32)
    rng = np.random.default_rng(n)
    order = rng.permutation(n)
    ref = _check_mesh(gpu, v[order], faces[rng.permutation(n)], 1.0, what=f"load 0.5 at {n}", fills=(0xFF, (2,)), ops_normals=(True,))
    assert ref.stats["kept_vertices"] == n and ref.stats["kept_faces"] == n and ref.stats["largest_cluster"] == 1
    assert np.array_equal(ref.vertex_map, ids) and np.array_equal(_bits(ref.out_v), _bits(v[order]))


# ---- 6. block and scan-round edges
@pytest.mark.parametrize("n_vertices", [255, 256, 257])
def test_block_edges(hip_lib, gpu, n_vertices):
    for n_faces in (255, 256, 257):
        rng = np.random.default_rng(1000 * n_vertices + n_faces)
        v, f = D.random_mesh(rng, n_vertices, n_faces, cell=0.5, spread=1.0)
        f[-1] = (n_vertices - 1, 0, n_vertices // 2)                # the last face and the last vertex take part
        ref = _check_mesh(gpu, v, f, 0.5, what=f"V = {n_vertices}, F = {n_faces}", fills=(0xFF, (3,)), ops_normals=(False,))
        assert ref.stats["kept_faces"] > 0 and ref.stats["invalid_faces"] > 0


def test_past_a_scan_round_and_a_table_of_four_million_slots(hip_lib, gpu):
    """V = F = 2^20 + 257: 4,098 block sums per scan (a round takes 4,096), tables of 2^22 slots; random points over 70^3 cells."""
    n = (1 << 20) + 257
    rng = np.random.default_rng(77)
    v = (rng.random((n, 3), dtype=np.float32) * np.float32(70.0)).astype(np.float32) - np.float32(35.0)
    f = rng.integers(0, n, size=(n, 3)).astype(np.int32)
    f[-1], v[-1] = (n - 1, n - 2, n - 3), (100.5, 0.5, 0.5)
    ref = _check_mesh(gpu, v, f, 1.0, what="2^20 + 257", fills=((4,),), ops_normals=(False,))
    assert ref.stats["kept_faces"] > n // 2 and ref.stats["kept_vertices"] > 300000 and ref.vertex_map[-1] == ref.stats["kept_vertices"] - 1
    assert ref.out_f[-1, 0] == ref.stats["kept_vertices"] - 1 and ref.stats["largest_cluster"] >= 8


# ---- 7. isosurfaces
ISO_N, ISO_LO, ISO_HI, ISO_ORIGIN = (33, 33, 33), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (-1.03, -1.01, -1.02)


@pytest.mark.parametrize("field", ["sphere", "torus", "two_spheres", "noise_field"])
def test_isosurfaces(hip_lib, gpu, field):
    from nerf import ops
    if field == "noise_field":
        values, n = R.noise_field(n=ISO_N), ISO_N
    else:
        values, n = getattr(R, field)(*R.grid_points(ISO_LO, ISO_HI, ISO_N)), ISO_N
    v, f, _ = ops.isosurface(torch.from_numpy(np.ascontiguousarray(values)).to(gpu), 0.0, ISO_LO, ISO_HI)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert len(f) > 1000
    h = 2.0 / 32
    before = R.mesh_report(v, f)
    for k in (1, 2, 3.7, 8, 100):
        ref = _Reference(v, f, k * h, ISO_ORIGIN)
        _check_entry_points(gpu, ref, (field, k), ws_fill=(int(10 * k),))
        _check_ops(gpu, ref, (field, k), with_normals=True)
        _check_ops(gpu, ref, (field, k), with_normals=False)
        if field == "sphere":
            assert (ref.stats["kept_vertices"], ref.stats["kept_faces"]) == {1: (1753, 3504), 2: (515, 1026), 3.7: (164, 324), 8: (38, 72), 100: (0, 0)}[k]
        if k == 100:
            assert ref.stats["kept_faces"] == 0 and ref.stats["largest_cluster"] == len(v)
        elif field != "noise_field":
            assert R.mesh_report(ref.out_v, ref.out_f)["chi"] == before["chi"]


# ---- 8. repeatability and inputs
def test_two_calls_give_the_same_bits_on_any_workspace(hip_lib, gpu):
    rng = np.random.default_rng(5)
    v, f = D.random_mesh(rng, 1500, 2600, cell=0.4)
    ref = _Reference(v, f, 0.4, (0.1, -0.2, 0.3))
    assert ref.stats["coincident_faces"] > 0 and ref.stats["degenerate_faces"] > 0 and ref.stats["largest_cluster"] > 2 and ref.stats["kept_faces"] > 500
    first = _check_entry_points(gpu, ref, "seeded", wrong_sizes=True)
    for fill in (0xFF, (1,), (2,), 0x00, 0x5A):
        again = _check_entry_points(gpu, ref, "seeded", ws_fill=fill)
        assert all(np.array_equal(a, b) for a, b in zip(again, first)), fill
    a, b = _check_ops(gpu, ref, "seeded"), _check_ops(gpu, ref, "seeded")
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[:4], b[:4]))


def test_strided_inputs(hip_lib, gpu):
    rng = np.random.default_rng(6)
    v, f = D.random_mesh(rng, 700, 1300, cell=0.5)
    ref = _Reference(v, f, (0.5, 0.25, 1.0))
    _check_ops(gpu, ref, "strided", with_normals=True, strided=True)
    _check_ops(gpu, ref, "strided", with_normals=False, strided=True)


# ---- 9. the Python layers on a model's grid
def test_extract_mesh_with_decimate_is_decimate_mesh_of_extract_mesh(hip_lib, gpu, monkeypatch):
    import nerf
    from nerf import ops
    c = C.build_case("eval_det_64_128")
    m, expr, latent = U.make_model(nerf, c["p_coarse"], gpu).eval(), c["expr"].to(gpu), c["latent"].to(gpu)
    box = dict(lo=GRID_LO, hi=GRID_HI, resolution=GRID_N)
    level = float(nerf.density_grid(m, expr, latent, **box).median())
    plain = nerf.extract_mesh(m, expr, latent, level=level, largest=True, smooth=2, **box)
    assert plain.faces.shape[0] > 0
    for k in (1, 2.5):
        cell = [k * (h - l) / (n - 1) for l, h, n in zip(GRID_LO, GRID_HI, GRID_N)]
        direct = nerf.extract_mesh(m, expr, latent, level=level, largest=True, smooth=2, decimate=k, **box)
        after = nerf.decimate_mesh(plain, cell=cell, origin=GRID_LO)
        want = D.decimate(*[t.cpu().numpy() for t in plain[:2]], cell, GRID_LO, normals=True)
        assert isinstance(direct, nerf.Mesh) and isinstance(after, nerf.Mesh) and 0 < direct.faces.shape[0] < plain.faces.shape[0]
        for d, a, w in zip(direct, after, want[:3]):
            assert torch.equal(d, a) and d.dtype == a.dtype and np.array_equal(d.cpu().numpy().view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
    bare = nerf.extract_mesh(m, expr, latent, level=level, normals=False, decimate=2, **box)
    assert bare.normals is None and torch.equal(bare.vertices, nerf.decimate_mesh(nerf.extract_mesh(m, expr, latent, level=level, normals=False, **box),
                                                                                cell=[2 * (h - l) / (n - 1) for l, h, n in zip(GRID_LO, GRID_HI, GRID_N)],
                                                                                origin=GRID_LO).vertices)
    # decimate = None: today's path and today's bits, and nothing of the new code is called
    monkeypatch.setattr(ops, "decimate_mesh", lambda *a, **k: pytest.fail("decimate=None must not reach the decimation code"))
    again = nerf.extract_mesh(m, expr, latent, level=level, largest=True, smooth=2, decimate=None, **box)
    assert all(torch.equal(x, y) for x, y in zip(again, plain))


def test_launcher_with_decimate_and_colour_writes_the_decimated_ply(hip_lib, gpu, tmp_path, capsys):
    """launch.extract_mesh --decimate 2 --colour on the synthetic dataset and an untrained checkpoint at 24^3: the .ply holds as many
    vertices and faces as the returned statistics say, the colours are those of the written vertices, and the stats line is there."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synthetic_dataset as MS
    import nerf
    from launch import common as CM
    from launch import extract_mesh
    base = str(tmp_path)
    data = MS.write(os.path.join(base, "data"))
    cfg_path = os.path.join(base, "config.yml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(MS.config(data, os.path.join(base, "logs")), f)
    torch.manual_seed(7)
    cfg = CM.load_config(cfg_path)
    model_c, model_f = CM.build_models(cfg, gpu)
    ck_path = os.path.join(base, "untrained.ckpt")
    latents = torch.randn(6, 32) * 0.1
    torch.save({"model_coarse_state_dict": model_c.state_dict(), "model_fine_state_dict": model_f.state_dict(), "latent_codes": latents}, ck_path)
    _, poses, _, hwf, _, expressions, _, _ = nerf.load_flame_data(data, half_res=False, testskip=1, test=True)
    lo, hi = extract_mesh.frustum_box(int(hwf[0]), int(hwf[1]), hwf[2], poses[1, :3, :4].float().to(gpu), 0.2, 0.8)
    grid = nerf.density_grid(model_f.eval(), expressions[1].float().to(gpu), latents[1].to(gpu), lo=lo, hi=hi, resolution=24)
    level = float(grid.median())
    common = ["--config", cfg_path, "--checkpoint", ck_path, "--frame", "1", "--level", repr(level), "--resolution", "24", "--largest"]
    fine = os.path.join(base, "fine.ply")
    stats = extract_mesh.main(common + ["--out", fine])
    assert "decimated" not in capsys.readouterr().out and "decimate" not in stats
    rows, faces, _, _, _ = R.read_ply(fine)
    out = os.path.join(base, "light.ply")
    stats = extract_mesh.main(common + ["--out", out, "--decimate", "2", "--colour"])
    text = capsys.readouterr().out
    cell, origin = nerf.mesh.decimation_lattice(lo, hi, 24, 2.0)
    want = D.decimate(rows[:, :3], faces, cell, origin, normals=True)
    got_rows, got_faces, got_colours, props = K.read_ply(out)
    d = stats["decimate"]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"] and got_colours.shape == (d["kept_vertices"], 3)
    assert len(got_rows) == d["kept_vertices"] == stats["vertices"] == stats["colour"]["vertices"] and len(got_faces) == d["kept_faces"] == stats["faces"]
    assert d == want[4] and 0 < d["kept_faces"] < d["faces"] == len(faces) and d["vertices"] == len(rows)
    assert np.array_equal(got_faces, want[1]) and np.array_equal(_bits(got_rows[:, :3]), _bits(want[0])) and np.array_equal(_bits(got_rows[:, 3:]), _bits(want[2]))
    assert stats["colour"]["depth"] == pytest.approx(float(np.sqrt(sum(x * x for x in cell))))
    assert f"decimated: cells of 2 grid cells; vertices {d['kept_vertices']} of {d['vertices']}, faces {d['kept_faces']} of {d['faces']}" in text
