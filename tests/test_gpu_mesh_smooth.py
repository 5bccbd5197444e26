"""Mesh smoothing on the GPU: ops.mesh_adjacency / ops.smooth_mesh / ops.vertex_normals and the C entry points against
tests/mesh_smooth_ref.py.  Every float32 operation of the specification is one NumPy float32 operation there, in the same order, so
every comparison is array_equal on the bit patterns; the entry points write into buffers pre-filled with 0xFF and may not write a
byte more than the specification names.  Hand meshes, rows on both sides of the one-thread / one-wave threshold of the sort, sizes
past a workgroup and a scan round, isosurfaces of known fields, and the model-level functions.  GPU only."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from oracle import cases as C
from tests import isosurface_ref as R
from tests import mesh_smooth_ref as S
from tests import util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 40                       # entries every output buffer is longer than it needs to be
TAUBIN = dict(lam=0.5, mu=-0.53)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _faces(faces):
    return np.ascontiguousarray(np.asarray(faces, dtype=np.int32).reshape(-1, 3))


def _entry_points(gpu, vertices, faces, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True, ws_fill=0xFF, tmp=True):
    """adjacency, run and normals (of the smoothed positions, in the workspace the adjacency left) through the C ABI.  The workspace
    arrives filled with `ws_fill` (a byte, or a seed for random bytes) and lies 256 bytes inside its allocation; every output is
    filled with 0xFF and PAD entries longer than needed.  Returns host copies: row_start, neighbours, multiplicity (int32),
    boundary (uint8), counts (int64, one guard entry on either side), out and normals (as int32)."""
    from nerf import _hip as H
    lib = H.lib()
    n_vertices, n_faces = vertices.shape[0], faces.shape[0]
    poison = lambda n, dtype=torch.int32: torch.full((n,), -1, dtype=dtype, device=gpu)       # -1: every byte 0xFF
    ws_bytes = lib.nf_mesh_smooth_workspace_bytes(n_vertices, n_faces)
    assert ws_bytes >= 256
    if isinstance(ws_fill, tuple):
        ws = torch.from_numpy(np.random.default_rng(ws_fill[0]).integers(0, 256, size=ws_bytes + 512, dtype=np.uint8)).to(gpu)
    else:
        ws = torch.full((ws_bytes + 512,), ws_fill, dtype=torch.uint8, device=gpu)
    guard = (ws[:256].clone(), ws[256 + ws_bytes:].clone())
    assert ws.data_ptr() % 256 == 0
    d_v, d_f = torch.from_numpy(np.ascontiguousarray(vertices)).to(gpu), torch.from_numpy(faces).to(gpu)
    row_start, neighbours, multiplicity = poison(n_vertices + 1 + PAD), poison(6 * n_faces + PAD), poison(6 * n_faces + PAD)
    boundary = torch.full((n_vertices + PAD,), 0xFF, dtype=torch.uint8, device=gpu)
    counts = poison(2 + 2, torch.int64)
    stream = H.stream_ptr(gpu)
    H.check(lib.nf_mesh_smooth_adjacency(H.ptr(d_f), n_vertices, n_faces, ws.data_ptr() + 256, ws_bytes, H.ptr(row_start), H.ptr(neighbours),
                                         H.ptr(multiplicity), H.ptr(boundary), counts.data_ptr() + 8, stream), "adjacency")
    d_tmp, d_out, d_n = poison(3 * n_vertices + PAD), poison(3 * n_vertices + PAD), poison(3 * n_vertices + PAD)
    H.check(lib.nf_mesh_smooth_run(H.ptr(d_v), n_vertices, H.ptr(row_start), H.ptr(neighbours), H.ptr(boundary) if fix_boundary else None, iterations,
                                   lam, mu, H.ptr(d_tmp) if tmp else None, H.ptr(d_out), stream), "run")
    H.check(lib.nf_mesh_smooth_normals(H.ptr(d_out), H.ptr(d_f), n_vertices, n_faces, ws.data_ptr() + 256, ws_bytes, H.ptr(d_n), stream), "normals")
    torch.cuda.synchronize()
    assert torch.equal(ws[:256], guard[0]) and torch.equal(ws[256 + ws_bytes:], guard[1])
    assert bool((d_tmp[3 * n_vertices:] == -1).all())
    return [t.cpu().numpy() for t in (row_start, neighbours, multiplicity, boundary, counts, d_out, d_n)]


class _Reference:
    """The restatement's adjacency of a mesh, once, and its smoothed positions and normals per setting."""

    def __init__(self, vertices, faces):
        self.vertices, self.faces = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3), _faces(faces)
        self.n_vertices, self.n_faces = self.vertices.shape[0], self.faces.shape[0]
        self.row_start, self.neighbours, self.multiplicity, self.boundary = S.adjacency(self.faces, self.n_vertices)
        self.edges, self.n_boundary = len(self.neighbours), int(self.boundary.sum())
        self._smoothed = {}

    def smoothed(self, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True):
        key = (iterations, lam, mu, fix_boundary)
        if key not in self._smoothed:
            p, pinned = self.vertices, self.boundary if fix_boundary else None
            for _ in range(iterations):
                p = S.one_pass(p, self.row_start, self.neighbours, lam, pinned)
                if np.float32(mu) != 0:
                    p = S.one_pass(p, self.row_start, self.neighbours, mu, pinned)
            self._smoothed[key] = (p, S.vertex_normals(p, self.faces))
        return self._smoothed[key]


def _check_entry_points(gpu, ref, what, **setting):
    """The seven buffers of _entry_points equal the restatement up to their counts and hold 0xFF past them."""
    fix = {k: setting.pop(k) for k in ("ws_fill", "tmp") if k in setting}
    got = _entry_points(gpu, ref.vertices, ref.faces, **setting, **fix)
    row_start, neighbours, multiplicity, boundary, counts, out, normals = got
    v, e = ref.n_vertices, ref.edges
    assert np.array_equal(row_start[:v + 1], ref.row_start) and (row_start[v + 1:] == -1).all(), what
    assert np.array_equal(neighbours[:e], ref.neighbours) and (neighbours[e:] == -1).all() and len(neighbours) - e >= PAD, what
    assert np.array_equal(multiplicity[:e], ref.multiplicity) and (multiplicity[e:] == -1).all(), what
    assert np.array_equal(boundary[:v], ref.boundary) and (boundary[v:] == 0xFF).all(), what
    assert counts.tolist() == [-1, e, ref.n_boundary, -1], (what, counts)
    want_v, want_n = ref.smoothed(**setting)
    assert np.array_equal(out[:3 * v].view(np.uint32), _bits(want_v).reshape(-1)) and (out[3 * v:] == -1).all(), (what, setting)
    assert np.array_equal(normals[:3 * v].view(np.uint32), _bits(want_n).reshape(-1)) and (normals[3 * v:] == -1).all(), (what, setting)
    return got


def _check_ops(gpu, ref, what, with_normals=True, **setting):
    """ops.mesh_adjacency, ops.smooth_mesh and ops.vertex_normals equal the restatement; returns the smoothed device mesh."""
    from nerf import ops
    d_v, d_f = torch.from_numpy(ref.vertices).to(gpu), torch.from_numpy(ref.faces).to(gpu)
    adjacency = ops.mesh_adjacency(d_f, ref.n_vertices)
    assert isinstance(adjacency, ops.MeshAdjacency)
    for name, g, w in zip(adjacency._fields, adjacency, (ref.row_start, ref.neighbours, ref.multiplicity, ref.boundary)):
        assert g.is_cuda and g.dtype == (torch.uint8 if name == "boundary" else torch.int32) and g.dim() == 1, (what, name)
        assert tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w), (what, name)
    want_v, want_n = ref.smoothed(**setting)
    got = ops.smooth_mesh(d_v, d_f, torch.full_like(d_v, 7.0) if with_normals else None, **setting)
    assert got[0].dtype == torch.float32 and got[0].is_cuda and tuple(got[0].shape) == (ref.n_vertices, 3) and got[1] is d_f, what
    assert np.array_equal(_bits(got[0].cpu().numpy()), _bits(want_v)), (what, setting)
    if with_normals:
        assert tuple(got[2].shape) == (ref.n_vertices, 3) and np.array_equal(_bits(got[2].cpu().numpy()), _bits(want_n)), (what, setting)
        assert torch.equal(ops.vertex_normals(got[0], d_f).view(torch.int32), got[2].view(torch.int32)), what
    else:
        assert got[2] is None
    mu = setting.get("mu", -0.53)
    fixed = setting.get("fix_boundary", True)
    assert isinstance(got[3], ops.MeshSmoothStats), what
    assert got[3] == (ref.edges, ref.n_boundary, ref.n_boundary if fixed else 0, setting.get("iterations", 10) * (2 if mu != 0 else 1)), (what, got[3])
    return got


def _check_mesh(gpu, vertices, faces, what, settings=(dict(iterations=1), dict(iterations=2, fix_boundary=False), dict(iterations=2, mu=0.0))):
    ref = _Reference(vertices, faces)
    for k, setting in enumerate(settings):
        _check_entry_points(gpu, ref, what, **setting)
        _check_ops(gpu, ref, what, with_normals=k != 1, **setting)
    return ref


# ---- 1. hand meshes
HAND = {
    "nothing": (0, []),
    "five vertices, no face": (5, []),
    "faces over no vertex": (0, [(0, 0, 0), (0, 1, 2)]),
    "one triangle": (3, [(2, 0, 1)]),
    "two triangles on a shared edge": (4, [(0, 1, 2), (2, 1, 3)]),
    "a closed tetrahedron": (4, [(0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3)]),
    "a repeated index": (4, [(1, 1, 3)]),
    "all three the same": (3, [(2, 2, 2)]),
    "faces holding -1 and V": (6, [(0, 1, 2), (2, -1, 3), (3, 4, 6), (4, 5, 4), (6, 6, 6), (-1, -1, -1)]),
    "a face listed twice": (3, [(0, 1, 2), (0, 1, 2)]),
    "unused vertices": (10, [(7, 8, 9), (0, 1, 2), (2, 1, 5)]),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_meshes(hip_lib, gpu, name):
    n_vertices, faces = HAND[name]
    vertices = S.positions(n_vertices, seed=3)
    ref = _check_mesh(gpu, vertices, faces, name)
    expect = {"nothing": ([0], [], []), "five vertices, no face": ([0] * 6, [], [0] * 5), "faces over no vertex": ([0], [], []),
              "one triangle": ([0, 2, 4, 6], [1, 2, 0, 2, 0, 1], [1, 1, 1]),
              "two triangles on a shared edge": ([0, 2, 5, 8, 10], [1, 2, 0, 2, 3, 0, 1, 3, 1, 2], [1, 1, 1, 1]),
              "a closed tetrahedron": ([0, 3, 6, 9, 12], [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2], [0, 0, 0, 0]),
              "a repeated index": ([0, 0, 1, 1, 2], [3, 1], [0, 0, 0, 0]), "all three the same": ([0, 0, 0, 0], [], [0, 0, 0]),
              "faces holding -1 and V": ([0, 2, 4, 6, 6, 7, 8], [1, 2, 0, 2, 0, 1, 5, 4], [1, 1, 1, 0, 0, 0]),
              "a face listed twice": ([0, 2, 4, 6], [1, 2, 0, 2, 0, 1], [0, 0, 0]),
              "unused vertices": ([0, 2, 5, 8, 8, 8, 10, 10, 12, 14, 16], [1, 2, 0, 2, 5, 0, 1, 5, 1, 2, 8, 9, 7, 9, 7, 8],
                                  [1, 1, 1, 0, 0, 1, 0, 1, 1, 1])}[name]
    assert ref.row_start.tolist() == expect[0] and ref.neighbours.tolist() == expect[1] and ref.boundary.tolist() == expect[2]
    if name == "a face listed twice":
        assert ref.multiplicity.tolist() == [2] * 6
    if name == "a repeated index":
        assert ref.multiplicity.tolist() == [2, 2]


def test_one_triangle_stays_under_fix_boundary_and_moves_without(hip_lib, gpu):
    from nerf import ops
    vertices = S.positions(3, seed=5)
    d_v, d_f = torch.from_numpy(vertices).to(gpu), torch.tensor([[2, 0, 1]], dtype=torch.int32, device=gpu)
    fixed, _, normals, stats = ops.smooth_mesh(d_v, d_f, torch.zeros_like(d_v))
    assert torch.equal(fixed.view(torch.int32), d_v.view(torch.int32)) and fixed.data_ptr() != d_v.data_ptr() and stats == (6, 3, 3, 20)
    assert np.array_equal(_bits(normals.cpu().numpy()), _bits(S.vertex_normals(vertices, [[2, 0, 1]])))
    free, _, none, stats = ops.smooth_mesh(d_v, d_f, iterations=1, fix_boundary=False)
    assert none is None and stats == (6, 3, 0, 2) and not bool((free == d_v).any())
    assert np.array_equal(_bits(free.cpu().numpy()), _bits(S.smooth(vertices, [[2, 0, 1]], 1, fix_boundary=False)))
    twice, _, _, stats = ops.smooth_mesh(d_v, torch.tensor([[2, 0, 1], [2, 0, 1]], dtype=torch.int32, device=gpu), iterations=1)
    assert stats == (6, 0, 0, 2) and torch.equal(twice.view(torch.int32), free.view(torch.int32))       # the same neighbours, and no boundary
    same = ops.smooth_mesh(d_v, d_f, d_v, iterations=0)
    assert same[0] is d_v and same[1] is d_f and same[2] is d_v and same[3] == (0, 0, 0, 0)


# ---- 2. row paths: one thread up to SHORT_ROW entries of the unsorted row, one wave past it
def test_the_threshold_above_is_the_kernels_own():
    from nerf import ops
    shared, unit = (open(os.path.join(ROOT, "4d-facial-avatars_amd", "csrc", f)).read() for f in ("nf_scan_dev.h", "nf_mesh_smooth.hip"))
    assert f"constexpr int SHORT_ROW = {ops.MESH_SMOOTH_SHORT_ROW};" in unit and "constexpr int THREADS = 256;" in shared
    assert "constexpr int SCAN_THREADS = 1024;" in shared and "constexpr int SCAN_PER_THREAD = 4;" in unit and ops.MESH_SMOOTH_SHORT_ROW % 2 == 0


@pytest.mark.parametrize("order", ["ascending", "descending", "permuted"])
def test_fans_on_both_sides_of_the_row_threshold_and_of_a_wave(hip_lib, gpu, order):
    """Fans round a hub of n neighbours.  The hub's unsorted row holds 2 (n - 1) entries in an open fan and 2 n in a closed one (every
    neighbour twice but the two ends), its row of faces n - 1 or n: n = T/2 .. T/2 + 2 puts the first at T - 2, T, T + 2 entries,
    n = T - 1 .. T + 2 the second at T - 2 .. T + 2, and 63, 64, 65 are the sizes round one wave's chunk of the rank sort.  Hub
    first and last, rim ids along the fan ascending, descending and permuted: fill order and sorted order differ."""
    from nerf import ops
    t = ops.MESH_SMOOTH_SHORT_ROW
    sizes = sorted({t // 2 - 1, t // 2, t // 2 + 1, t // 2 + 2, t - 1, t, t + 1, t + 2, 63, 64, 65, 2 * t + 1})
    for n in sizes:
        for k, (hub, closed) in enumerate((("first", False), ("last", True), ("last", False), ("first", True))):
            if k >= 2 and n not in (t // 2, t // 2 + 1, t, t + 1, 64):
                continue
            n_vertices, faces = S.fan(n, hub, order, closed, seed=n)
            ref = _check_mesh(gpu, S.positions(n_vertices, seed=n), faces, f"fan of {n}, hub {hub}, {order}, closed {closed}",
                              settings=(dict(iterations=2, fix_boundary=False),))
            centre = 0 if hub == "first" else n_vertices - 1
            # a closed fan is a disc: its rim is the boundary, its hub is not
            assert ref.row_start[centre + 1] - ref.row_start[centre] == n and ref.n_boundary == (n if closed else n_vertices)
            assert ref.boundary[centre] == (0 if closed else 1)


@pytest.mark.parametrize("order", ["ascending", "descending", "permuted"])
@pytest.mark.parametrize("hub", ["first", "last"])
def test_a_fan_of_3000_faces(hip_lib, gpu, hub, order):
    """One row of 5,998 unsorted entries (94 chunks of the rank sort, every neighbour but two twice) and one of 2,999 faces."""
    n_vertices, faces = S.fan(3000, hub, order, seed=9)
    ref = _check_mesh(gpu, S.positions(n_vertices, seed=11), faces, f"fan of 3000, hub {hub}, {order}",
                      settings=(dict(iterations=1, fix_boundary=False), dict(iterations=1)))
    assert ref.edges == 2 * (3000 + 2999) and ref.n_boundary == n_vertices and int((ref.multiplicity == 2).sum()) == 2 * 2998


# ---- 3. sizes
@pytest.mark.parametrize("order", ["ascending", "descending", "permuted"])
def test_a_strip_past_a_workgroup_and_a_wave(hip_lib, gpu, order):
    n = 4099
    rng = np.random.default_rng(17)
    ids = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "permuted": rng.permutation(n)}[order]
    at = np.arange(n - 2)
    faces = np.stack([ids[at], ids[at + 1], ids[at + 2]], axis=1).astype(np.int32)
    if order == "permuted":
        faces = faces[rng.permutation(len(faces))]
    ref = _check_mesh(gpu, S.positions(n, seed=2), faces, f"strip {order}", settings=(dict(iterations=2, fix_boundary=False), dict(iterations=1)))
    assert ref.n_boundary == n and ref.edges == 2 * (2 * n - 3)


def test_triangles_across_block_and_scan_round_boundaries(hip_lib, gpu):
    """1,025 triangles, one every 1,024 vertices on the vertices 254, 255, 256 of their stretch (each straddles a workgroup boundary),
    every other vertex unused: V = 2^20 + 300 is past what one round of the scan of the block sums takes."""
    n_tri, stride = 1025, 1024
    base = np.arange(n_tri, dtype=np.int64) * stride + 254
    n_vertices = int(base[-1]) + 46
    assert n_vertices == (1 << 20) + 300
    faces = np.stack([base + 2, base, base + 1], axis=1).astype(np.int32)[::-1].copy()
    ref = _check_mesh(gpu, S.positions(n_vertices, seed=4), faces, "1025 triangles", settings=(dict(iterations=1, fix_boundary=False),))
    assert ref.edges == 6 * n_tri and ref.n_boundary == 3 * n_tri and ref.row_start[-1] == 6 * n_tri


# ---- 4. isosurface meshes
def _isosurface(gpu, field, lo, hi):
    from nerf import ops
    v, f, _ = ops.isosurface(torch.from_numpy(np.ascontiguousarray(field)).to(gpu), 0.0, lo, hi)
    return v.cpu().numpy(), f.cpu().numpy()


ISO_SETTINGS = (dict(iterations=1), dict(iterations=2), dict(iterations=10), dict(iterations=10, mu=0.0))


def test_the_closed_sphere(hip_lib, gpu):
    v, f = _isosurface(gpu, R.sphere(*R.grid_points(R.BOX_LO, R.BOX_HI, R.BOX_N)), R.BOX_LO, R.BOX_HI)
    ref = _check_mesh(gpu, v, f, "sphere", settings=ISO_SETTINGS)
    assert ref.n_boundary == 0 and ref.edges == 3 * len(f) and (ref.multiplicity == 2).all() and len(f) > 1000
    radius = lambda p: np.linalg.norm(p.astype(np.float64), axis=1).mean()
    taubin, laplace = ref.smoothed(iterations=10)[0], ref.smoothed(iterations=10, mu=0.0)[0]
    assert abs(radius(taubin) / radius(v) - 1) < 2e-3 and radius(laplace) < 0.99 * radius(v)


def test_a_sphere_the_box_cuts_keeps_its_cut(hip_lib, gpu):
    from nerf import ops
    v, f = _isosurface(gpu, R.sphere(*R.grid_points(R.BOX_LO, R.BOX_HI, R.BOX_N), r=1.3), R.BOX_LO, R.BOX_HI)
    ref = _check_mesh(gpu, v, f, "sphere r = 1.3 cut by the box", settings=ISO_SETTINGS)
    pinned = ref.boundary == 1
    assert 0 < ref.n_boundary < len(v)
    out = ops.smooth_mesh(torch.from_numpy(v).to(gpu), torch.from_numpy(f).to(gpu))
    assert out[3].pinned_vertices == ref.n_boundary
    got = out[0].cpu().numpy()
    assert np.array_equal(_bits(got[pinned]), _bits(v[pinned])) and (_bits(got[~pinned]) != _bits(v[~pinned])).any(axis=1).mean() > 0.9
    ends = np.stack([R._axis(R.BOX_LO[a], R.BOX_HI[a], R.BOX_N[a])[0][[0, -1]] for a in range(3)], axis=1)       # the grid's first and last coordinates
    on_box = lambda p: ((p == ends[0]) | (p == ends[1])).any(axis=1)
    assert on_box(v[pinned]).all() and not on_box(v[~pinned]).any()                    # the boundary vertices are those on the box's faces


def test_the_noisy_sphere_of_the_host_test(hip_lib, gpu):
    lo, hi, n = (-1, -1, -1), (1, 1, 1), (24, 24, 24)
    field = S.radial_sphere(*R.grid_points(lo, hi, n))
    field = (field + 0.03 * np.random.default_rng(7).standard_normal(field.shape)).astype(np.float32)
    v, f = _isosurface(gpu, field, lo, hi)
    ref = _check_mesh(gpu, v, f, "noisy sphere", settings=ISO_SETTINGS)
    spread = lambda p: np.linalg.norm(p.astype(np.float64), axis=1).std()
    assert spread(ref.smoothed(iterations=10)[0]) <= 0.9 * spread(v)


# ---- 5. the entry points directly
def test_entry_points_repeat_bit_for_bit_on_any_workspace(hip_lib, gpu):
    """Seeded faces (some invalid, some with repeated indices, some listed twice) over 1,500 vertices, the outputs exactly 6 F entries
    plus the guard: two calls give the same bits; a workspace of random bytes, of zeros or of 0x5A gives the bits of the one filled
    with 0xFF; the single pass of iterations = 1, mu = 0 needs no tmp."""
    from tests import mesh_components_ref as M
    n_vertices, n_faces = 1500, 2600
    rng = np.random.default_rng(5)
    faces = M.random_faces(rng, n_vertices, n_faces)
    faces[rng.integers(0, n_faces, 300)] = faces[rng.integers(0, n_faces, 300)]
    ref = _Reference(S.positions(n_vertices, seed=6), faces)
    assert 0 < ref.n_boundary < n_vertices and (ref.multiplicity > 2).any() and (np.diff(ref.row_start) == 0).any() and ref.edges < 6 * n_faces - 100
    first = _check_entry_points(gpu, ref, "seeded", iterations=3)
    for fill in (0xFF, (1,), (2,), 0x00, 0x5A):
        again = _check_entry_points(gpu, ref, "seeded", iterations=3, ws_fill=fill)
        assert all(np.array_equal(a, b) for a, b in zip(again, first)), fill
    _check_entry_points(gpu, ref, "seeded", iterations=1, mu=0.0, tmp=False)
    _check_entry_points(gpu, ref, "seeded", iterations=3, fix_boundary=False, lam=1.0, mu=-1.0)
    _check_ops(gpu, ref, "seeded", iterations=3)


def test_iterations_zero_through_the_entry_point_is_a_copy(hip_lib, gpu):
    from nerf import _hip as H
    lib = H.lib()
    v = torch.from_numpy(S.positions(300, seed=8)).to(gpu)
    out = torch.full((300 * 3 + PAD,), -1, dtype=torch.int32, device=gpu)
    H.check(lib.nf_mesh_smooth_run(H.ptr(v), 300, None, None, None, 0, 0.5, -0.53, None, H.ptr(out), H.stream_ptr(gpu)), "run")
    torch.cuda.synchronize()
    assert torch.equal(out[:900], v.view(torch.int32).reshape(-1)) and bool((out[900:] == -1).all())


# ---- 6. the Python layer on a model's grid
GRID_N, GRID_LO, GRID_HI = (17, 13, 11), (-0.4, -0.35, -0.3), (0.35, 0.4, 0.4)       # the grid of tests/test_gpu_isosurface.py's model tests


def test_extract_mesh_with_smooth_is_smooth_mesh_of_extract_mesh(hip_lib, gpu, monkeypatch):
    import nerf
    from nerf import ops
    c = C.build_case("eval_det_64_128")
    m, expr, latent = U.make_model(nerf, c["p_coarse"], gpu).eval(), c["expr"].to(gpu), c["latent"].to(gpu)
    box = dict(lo=GRID_LO, hi=GRID_HI, resolution=GRID_N)
    level = float(nerf.density_grid(m, expr, latent, **box).median())
    largest = nerf.extract_mesh(m, expr, latent, level=level, largest=True, **box)
    assert largest.faces.shape[0] > 0
    direct = nerf.extract_mesh(m, expr, latent, level=level, largest=True, smooth=3, **box)
    after = nerf.smooth_mesh(largest, iterations=3)
    want = S.smooth_mesh(*[t.cpu().numpy() for t in largest], iterations=3)
    assert isinstance(direct, nerf.Mesh) and isinstance(after, nerf.Mesh) and len(direct) == 3
    for d, a, w in zip(direct, after, want[:3]):
        assert torch.equal(d, a) and np.array_equal(d.cpu().numpy().view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
    assert torch.equal(nerf.vertex_normals(direct).view(torch.int32), direct.normals.view(torch.int32))
    assert not torch.equal(direct.vertices, largest.vertices) and not torch.equal(direct.normals, largest.normals)
    other = nerf.extract_mesh(m, expr, latent, level=level, min_faces=1, normals=False, smooth=2, smooth_lam=0.6, smooth_mu=0.0, **box)
    plain = nerf.extract_mesh(m, expr, latent, level=level, **box)
    assert other.normals is None and torch.equal(other.vertices, nerf.smooth_mesh(nerf.filter_mesh(plain, min_faces=1), iterations=2, lam=0.6, mu=0.0).vertices)
    # smooth = 0: today's path and today's bits, and nothing of the new code is called
    for name in ("smooth_mesh", "vertex_normals", "mesh_adjacency", "_adjacency", "_vertex_normals", "_mesh_smooth_workspace"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("smooth=0 must not reach the smoothing code"))
    again = nerf.extract_mesh(m, expr, latent, level=level, smooth=0, **box)
    grid = nerf.density_grid(m, expr, latent, **box)
    today = ops.isosurface(grid, level, GRID_LO, GRID_HI, normals=True)
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(again, plain, today))


def test_launcher_with_smooth_writes_the_smoothed_ply(hip_lib, gpu, tmp_path, capsys):
    """launch.extract_mesh --largest --smooth 3 on the synthetic dataset and an untrained checkpoint at 24^3: the .ply holds the
    smoothed positions and the recomputed normals of the mesh the launcher writes with --largest alone, and the stats line is there."""
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
    rough = os.path.join(base, "rough.ply")
    stats = extract_mesh.main(common + ["--out", rough])
    assert "smoothed" not in capsys.readouterr().out and "smooth" not in stats
    rows, faces, _, _, _ = R.read_ply(rough)
    out = os.path.join(base, "smooth.ply")
    stats = extract_mesh.main(common + ["--out", out, "--smooth", "3"])
    text = capsys.readouterr().out
    want = S.smooth_mesh(rows[:, :3], faces, rows[:, 3:], iterations=3)
    got_rows, got_faces, props, _, _ = R.read_ply(out)
    assert props == ["x", "y", "z", "nx", "ny", "nz"] and np.array_equal(got_faces, faces) and len(faces) > 0
    assert np.array_equal(_bits(got_rows[:, :3]), _bits(want[0])) and np.array_equal(_bits(got_rows[:, 3:]), _bits(want[2]))
    assert stats["smooth"] == want[3] and (_bits(got_rows[:, :3]) != _bits(rows[:, :3])).any()
    assert f"smoothed: 3 iterations (lambda 0.5, mu -0.53) in 6 passes over {want[3]['edges'] // 2} edges; {want[3]['pinned_vertices']} boundary vertices" in text
    stats = extract_mesh.main(common + ["--out", out, "--smooth", "2", "--smooth-lambda", "0.6", "--smooth-mu", "0"])
    capsys.readouterr()
    got_rows = R.read_ply(out)[0]
    assert stats["smooth"]["passes"] == 2 and np.array_equal(_bits(got_rows[:, :3]), _bits(S.smooth(rows[:, :3], faces, 2, 0.6, 0.0)))
