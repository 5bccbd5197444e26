"""Sparse density grids on the GPU: ops.sparse_grid against tests/sparse_grid_ref.py (torch.equal: the analytic functions are torch
elementwise operations, so a point has the same bits whether it is evaluated with the dense grid or alone), the mesh guarantee, how
the function is called, the C entry points on poisoned buffers, and the model-level functions (nerf.density_grid_sparse,
nerf.extract_mesh(brick=), launch.extract_mesh --brick).  Everything the library's output is compared with -- masks, counts, the
expected grid -- comes from the test's own dense grid.  GPU only."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from oracle import cases as C
from oracle import nerface_oracle as O
from tests import isosurface_ref as R
from tests import sparse_grid_ref as S
from tests import util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _points(gpu, lo, hi, n):
    """(nx * ny * nz, 3) device tensor of the grid points of nerf.mesh.grid_axes, x fastest."""
    import nerf
    xs, ys, zs = nerf.mesh.grid_axes(lo, hi, n)
    z, y, x = np.meshgrid(zs, ys, xs, indexing="ij")
    return torch.from_numpy(np.stack([x, y, z], axis=-1).reshape(-1, 3)).to(gpu)


def _ball(centre, r):
    return lambda pts: S.sphere_field(pts[:, 0], pts[:, 1], pts[:, 2], centre=centre, r=r)


def _torus(pts):
    return S.torus_field(pts[:, 0], pts[:, 1], pts[:, 2])


def _dense(gpu, fn, lo, hi, n):
    return fn(_points(gpu, lo, hi, n)).view(n[2], n[1], n[0])


def _check_against_the_restatement(gpu, fn, level, lo, hi, n, brick, what, **kw):
    """ops.sparse_grid == the restatement of the test's own dense grid: the grid torch.equal, the five counts equal."""
    from nerf import ops
    want = S.restate(_dense(gpu, fn, lo, hi, n).cpu().numpy(), level, brick, **kw)
    grid, stats = ops.sparse_grid(fn, level, lo, hi, n, brick=brick, **kw)
    assert grid.shape == (n[2], n[1], n[0]) and grid.dtype == torch.float32 and grid.is_cuda
    print(f"{what}: {stats}")
    assert stats == (want.seed.size, int(want.seed.sum()), int(want.active.sum()), n[0] * n[1] * n[2], int(want.evaluated.sum())), (what, stats)
    assert not np.isnan(want.grid).any() and torch.equal(grid.cpu(), torch.from_numpy(want.grid)), what
    return want, grid, stats


# (nx, ny, nz), brick: two bricks per axis; short last bricks on three different axis lengths; one brick; a brick larger than the
# grid; the smallest brick
SHAPES = [((17, 17, 17), 8), ((19, 13, 10), 4), ((9, 9, 9), 8), ((9, 9, 9), 16), ((12, 12, 12), 2)]


@pytest.mark.parametrize("n,brick", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"B{v}")
@pytest.mark.parametrize("dilate", [0, 1])
def test_grid_against_the_restatement(hip_lib, gpu, n, brick, dilate):
    """A ball of radius 1 round the lower corner of the isosurface tests' box: that corner is inside and the others are outside, so
    even the single brick of 9^3 is a seed, and with more bricks some have no crossing corner pair.  Then two fields without any
    seed: all outside (-inf beside the lattice) and all inside (+inf)."""
    want, _, _ = _check_against_the_restatement(gpu, _ball(R.BOX_LO, 1.0), 0.0, R.BOX_LO, R.BOX_HI, n, brick, f"ball {n} B={brick}", dilate=dilate)
    assert want.seed.any()
    if dilate == 0 and want.seed.size > 1:
        assert not want.active.all() and not want.evaluated.all()
    for sign in (-1.0, 1.0):
        none, grid, stats = _check_against_the_restatement(gpu, lambda pts: pts[:, 0] * 0.0 + sign, 0.0, R.BOX_LO, R.BOX_HI, n, brick,
                                                           f"constant {sign} {n} B={brick}", dilate=dilate)
        assert stats.seed_bricks == 0 and stats.active_bricks == 0 and stats.evaluated_points == int(none.lattice.sum())
        assert bool((grid[torch.from_numpy(~none.lattice).to(gpu)] == sign * float("inf")).all())


@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_most_bricks_stay_inactive_round_a_small_ball(hip_lib, gpu, dilate):
    """33^3 in bricks of 8 (4 per axis): 8 seeds round one brick corner; 8, 27 and all 64 bricks active at dilate 0, 1 and 2.  A
    margin of 0.05 adds the bricks whose corners come that near the level; a margin above every corner value makes all bricks seeds."""
    fn = _ball(S.SPHERE["centre"], S.SPHERE["r"])
    want, _, stats = _check_against_the_restatement(gpu, fn, 0.0, S.FIELD_LO, S.FIELD_HI, S.FIELD_N, S.FIELD_BRICK, f"small ball dilate {dilate}",
                                                    dilate=dilate)
    assert (stats.seed_bricks, stats.active_bricks) == (8, (8, 27, 64)[dilate])
    if dilate == 1:
        _check_against_the_restatement(gpu, fn, 0.0, S.FIELD_LO, S.FIELD_HI, S.FIELD_N, S.FIELD_BRICK, "small ball margin 0.05", margin=0.05)
        _, _, all_seeds = _check_against_the_restatement(gpu, fn, 0.0, S.FIELD_LO, S.FIELD_HI, S.FIELD_N, S.FIELD_BRICK, "small ball margin 10", margin=10.0)
        assert all_seeds.seed_bricks == 64


def test_nan_and_level_corners_make_seeds_on_the_device(hip_lib, gpu):
    """One lattice corner of an all-inside field set to NaN, and to the level itself: its bricks are seeds (NaN compares false
    both ways; == level is neither above nor below at margin 0)."""
    from nerf import ops
    n, lo, hi = (17, 17, 17), (0.0, 0.0, 0.0), (16.0, 16.0, 16.0)              # the coordinates are the indices
    for value in (float("nan"), 0.0):
        def fn(pts):
            at_corner = (pts[:, 0] == 16.0) & (pts[:, 1] == 8.0) & (pts[:, 2] == 0.0)
            return torch.where(at_corner, torch.full_like(pts[:, 0], value), torch.ones_like(pts[:, 0]))
        grid, stats = ops.sparse_grid(fn, 0.0, lo, hi, n, brick=8, dilate=0)
        want = S.restate(_dense(gpu, fn, lo, hi, n).cpu().numpy(), 0.0, 8, dilate=0)
        assert want.seed.sum() == 2 and (stats.seed_bricks, stats.active_bricks, stats.evaluated_points) == (2, 2, int(want.evaluated.sum()))
        assert torch.equal(torch.nan_to_num(grid.cpu(), nan=-7.0), torch.from_numpy(np.nan_to_num(want.grid, nan=-7.0)))
        assert bool(torch.isinf(grid).any())


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_the_sparse_grid_gives_the_dense_mesh(hip_lib, gpu, name):
    """ops.isosurface on the sparse grid == on the dense grid, vertices, faces and normals torch.equal, with the precondition (every
    brick that is no seed lies on one side) asserted from the dense grid and a quarter of the grid never evaluated."""
    from nerf import ops
    fn = _ball(S.SPHERE["centre"], S.SPHERE["r"]) if name == "sphere" else _torus
    dense = _dense(gpu, fn, S.FIELD_LO, S.FIELD_HI, S.FIELD_N)
    want = S.restate(dense.cpu().numpy(), 0.0, S.FIELD_BRICK)
    assert S.one_sided(dense.cpu().numpy(), 0.0, S.FIELD_BRICK, want.seed)
    grid, stats = ops.sparse_grid(fn, 0.0, S.FIELD_LO, S.FIELD_HI, S.FIELD_N, brick=S.FIELD_BRICK)
    assert stats.active_bricks <= 48 and stats.evaluated_points < 0.8 * stats.points and bool(torch.isinf(grid).any())
    a, b = ops.isosurface(dense, 0.0, S.FIELD_LO, S.FIELD_HI, normals=True), ops.isosurface(grid, 0.0, S.FIELD_LO, S.FIELD_HI, normals=True)
    assert a[1].shape[0] > 1000 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert bool(torch.isfinite(b[0]).all()) and bool(torch.isfinite(b[2]).all())


def test_how_the_function_is_called(hip_lib, gpu):
    """chunk_points = 1000 on the small ball's 33^3 grid in bricks of 8 (125 lattice points, 15561 others): no call takes more than 1000 points; the lattice comes first and the other
    points after it, each in ascending linear index; no point twice; the points are exactly the restatement's evaluated set; every
    coordinate has the bits of the grid_axes point of its index."""
    from nerf import ops
    n, brick, lo, hi = S.FIELD_N, S.FIELD_BRICK, S.FIELD_LO, S.FIELD_HI
    field = _ball(S.SPHERE["centre"], S.SPHERE["r"])
    calls = []

    def fn(pts):
        assert pts.is_cuda and pts.dtype == torch.float32 and pts.dim() == 2 and pts.shape[1] == 3 and pts.is_contiguous()
        calls.append(pts.clone())
        return field(pts)

    _, stats = ops.sparse_grid(fn, 0.0, lo, hi, n, brick=brick, chunk_points=1000)
    table = _points(gpu, lo, hi, n)
    want = S.restate(field(table).view(n[2], n[1], n[0]).cpu().numpy(), 0.0, brick)
    assert all(0 < c.shape[0] <= 1000 for c in calls) and sum(c.shape[0] == 1000 for c in calls) >= 2
    seen = torch.cat(calls).cpu().numpy()
    assert seen.shape[0] == stats.evaluated_points == int(want.evaluated.sum())
    import nerf
    axes = nerf.mesh.grid_axes(lo, hi, n)
    ijk = [np.searchsorted(axes[a], seen[:, a]) for a in range(3)]
    assert all((ijk[a] < n[a]).all() and np.array_equal(axes[a][ijk[a]], seen[:, a]) for a in range(3))      # exact bits of the axis values
    index = (ijk[2] * n[1] + ijk[1]) * n[0] + ijk[0]
    n_lattice = int(want.lattice.sum())
    assert np.array_equal(index[:n_lattice], np.flatnonzero(want.lattice.reshape(-1)))
    assert (np.diff(index[n_lattice:]) > 0).all() and np.unique(index).size == index.size
    assert np.array_equal(np.sort(index), np.flatnonzero(want.evaluated.reshape(-1)))
    assert torch.equal(torch.from_numpy(seen), table.cpu()[torch.from_numpy(index)])
    # the lattice alone takes 5^3 = 125 points: the first call is the lattice, the second starts the rest
    assert calls[0].shape[0] == n_lattice == 125 and [c.shape[0] for c in calls[1:]] == [1000] * 15 + [561]


GUARD = 96                     # elements of poison before and after every buffer
F_POISON, I_POISON = 0x7FC0BEEF, 0x5EADBEEF


def _guarded(gpu, count, dtype, poison):
    buf = torch.full((count + 2 * GUARD,), poison, dtype=dtype, device=gpu)
    return buf, buf.data_ptr() + GUARD * buf.element_size()


def _entry_points(gpu, dense, level, lo, hi, brick, cut=0, **kw):
    """The whole pipeline through ctypes on buffers between guards; `cut`: the capacity of nf_sparse_grid_emit below the count.
    Returns the buffers (with their guards) on the host and the three counts."""
    from nerf import _hip as H
    lib, stream = H.lib(), H.stream_ptr(gpu)
    nz, ny, nx = dense.shape
    n_lattice = int(np.prod([S.n_bricks(n, brick) + 1 for n in (nx, ny, nz)]))
    c_lo, c_hi = (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi)
    a = ctypes.addressof
    ws_bytes = lib.nf_sparse_grid_workspace_bytes(nx, ny, nz, brick)
    ws, ws_p = _guarded(gpu, ws_bytes, torch.uint8, 0xA5)
    assert ws_p % 8 == 0
    grid, grid_p = _guarded(gpu, nx * ny * nz, torch.int32, F_POISON)
    counts, counts_p = _guarded(gpu, 3, torch.int64, -7)
    l_index, l_index_p = _guarded(gpu, n_lattice, torch.int32, I_POISON)
    l_coords, l_coords_p = _guarded(gpu, 3 * n_lattice, torch.int32, F_POISON)
    H.check(lib.nf_sparse_grid_lattice(nx, ny, nz, brick, a(c_lo), a(c_hi), l_index_p, l_coords_p, n_lattice, stream), "lattice")
    flat = dense.reshape(-1)
    values = flat[l_index[GUARD:GUARD + n_lattice].long()].contiguous()
    H.check(lib.nf_sparse_grid_scatter(values.data_ptr(), l_index_p, n_lattice, grid_p, nx, ny, nz, stream), "scatter")
    H.check(lib.nf_sparse_grid_classify(grid_p, nx, ny, nz, brick, level, kw.get("margin", 0.0), kw.get("dilate", 1), ws_p, ws_bytes, stream), "classify")
    H.check(lib.nf_sparse_grid_mark(nx, ny, nz, brick, ws_p, ws_bytes, counts_p, stream), "mark")
    n_seed, n_active, n_more = counts[GUARD:GUARD + 3].tolist()
    index, index_p = _guarded(gpu, n_more, torch.int32, I_POISON)
    coords, coords_p = _guarded(gpu, 3 * n_more, torch.int32, F_POISON)
    H.check(lib.nf_sparse_grid_emit(grid_p, nx, ny, nz, brick, a(c_lo), a(c_hi), ws_p, ws_bytes, index_p, coords_p, n_more - cut, stream), "emit")
    listed = index[GUARD:GUARD + n_more - cut]
    assert int(listed.min()) >= 0 and int(listed.max()) < nx * ny * nz
    values = flat[listed.long()].contiguous()
    H.check(lib.nf_sparse_grid_scatter(values.data_ptr(), index_p, n_more - cut, grid_p, nx, ny, nz, stream), "scatter")
    torch.cuda.synchronize()
    for buf, poison in ((ws, 0xA5), (grid, F_POISON), (counts, -7), (l_index, I_POISON), (l_coords, F_POISON), (index, I_POISON), (coords, F_POISON)):
        assert bool((buf[:GUARD] == poison).all()) and bool((buf[-GUARD:] == poison).all())
    return dict(grid=grid.cpu(), l_index=l_index.cpu(), l_coords=l_coords.cpu(), index=index.cpu(), coords=coords.cpu()), (n_seed, n_active, n_more)


def test_entry_points_keep_inside_their_buffers_and_repeat_bit_for_bit(hip_lib, gpu):
    """96 elements of poison on both sides of the workspace, the grid, the counts and the four index / coordinate buffers are intact
    after the whole pipeline; the grid is the restatement's; a second run gives the same bits; with a capacity 5 rows below the
    count the rows at and past it stay poison and the rows before it are the full run's; an index outside the grid writes nothing."""
    from nerf import _hip as H
    n, brick, lo, hi = (19, 13, 10), 4, R.BOX_LO, R.BOX_HI
    dense = _dense(gpu, _ball((-0.5, -0.4, -0.45), 0.5), lo, hi, n).contiguous()
    want = S.restate(dense.cpu().numpy(), 0.0, brick)
    bufs, counts = _entry_points(gpu, dense, 0.0, lo, hi, brick)
    n_more = counts[2]
    assert counts == (int(want.seed.sum()), int(want.active.sum()), int(want.evaluated.sum() - want.lattice.sum())) and n_more > 1000
    points = n[0] * n[1] * n[2]
    assert torch.equal(bufs["grid"][GUARD:GUARD + points].view(torch.float32).view(n[2], n[1], n[0]), torch.from_numpy(want.grid))
    assert np.array_equal(bufs["index"][GUARD:GUARD + n_more].numpy(), np.flatnonzero((want.evaluated & ~want.lattice).reshape(-1)))
    assert np.array_equal(bufs["l_index"][GUARD:-GUARD].numpy(), np.flatnonzero(want.lattice.reshape(-1)))
    table = _points(gpu, lo, hi, n).cpu()
    assert torch.equal(bufs["coords"][GUARD:-GUARD].view(torch.float32).view(-1, 3), table[bufs["index"][GUARD:-GUARD].long()])
    assert torch.equal(bufs["l_coords"][GUARD:-GUARD].view(torch.float32).view(-1, 3), table[bufs["l_index"][GUARD:-GUARD].long()])
    again, counts_again = _entry_points(gpu, dense, 0.0, lo, hi, brick)
    assert counts_again == counts and all(torch.equal(again[k], bufs[k]) for k in bufs)
    cut, counts_cut = _entry_points(gpu, dense, 0.0, lo, hi, brick, cut=5)
    assert counts_cut == counts
    for key, poison, width in (("index", I_POISON, 1), ("coords", F_POISON, 3)):
        keep = GUARD + width * (n_more - 5)
        assert torch.equal(cut[key][:keep], bufs[key][:keep]) and bool((cut[key][keep:] == poison).all())
    # scatter: indices outside the grid write nothing
    grid, grid_p = _guarded(gpu, points, torch.int32, F_POISON)
    index = torch.tensor([-1, points, points + 50, -(2 ** 31), 2 ** 31 - 1, 3], dtype=torch.int32, device=gpu)
    values = torch.arange(6, dtype=torch.float32, device=gpu)
    H.check(hip_lib.nf_sparse_grid_scatter(values.data_ptr(), index.data_ptr(), 6, grid_p, n[0], n[1], n[2], H.stream_ptr(gpu)), "scatter")
    torch.cuda.synchronize()
    written = (grid != F_POISON).nonzero().flatten().tolist()
    assert written == [GUARD + 3] and grid[GUARD + 3:GUARD + 4].view(torch.float32).item() == 5.0


# ---- model level
GRID_N, GRID_LO, GRID_HI, BRICK = (33, 33, 33), (-0.4, -0.35, -0.3), (0.35, 0.4, 0.4), 8
_MODELS = {}


def _model(kind, gpu):
    import nerf
    if kind not in _MODELS:
        m = U.make_model(nerf, C.build_case("eval_det_64_128")["p_coarse"], gpu) if kind == "paper" else U.make_lcode_model(nerf, O.init_lcode_params(6), gpu)
        _MODELS[kind] = m.eval()
    c = C.build_case("eval_det_64_128")
    return _MODELS[kind], c["expr"].to(gpu), c["latent"].to(gpu)


@pytest.mark.parametrize("kind,precision", [("paper", "f32"), ("lcode", "f16x3")])
def test_a_models_sparse_grid_is_its_dense_grid_where_it_is_evaluated(hip_lib, gpu, kind, precision):
    """nerf.density_grid_sparse == nerf.density_grid on the restatement's evaluated mask, bit for bit, and +-inf with the sign of the
    brick's corners elsewhere (the whole grid torch.equal to the restatement of the dense grid); extract_mesh(brick=8) is
    ops.isosurface of that grid; extract_mesh(brick=None) is ops.isosurface of the dense grid, as before."""
    import nerf
    from nerf import ops
    m, expr, latent = _model(kind, gpu)
    nerf.set_mlp_precision(precision)
    box = dict(lo=GRID_LO, hi=GRID_HI, resolution=GRID_N)
    dense = nerf.density_grid(m, expr, latent, **box)
    level = float(dense.flatten().kthvalue(int(0.98 * dense.numel())).values)          # a level few points exceed: some bricks stay inactive
    want = S.restate(dense.cpu().numpy(), level, BRICK)
    grid, stats = nerf.density_grid_sparse(m, expr, latent, level=level, brick=BRICK, **box)
    print(f"{kind} {precision}: level {level:.5g}, {stats}")
    assert not grid.requires_grad and grid.is_cuda and isinstance(stats, ops.SparseGridStats)
    assert stats == (64, int(want.seed.sum()), int(want.active.sum()), 33 ** 3, int(want.evaluated.sum())) and stats.seed_bricks > 0
    mask = torch.from_numpy(want.evaluated).to(gpu)
    assert torch.equal(grid[mask], dense[mask])
    side = torch.from_numpy(np.where(want.grid > 0, np.float32(np.inf), np.float32(-np.inf))).to(gpu)
    assert torch.equal(grid[~mask], side[~mask]) and torch.equal(grid.cpu(), torch.from_numpy(want.grid))
    chunked, stats_chunked = nerf.density_grid_sparse(m, expr, latent, level=level, brick=BRICK, chunk_points=1000, **box)
    assert torch.equal(chunked, grid) and stats_chunked == stats
    mesh = nerf.extract_mesh(m, expr, latent, level=level, brick=BRICK, **box)
    assert isinstance(mesh, nerf.Mesh) and all(torch.equal(x, y) for x, y in zip(mesh, ops.isosurface(grid, level, GRID_LO, GRID_HI, normals=True)))
    assert mesh.faces.shape[0] > 0
    today = nerf.extract_mesh(m, expr, latent, level=level, **box)
    assert all(torch.equal(x, y) for x, y in zip(today, ops.isosurface(dense, level, GRID_LO, GRID_HI, normals=True)))
    assert nerf.extract_mesh(m, expr, latent, level=level, brick=BRICK, normals=False, dilate=0, **box).normals is None
    with pytest.raises(ValueError):
        nerf.extract_mesh(m, expr, latent, level=level, brick=BRICK, dilate=0, **box)


def test_launcher_writes_a_ply_from_a_sparse_grid(hip_lib, gpu, tmp_path, capsys):
    """launch.extract_mesh --brick 8 on the synthetic dataset and an untrained checkpoint at 24^3: it prints the brick statistics, they
    are the restatement's for the dense grid of the same inputs, and the .ply holds ops.isosurface of the sparse grid."""
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
    dense = nerf.density_grid(model_f.eval(), expressions[1].float().to(gpu), latents[1].to(gpu), lo=lo, hi=hi, resolution=24)
    level = float(dense.median())
    want = S.restate(dense.cpu().numpy(), level, 8)
    out = os.path.join(base, "meshes", "frame1.ply")
    stats = extract_mesh.main(["--config", cfg_path, "--checkpoint", ck_path, "--frame", "1", "--level", repr(level), "--resolution", "24", "--out", out,
                               "--brick", "8"])
    text = capsys.readouterr().out
    sparse = stats["sparse"]
    assert sparse == dict(bricks=27, seed_bricks=int(want.seed.sum()), active_bricks=int(want.active.sum()), points=24 ** 3,
                          evaluated_points=int(want.evaluated.sum()))
    assert f"{sparse['seed_bricks']} seed and {sparse['active_bricks']} active of 27 bricks" in text
    assert f"density evaluated on {sparse['evaluated_points']} of {24 ** 3} points" in text and f"V = {stats['vertices']}, F = {stats['faces']}" in text
    vert, faces, props, _, _ = R.read_ply(out)
    assert props == ["x", "y", "z", "nx", "ny", "nz"] and stats["faces"] > 0 and np.isfinite(vert).all()
    mesh = nerf.ops.isosurface(torch.from_numpy(want.grid).to(gpu), level, lo, hi, normals=True)
    assert np.array_equal(faces, mesh[1].cpu().numpy()) and np.array_equal(vert[:, :3], mesh[0].cpu().numpy())
    assert np.array_equal(vert[:, 3:], mesh[2].cpu().numpy())
    with pytest.raises(SystemExit):
        extract_mesh.main(["--config", cfg_path, "--checkpoint", ck_path, "--frame", "1", "--level", "0", "--resolution", "24", "--out", out, "--brick", "1"])
