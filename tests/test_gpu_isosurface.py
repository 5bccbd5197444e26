"""Isosurface extraction on the GPU: ops.isosurface against tests/isosurface_ref.py (faces equal, positions to the last bit or so,
normals to 1e-5) at every size at which csrc/nf_isosurface.hip takes another path, the C entry points on poisoned buffers, and the
model-level functions (nerf.density_grid, nerf.extract_mesh, launch.extract_mesh).  GPU only."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest
import torch
import yaml

from oracle import cases as C
from oracle import nerface_oracle as O
from tests import isosurface_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 256                    # nfc::THREADS: points per workgroup, one block sum each
SCAN_ROUND = 16 * 1024         # k_iso_scan: block sums per round of its one workgroup (SCAN_PER_THREAD * SCAN_THREADS)

# (nx, ny, nz).  (41, 5, 5) = 1025 points: one more than four workgroups' 4 * 256, so the last point sits alone in a fifth workgroup,
# cells read vertex bases across every workgroup boundary, and (65, 3, 2) and (257, 2, 2) end inside their second / fifth workgroup.
SMALL_GRIDS = [(2, 2, 2), (3, 2, 2), (65, 3, 2), (257, 2, 2), (23, 19, 21), (41, 5, 5)]


def test_the_constants_above_are_the_kernels_own():
    shared, unit = (open(os.path.join(ROOT, "4d-facial-avatars_amd", "csrc", f)).read() for f in ("nf_scan_dev.h", "nf_isosurface.hip"))
    assert "constexpr int THREADS = 256;" in shared and "constexpr int SCAN_THREADS = 1024;" in shared and "constexpr int SCAN_PER_THREAD = 16;" in unit
    assert 41 * 5 * 5 == 4 * BLOCK + 1


def _field(n, seed):
    """Seeded smooth-plus-noise field on the grid n = (nx, ny, nz) with both signs in every part of the grid."""
    rng = np.random.default_rng(seed)
    x, y, z = R.grid_points((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), n)
    return (np.sin(3.0 * x + 1.0) * np.cos(2.0 * y) + 0.5 * z + 0.4 * rng.standard_normal(x.shape)).astype(np.float32)


def _run(gpu, v, level, lo, hi, normals=True):
    from nerf import ops
    return ops.isosurface(torch.from_numpy(np.ascontiguousarray(v)).to(gpu), level, lo, hi, normals=normals)


def _compare(gpu, v, level, lo, hi, what, normals_gate=None):
    """Faces equal, positions within 2^-22 * max(|lo|, |hi|) per component (one ulp in the division, one rounding each in the product
    and the sum; expected: 0), the measured maximum printed.  Returns (device mesh, restatement mesh)."""
    got = _run(gpu, v, level, lo, hi)
    want = R.isosurface(v, level, lo, hi, normals=True)
    gv, gf, gn = (t.cpu() for t in got)
    assert gv.dtype == torch.float32 and gf.dtype == torch.int32 and gn.dtype == torch.float32
    assert gv.shape == want[0].shape and gf.shape == want[1].shape and gn.shape == want[0].shape, (what, gv.shape, gf.shape, want[0].shape, want[1].shape)
    assert torch.equal(gf, torch.from_numpy(want[1])), what
    gate = 2.0 ** -22 * float(max(np.abs(np.float32(lo)).max(), np.abs(np.float32(hi)).max()))
    err = float((gv.double() - torch.from_numpy(want[0]).double()).abs().max()) if gv.numel() else 0.0
    print(f"{what}: V {gv.shape[0]} F {gf.shape[0]} max position difference {err:.3e} (gate {gate:.3e})")
    assert err <= gate, (what, err)
    if normals_gate is not None:
        nerr = float((gn.double() - torch.from_numpy(want[2]).double()).abs().max())
        print(f"{what}: max normal difference {nerr:.3e} (gate {normals_gate:.0e})")
        assert nerr <= normals_gate, (what, nerr)
    return (gv, gf, gn), want


@pytest.mark.parametrize("n", SMALL_GRIDS, ids=lambda n: "x".join(map(str, n)))
def test_small_grids_against_the_restatement(hip_lib, gpu, n):
    (gv, gf, gn), _ = _compare(gpu, _field(n, 3), 0.1, (-1.1, -0.9, -1.0), (1.2, 1.0, 1.1), f"grid {n}")
    assert gf.shape[0] > 0 and torch.isfinite(gv).all() and torch.isfinite(gn).all()


def test_block_sums_carry_across_scan_rounds(hip_lib, gpu):
    """More block sums than one round of k_iso_scan takes (16384): two small blobs, one among the first workgroups' points and one in the
    last planes (block sums past the first round), so the second blob's bases are a carry plus a prefix."""
    n = (1024, 64, 72)
    assert n[0] * n[1] * n[2] // BLOCK > SCAN_ROUND
    lo, hi = (0.0, 0.0, 0.0), (1023.0, 63.0, 71.0)
    x, y, z = R.grid_points(lo, hi, n)
    blob = lambda cx, cy, cz: np.float32(6.3) - ((x - np.float32(cx)) ** 2 + (y - np.float32(cy)) ** 2 + (z - np.float32(cz)) ** 2)
    v = np.maximum(blob(4.2, 3.6, 3.1), blob(1019.4, 59.3, 67.1)).astype(np.float32)
    (gv, gf, _), _ = _compare(gpu, v, 0.0, lo, hi, "two blobs on 1024 x 64 x 72")
    rep = R.mesh_report(gv.numpy(), gf.numpy())
    assert rep["closed"] and rep["chi"] == 4 and rep["volume"] > 0
    first_of_second_blob = int((gv[:, 2] > 30).nonzero()[0])
    assert 0 < first_of_second_blob < gv.shape[0]


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_normals_on_analytic_fields(hip_lib, gpu, name):
    """Normals within 1e-5 per component of the restatement (the normalisation is a few ulp); on the sphere the angle to the radial
    direction is at most 1.5 x the restatement's own worst angle."""
    v = getattr(R, name)(*R.grid_points(R.BOX_LO, R.BOX_HI, R.BOX_N))
    (gv, gf, gn), want = _compare(gpu, v, 0.0, R.BOX_LO, R.BOX_HI, name, normals_gate=1e-5)
    rep = R.mesh_report(gv.numpy(), gf.numpy())
    assert rep["closed"] and rep["chi"] == (2 if name == "sphere" else 0) and rep["volume"] > 0
    if name == "sphere":
        def worst_angle(verts, normals):
            radial = verts.astype(np.float64) / np.linalg.norm(verts.astype(np.float64), axis=1, keepdims=True)
            return float(np.degrees(np.arccos(np.clip(np.sum(radial * normals.astype(np.float64), axis=1), -1.0, 1.0)).max()))
        ref_angle, got_angle = worst_angle(want[0], want[2]), worst_angle(gv.numpy(), gn.numpy())
        print(f"sphere: worst angle to the radial direction {got_angle:.4f} deg (restatement {ref_angle:.4f} deg)")
        assert got_angle <= 1.5 * ref_angle and ref_angle < 10.0


def test_all_inside_all_outside_and_values_at_the_level(hip_lib, gpu):
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    for fill in (1.0, -1.0, 0.0, float("nan")):                                  # inside, outside, == level (outside), NaN (outside)
        v, f, n = _run(gpu, np.full((4, 5, 6), fill, dtype=np.float32), 0.0, lo, hi)
        assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3) and f.dtype == torch.int32 and v.is_cuda
    assert _run(gpu, np.zeros((3, 3, 3), dtype=np.float32), 0.0, lo, hi, normals=False)[2] is None
    # a field of small integers: many values exactly at the level, which count as outside
    v = np.round(3.0 * _field((13, 11, 9), 5)).astype(np.float32)
    assert (v == 1.0).sum() > 50
    (gv, gf, _), _ = _compare(gpu, v, 1.0, lo, hi, "integer field at level 1")
    assert gf.shape[0] > 0


def test_nan_and_infinities_take_the_midpoint(hip_lib, gpu):
    """NaN, +inf and -inf entries: NaN and -inf are outside, +inf inside; an edge with such an end gets t = 0.5; every output is finite."""
    rng = np.random.default_rng(11)
    v = _field((12, 10, 9), 7)
    flat = v.reshape(-1)
    picks = rng.choice(flat.size, size=90, replace=False)
    flat[picks[:30]], flat[picks[30:60]], flat[picks[60:]] = np.nan, np.inf, -np.inf
    (gv, gf, gn), want = _compare(gpu, v, 0.1, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), "field with NaN and infinities")
    assert torch.isfinite(gv).all() and torch.isfinite(gn).all() and gf.shape[0] > 0
    assert torch.equal(gn == 0, torch.from_numpy(want[2]) == 0)                  # the zero normals sit at the same vertices


def test_crossing_only_in_the_last_cell_and_a_surface_cut_by_the_box(hip_lib, gpu):
    v = np.full((3, 4, 5), -1.0, dtype=np.float32)
    v[-1, -1, -1] = 2.0                                                           # the last grid point: seven edges end there
    (gv, gf, _), _ = _compare(gpu, v, 0.0, (0.0, 0.0, 0.0), (4.0, 3.0, 2.0), "last point inside")
    assert gv.shape[0] == 7 and gf.shape[0] == 6 and not R.mesh_report(gv.numpy(), gf.numpy())["closed"]
    big = R.sphere(*R.grid_points(R.BOX_LO, R.BOX_HI, R.BOX_N), r=1.3)            # leaves the box on every side: an open mesh
    (gv, gf, _), _ = _compare(gpu, big, 0.0, R.BOX_LO, R.BOX_HI, "sphere r = 1.3 cut by the box")
    assert gf.shape[0] > 0 and not R.mesh_report(gv.numpy(), gf.numpy())["closed"]


GUARD = 96
F_POISON, I_POISON = 0x7FC0BEEF, 0x5EADBEEF


def _entry_points(gpu, v, level, lo, hi, cut_v=0, cut_f=0, normals=True):
    """nf_isosurface_count / _emit on output buffers with GUARD poisoned words on either side and capacities cut_v / cut_f rows below
    the counts.  Returns (V, F, verts, faces, normals) buffers with their guards, on the host."""
    from nerf import _hip as H
    lib = H.lib()
    nz, ny, nx = v.shape
    grid = torch.from_numpy(v).to(gpu)
    ws_bytes = lib.nf_isosurface_workspace_bytes(nx, ny, nz)
    ws = torch.full((ws_bytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=gpu)
    counts = torch.full((2 + 2,), -7, dtype=torch.int64, device=gpu)
    assert (ws.data_ptr() + GUARD) % 32 == 0
    stream = H.stream_ptr(gpu)
    H.check(lib.nf_isosurface_count(H.ptr(grid), nx, ny, nz, level, ws.data_ptr() + GUARD, ws_bytes, counts.data_ptr() + 8, stream), "count")
    assert counts[0].item() == -7 and counts[3].item() == -7
    n_v, n_f = counts[1:3].tolist()
    fbuf = lambda rows: torch.full((rows * 3 + 2 * GUARD,), F_POISON, dtype=torch.int32, device=gpu)
    verts, norm, faces = fbuf(n_v), fbuf(n_v), torch.full((n_f * 3 + 2 * GUARD,), I_POISON, dtype=torch.int32, device=gpu)
    c_lo, c_hi = (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi)
    H.check(lib.nf_isosurface_emit(H.ptr(grid), nx, ny, nz, level, ctypes.addressof(c_lo), ctypes.addressof(c_hi), ws.data_ptr() + GUARD, ws_bytes,
                                   verts.data_ptr() + 4 * GUARD, n_v - cut_v, faces.data_ptr() + 4 * GUARD, n_f - cut_f,
                                   norm.data_ptr() + 4 * GUARD if normals else None, stream), "emit")
    torch.cuda.synchronize()
    assert bool((ws[:GUARD] == 0xA5).all()) and bool((ws[-GUARD:] == 0xA5).all())
    return n_v, n_f, verts.cpu(), faces.cpu(), norm.cpu()


def test_entry_points_keep_inside_their_buffers_and_repeat_bit_for_bit(hip_lib, gpu):
    """Guards of 96 words on both sides of verts, faces, normals and of the workspace stay as they were; V and F equal the
    restatement's counts; with capacities below the counts the rows at and past the capacity stay untouched and the rows before it
    are the full run's; a second run gives the same bits."""
    v, lo, hi = _field((41, 5, 5), 9), (-1.0, -0.5, 0.0), (1.0, 0.5, 2.0)
    want = R.isosurface(v, 0.1, lo, hi, normals=True)
    n_v, n_f, verts, faces, norm = _entry_points(gpu, v, 0.1, lo, hi)
    assert (n_v, n_f) == (want[0].shape[0], want[1].shape[0]) and n_v > 40 and n_f > 40
    for buf, poison, rows in ((verts, F_POISON, n_v), (norm, F_POISON, n_v), (faces, I_POISON, n_f)):
        assert bool((buf[:GUARD] == poison).all()) and bool((buf[GUARD + 3 * rows:] == poison).all())
        assert buf.numel() == 3 * rows + 2 * GUARD
    assert torch.equal(faces[GUARD:GUARD + 3 * n_f].view(-1, 3), torch.from_numpy(want[1]))
    assert np.array_equal(verts[GUARD:GUARD + 3 * n_v].numpy().view(np.float32).reshape(-1, 3), want[0])
    again = _entry_points(gpu, v, 0.1, lo, hi)
    assert again[:2] == (n_v, n_f) and all(torch.equal(a, b) for a, b in zip(again[2:], (verts, faces, norm)))
    cut = _entry_points(gpu, v, 0.1, lo, hi, cut_v=5, cut_f=7)
    for full, part, poison, rows in ((verts, cut[2], F_POISON, n_v - 5), (norm, cut[4], F_POISON, n_v - 5), (faces, cut[3], I_POISON, n_f - 7)):
        assert torch.equal(part[:GUARD + 3 * rows], full[:GUARD + 3 * rows]) and bool((part[GUARD + 3 * rows:] == poison).all())
    none = _entry_points(gpu, v, 0.1, lo, hi, normals=False)
    assert torch.equal(none[2], verts) and torch.equal(none[3], faces) and bool((none[4] == F_POISON).all())
    # the Python layer twice
    a, b = _run(gpu, v, 0.1, lo, hi), _run(gpu, v, 0.1, lo, hi)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- model level
GRID_N, GRID_LO, GRID_HI = (17, 13, 11), (-0.4, -0.35, -0.3), (0.35, 0.4, 0.4)
_MODELS = {}


def _model(kind, gpu):
    import nerf
    if kind not in _MODELS:
        m = U.make_model(nerf, C.build_case("eval_det_64_128")["p_coarse"], gpu) if kind == "paper" else U.make_lcode_model(nerf, O.init_lcode_params(6), gpu)
        _MODELS[kind] = m.eval()
    c = C.build_case("eval_det_64_128")
    return _MODELS[kind], c["expr"].to(gpu), c["latent"].to(gpu)


@pytest.mark.parametrize("kind,precision", [("paper", "f32"), ("paper", "f16x3"), ("lcode", "f32")])
def test_density_grid_is_density_on_the_same_points(hip_lib, gpu, kind, precision):
    """nerf.density_grid in three slabs (4 + 4 + 3 planes of 17 x 13) == nerf.density on all the points at once, torch.equal."""
    import nerf
    m, expr, latent = _model(kind, gpu)
    nerf.set_mlp_precision(precision)
    nx, ny, nz = GRID_N
    grid = nerf.density_grid(m, expr, latent, lo=GRID_LO, hi=GRID_HI, resolution=GRID_N, chunk_points=4 * nx * ny + 5)
    assert grid.shape == (nz, ny, nx) and grid.dtype == torch.float32 and grid.is_cuda and not grid.requires_grad
    x, y, z = R.grid_points(GRID_LO, GRID_HI, GRID_N)
    pts = torch.from_numpy(np.stack([x, y, z], axis=-1).reshape(-1, 3)).to(gpu)
    with torch.no_grad():
        want = nerf.density(m, pts, expr, latent)
    assert torch.equal(grid.reshape(-1), want)
    one = nerf.density_grid(m, expr, latent, lo=GRID_LO, hi=GRID_HI, resolution=GRID_N)
    assert torch.equal(one, grid)
    assert float(grid.std()) > 0


def test_extract_mesh_is_the_restatement_on_the_models_grid(hip_lib, gpu):
    import nerf
    m, expr, latent = _model("paper", gpu)
    grid = nerf.density_grid(m, expr, latent, lo=GRID_LO, hi=GRID_HI, resolution=GRID_N)
    level = float(grid.median())
    mesh = nerf.extract_mesh(m, expr, latent, lo=GRID_LO, hi=GRID_HI, resolution=GRID_N, level=level)
    assert isinstance(mesh, nerf.Mesh) and mesh.vertices.is_cuda and mesh.faces.is_cuda and mesh.normals.is_cuda
    want = R.isosurface(grid.cpu().numpy(), level, GRID_LO, GRID_HI, normals=True)
    assert want[1].shape[0] > 0
    assert torch.equal(mesh.faces.cpu(), torch.from_numpy(want[1]))
    gate = 2.0 ** -22 * 0.4
    err = float((mesh.vertices.cpu().double() - torch.from_numpy(want[0]).double()).abs().max())
    print(f"extract_mesh: V {mesh.vertices.shape[0]} F {mesh.faces.shape[0]} max position difference {err:.3e} (gate {gate:.3e})")
    assert err <= gate
    assert nerf.extract_mesh(m, expr, latent, lo=GRID_LO, hi=GRID_HI, resolution=GRID_N, level=level, normals=False).normals is None


def test_launcher_writes_a_ply(hip_lib, gpu, tmp_path, capsys):
    """launch.extract_mesh on the synthetic dataset and an untrained checkpoint at 24^3: the frustum box, a .ply that parses, F > 0."""
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
    # the launcher's own inputs for frame 1, to pick a level that has a surface: the median of the fine network's grid
    _, poses, _, hwf, _, expressions, _, _ = nerf.load_flame_data(data, half_res=False, testskip=1, test=True)
    lo, hi = extract_mesh.frustum_box(int(hwf[0]), int(hwf[1]), hwf[2], poses[1, :3, :4].float().to(gpu), 0.2, 0.8)
    ro, rd = nerf.get_ray_bundle(int(hwf[0]), int(hwf[1]), hwf[2], poses[1, :3, :4].float().to(gpu))
    ends = torch.cat([ro[0, 0] + rd[0, 0] * 0.2, ro[-1, -1] + rd[-1, -1] * 0.8]).cpu()
    assert all(l <= float(e) + 1e-6 and float(e) - 1e-6 <= h for e, l, h in zip(ends, lo + lo, hi + hi))
    grid = nerf.density_grid(model_f.eval(), expressions[1].float().to(gpu), latents[1].to(gpu), lo=lo, hi=hi, resolution=24)
    level = float(grid.median())
    out = os.path.join(base, "meshes", "frame1.ply")
    stats = extract_mesh.main(["--config", cfg_path, "--checkpoint", ck_path, "--frame", "1", "--level", repr(level), "--resolution", "24", "--out", out])
    text = capsys.readouterr().out
    assert f"V = {stats['vertices']}, F = {stats['faces']}" in text and "density" in text and "extraction" in text and "box lo" in text
    assert stats["faces"] > 0 and stats["network"] == "fine" and stats["resolution"] == [24, 24, 24]
    assert np.allclose(stats["lo"], lo) and np.allclose(stats["hi"], hi)
    vert, faces, props, _, _ = R.read_ply(out)
    assert props == ["x", "y", "z", "nx", "ny", "nz"] and vert.shape[0] == stats["vertices"] and faces.shape[0] == stats["faces"]
    assert faces.min() >= 0 and faces.max() < vert.shape[0] and np.isfinite(vert).all()
    want = R.isosurface(grid.cpu().numpy(), level, lo, hi)
    assert np.array_equal(faces, want[1])
    coarse = extract_mesh.main(["--config", cfg_path, "--checkpoint", ck_path, "--frame", "1", "--level", repr(level), "--resolution", "12", "10", "8",
                                "--out", os.path.join(base, "c.off"), "--coarse", "--bounds", "-0.2", "-0.2", "-0.2", "0.2", "0.2", "0.2"])
    assert coarse["network"] == "coarse" and coarse["resolution"] == [12, 10, 8] and os.path.exists(os.path.join(base, "c.off"))
