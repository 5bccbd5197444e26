"""Density-only forward on the GPU: the sigma kernels against the full inference kernels (bit for bit), the colour-free integrator
against the full one (bit for bit), nerf.density, the coarse_density_only render option and the launcher flag.  GPU only.
Nothing here has a tolerance except nerf.density against model.forward, which is held to the bound tests/test_gpu_lcode.py
already uses for that forward against the oracle."""
import os
import re
import sys

import pytest
import torch
import yaml

from oracle import cases as C
from oracle import nerface_oracle as O
from tests import blendshape_ref as B
from tests import smaller_ref as S
from tests import util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("f32", "bf16x3", "f16x3", "f16x2")
KINDS = {"paper": ALL, "lcode": ALL, "bshape": ALL, "cbshape": ALL, "smaller": ("f32",)}
COMBOS = [(k, p) for k, ps in KINDS.items() for p in ps]


def _shares():
    """Points per wave and per workgroup of the exact-f32 kernels, from their own #defines (the split kernels: 32 and 128)."""
    text = open(os.path.join(ROOT, "4d-facial-avatars_amd", "csrc", "nf_mlp_dev.h")).read()
    nt, waves = (int(re.search(r"#define %s (\d+)" % n, text).group(1)) for n in ("NF_MLP_NT", "NF_MLP_WAVES"))
    return 16 * nt, 16 * nt * waves


_MODELS = {}


def _model(kind, gpu):
    """The five classes: paper and lcode as the existing GPU tests build them, the others with their own test files' initialisers."""
    import nerf
    if kind not in _MODELS:
        if kind == "paper":
            m = U.make_model(nerf, C.build_case("eval_det_64_128")["p_coarse"], gpu)
        elif kind == "lcode":
            m = U.make_lcode_model(nerf, O.init_lcode_params(6), gpu)
        elif kind == "smaller":
            m = nerf.models.ConditionalBlendshapePaperSmallerNeRFModel(**S.SMALLER_KW)
            m.load_state_dict(S.init_smaller_params(14))
            m = m.to(gpu)
        else:
            m = getattr(nerf.models, B.CLASS[kind])(**B.MODEL_KW)
            m.load_state_dict(B.init_params(kind, 14, boost="survey"))
            m = m.to(gpu)
        assert m.fused_supported()
        _MODELS[kind] = m.eval()
    c = C.build_case("eval_det_64_128")
    return _MODELS[kind], c["expr"].to(gpu), c["latent"].to(gpu)


def _points(n_rays, s, seed):
    g = torch.Generator().manual_seed(seed)
    ro, rd, _, _, _ = C.ray_subset(512, 512, 3, n_rays, seed + 7)
    z = torch.sort(torch.rand((n_rays, s), generator=g) * 0.6 + 0.2, dim=-1)[0]
    return ro, rd, z


NAN_PAYLOAD = 0x7FC0BEEF
GUARD = 64


@pytest.mark.parametrize("kind,precision", COMBOS)
def test_sigma_is_the_full_forward_bit_for_bit(hip_lib, gpu, kind, precision):
    """hip_sigma == hip_forward(..., need_grad=False)[0][..., 3] with torch.equal, at 1 and 15 points, one below / at / one above a wave's
    and a workgroup's share, and over three and four workgroups; the entry point writes nothing outside sigma[n_points]."""
    import nerf
    from nerf import _hip as H
    from nerf import ops
    per_wave, per_wg = _shares()
    assert (per_wave, per_wg) == (32, 128)                                    # the split kernels' shares: one list serves both
    shapes = [(1, 1), (3, 5), (1, per_wave - 1), (1, per_wave), (1, per_wave + 1), (1, per_wg - 1), (4, per_wg // 4), (3, 43),
              (3, 100), (7, 64)]
    assert [r * s for r, s in shapes] == [1, 15, 31, 32, 33, 127, 128, 129, 300, 448]
    m, expr, latent = _model(kind, gpu)
    nerf.set_mlp_precision(precision)
    fam, hw = m.FAMILY, m.hip_weights()
    for i, (n_rays, s) in enumerate(shapes):
        ro, rd, z = (t.to(gpu) for t in _points(n_rays, s, 11 + i))
        full, _ = m.hip_forward(ro, rd, z, None, expr, latent, O.NEAR, O.FAR, False)
        sig = m.hip_sigma(ro, rd, z, expr, latent, O.NEAR, O.FAR)
        assert sig.shape == (n_rays, s) and sig.dtype == torch.float32
        assert torch.equal(sig, full[..., 3]), (kind, precision, n_rays, s, float((sig - full[..., 3]).abs().max()))
        # the C entry point on a buffer with poisoned guards
        n = n_rays * s
        buf = torch.full((n + 2 * GUARD,), NAN_PAYLOAD, dtype=torch.int32, device=gpu)
        image = {"f32": hw.get, "bf16x3": hw.get_bf16, "f16x3": hw.get_f16, "f16x2": hw.get_f16}[precision]()
        cond = ops.mlp_condition(fam, hw.get(), expr, latent, O.NEAR, O.FAR)
        fam.call(ops._SIGMA_ENTRY[precision], H.ptr(image), H.ptr(cond), H.ptr(ro), H.ptr(rd), 0, H.ptr(z), n_rays, s,
                 buf.data_ptr() + 4 * GUARD, H.stream_ptr(gpu))
        assert torch.equal(buf[GUARD:GUARD + n].view(torch.float32), full[..., 3].reshape(-1)), (kind, precision, n_rays, s)
        assert bool((buf[:GUARD] == NAN_PAYLOAD).all()) and bool((buf[GUARD + n:] == NAN_PAYLOAD).all()), (kind, precision, n_rays, s)
    if precision in ops.F16_MODES:
        ops.check_f16_range(m)                                                 # the range flag keeps its meaning: nothing overflowed


@pytest.mark.parametrize("S_", [1, 2, 63, 64, 65, 129])
def test_volume_weights_is_the_integrator_without_colours(hip_lib, gpu, S_):
    """weights, disparity and acc of volume_render_fwd from raw[..., 3] alone, bit for bit, with and without noise and background;
    ray 0 has no positive density, ray 1 a zero direction."""
    from nerf import ops
    g = torch.Generator().manual_seed(100 + S_)
    R = 9
    raw = (torch.randn((R, S_, 4), generator=g) * 3.0)
    raw[0, :, 3] = -raw[0, :, 3].abs() - 0.1
    z = torch.sort(torch.rand((R, S_), generator=g) * 0.6 + 0.2, dim=-1)[0]
    rd = torch.randn((R, 3), generator=g)
    rd[1] = 0.0
    noise = torch.randn((R, S_), generator=g)
    bg = torch.rand((R, 3), generator=g)
    raw, z, rd, noise, bg = (t.to(gpu).contiguous() for t in (raw, z, rd, noise, bg))
    sigma = raw[..., 3].contiguous()
    for nz in (None, noise):
        disp, acc, w = ops.volume_weights_fwd(sigma, z, rd, nz)
        for b in (None, bg):
            _, disp_f, acc_f, w_f = ops.volume_render_fwd(raw, z, rd, nz, b)
            for name, a, ref in (("weights", w, w_f), ("disp", disp, disp_f), ("acc", acc, acc_f)):
                assert torch.equal(a.view(torch.int32), ref.view(torch.int32)), (S_, nz is not None, b is not None, name)


@pytest.mark.parametrize("kind,precision", COMBOS)
def test_density_at_points(hip_lib, gpu, kind, precision):
    """nerf.density = hip_sigma on the same points bit for bit; in f32 also model.forward's density column for any direction, within
    2e-5 * scale + 2e-5 (the bound of that forward against the oracle); no points -> shape (0,)."""
    import nerf
    m, expr, latent = _model(kind, gpu)
    g = torch.Generator().manual_seed(5)
    pts = ((torch.rand((131, 3), generator=g) - 0.5) * 0.8).to(gpu)
    lat = None if not m.NEEDS_LATENT else latent
    nerf.set_mlp_precision(precision)
    with torch.no_grad():
        d = nerf.density(m, pts, expr, lat)
        assert nerf.density(m, pts[:0], expr, lat).shape == (0,)
    assert d.shape == (131,)
    zero = torch.zeros_like(pts)
    ref = m.hip_sigma(pts, zero, torch.zeros((131, 1), device=gpu), expr, latent, 0.0, 0.0)
    assert torch.equal(d, ref.reshape(-1))
    with pytest.raises(NotImplementedError, match="no autograd"):            # the parameters require grad
        nerf.density(m, pts, expr, lat)
    if precision == "f32":
        dirs = torch.randn((131, 3), generator=g)
        x87 = O.encode_points(pts.cpu(), dirs, torch.zeros((131, 1)), O.NEAR, O.FAR).to(gpu)
        with torch.no_grad():
            fwd = m(x87, expr, latent)[..., 3]
        scale = float(fwd.abs().max())
        err = float((d - fwd).abs().max())
        print(f"{kind} density vs forward(x87): err {err:.3e} scale {scale:.3e}")
        assert err <= 2e-5 * scale + 2e-5


@pytest.mark.parametrize("perturbed", [True, False])
@pytest.mark.parametrize("kind,precision", COMBOS)
def test_coarse_density_only_end_to_end(hip_lib, gpu, kind, precision, perturbed):
    """run_one_iter_of_nerf(mode="validation") on an 8 x 8 image, 5 + 7 samples, chunks of 48 rays (a ragged last chunk): with the flag
    the coarse colour is None and every other output is torch.equal to the default path's from the same seed."""
    import nerf
    mc, expr, latent = _model(kind, gpu)
    mf = mc                                                                     # any fine network of the class will do
    ro, rd, _, _, _ = C.ray_subset(512, 512, 3, 64, 21)
    ro, rd = ro.reshape(8, 8, 3).to(gpu), rd.reshape(8, 8, 3).to(gpu)
    bg = torch.rand((64, 3), generator=torch.Generator().manual_seed(3)).to(gpu)
    ex, ed = U.encoders(nerf)
    nerf.set_mlp_precision(precision)
    outs = []
    for flag in (False, True):
        opt = U.make_options(nerf, 5, 7, perturbed, 1.0 if perturbed else 0.0, chunksize=48)
        if flag:
            opt.nerf.validation.coarse_density_only = True
        torch.manual_seed(1234)
        with torch.no_grad():
            outs.append(nerf.run_one_iter_of_nerf(8, 8, None, mc, mf, ro, rd, opt, mode="validation", encode_position_fn=ex,
                                                  encode_direction_fn=ed, expressions=expr, background_prior=bg, latent_code=latent))
    full, lean = outs
    assert len(full) == len(lean) == 7
    assert torch.is_tensor(full[0]) and full[0].shape == (8, 8, 3) and lean[0] is None
    for k in range(1, 7):
        assert lean[k].shape == full[k].shape and torch.equal(lean[k], full[k]), (kind, precision, perturbed, k)


def test_eval_sharded_flag_writes_the_same_bytes(hip_lib, gpu, tmp_path):
    """launch/eval_sharded.py --coarse-density-only on the launcher tests' synthetic sequence: the PNGs (the fine image) are the same
    files byte for byte."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))
    import make_synthetic_dataset as MS
    from launch import common as CM
    from launch import eval_sharded
    base = str(tmp_path)
    MS.write(os.path.join(base, "data"))
    cfg_path = os.path.join(base, "config.yml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(MS.config(os.path.join(base, "data"), os.path.join(base, "logs")), f)
    torch.manual_seed(7)
    model_c, model_f = CM.build_models(CM.load_config(cfg_path), gpu)
    ck_path = os.path.join(base, "ck.ckpt")
    torch.save({"model_coarse_state_dict": model_c.state_dict(), "model_fine_state_dict": model_f.state_dict()}, ck_path)
    files = {}
    for name, extra in (("a", []), ("b", ["--coarse-density-only"])):
        out = os.path.join(base, name)
        torch.manual_seed(99)                                                  # validation perturbs: the same draws for both runs
        assert eval_sharded.main(["--config", cfg_path, "--checkpoint", ck_path, "--savedir", out, *extra]) == [0, 1, 2]
        files[name] = {p: open(os.path.join(out, p), "rb").read() for p in sorted(os.listdir(out)) if p.endswith(".png")}
    assert sorted(files["a"]) == ["0000.png", "0001.png", "0002.png"] and files["a"] == files["b"]
