"""The integrator's full backward (csrc/nf_render_bwd_full.hip) and everything that carries it up to the trainer: a cotangent of every
output, the gradient of the background prior, the two autograd Functions, get_ray_batch and the launcher's --train-background.  GPU only.

The yardstick is the oracle (oracle.nerface_oracle.volume_render / render_volume_density) under float64 autograd, on the input recipe
of tests/test_gpu_render_sizes.py (|raw_sigma + noise| >= 9e-3: no element is excluded for a ReLU flip; depths >= 0.2: the
max(1e-10, .) of the disparity is never a tie).  The prior is a leaf that enters the oracle as raw[:, -1, :3] (T:95-96); its gradient
is d_bg.

The gate, as in that file: per ray e = max |got - g64| / max |g64|, floor = max(e of the float32 oracle on the same inputs, 1e-7), and
the kernel stays within K x floor on every ray, for d_raw and for d_bg; whole tensors rel_l2 < 2e-5 (the float32 oracle itself stays
below 1e-6 on every case of this file, so no case needs a gate relative to it).

K = twice the worst kernel / floor ratio measured on an MI355X, rounded up.  d_bg has a K of its own by the same rule: it is ONE number
per ray and channel, w_last * d_rgb, so its ratio is the rounding of one product of up to 1024 transmittance factors in the kernel's scan
order against the same in the oracle's sequential order (the forward's weights carry the same error), not a maximum over S x 4 elements.
Measured worst ratio per ray, d_raw | d_bg, all cotangents at once:
  NeRFace mode  <1> 2.31 | 2.69   <2> 1.60 | 5.67   <3> 2.35 | 5.71   <4> 1.51 | 6.47   <8> 2.86 | 10.68   <16> 5.06 | 18.10
  tiny mode     <1> 3.47          <2> 1.67          <3> 1.63          <4> 1.27          <8> 1.68           <16> 1.82
one cotangent alone, S = 65 / 320:
  NeRFace  rgb 1.57 | 3.11 / 1.20 | 7.60   disparity 1.68 / 2.95   weights 2.15 / 2.24   last weight 2.47 / 5.42
  tiny     rgb 1.67 / 1.41   depth map 11.24 / 3.10   acc (thin rays) 2.77 / 7.85
volume_render_radiance_field, all outputs, S = 65: 1.57 | 3.11.  End to end (d_bg against the float32 oracle's whole render): 14.81
(soft_train_noflip_64_64), 2.67 (ragged_5_7).
  -> K_FULL = 2 x 11.24, rounded up = 23;  K_BG = 2 x 18.10, rounded up = 37
translucent regime (acc < 1: the one input on which d_acc and the A-dependence of the disparity have a gradient; its alphas are
1 - exp(-x) at x ~ 2e-3, so the ratio is the device's expf against the host's, see tests/test_gpu_render_sizes.py):
  all cotangents, S = 64: 2.65, 2.84 | 4.05   S = 320: 9.39, 5.44 | 11.38;   acc alone, S = 65 / 320: 6.13 / 10.28
  -> K_FULL_TRANSLUCENT = 2 x 11.38, rounded up = 23 (d_raw and d_bg)
rel_l2, worst: d_raw 9.8e-7 (float32 oracle 8.7e-7), d_bg 2.95e-6 (S = 1024; float32 oracle 2.95e-7); the rgb-only call of the full
kernel equals k_volume_render_bwd bit for bit (rel_l2 0) at every template.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import cases as C
from oracle import nerface_oracle as O
from tests import util as U
from tests.test_gpu_render_sizes import ABS_FLOOR, _inputs, _keep_relu_argument_off_zero

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

S_FULL = [1, 2, 63, 64, 65, 128, 129, 193, 257, 320, 513, 1024]
K_FULL = 23
K_BG = 37
K_FULL_TRANSLUCENT = 23
L2_GATE = 2e-5


def _cotangents(x, seed, only=None):
    """Random cotangents for every output of the case `x` (tiny mode has no weights output); `only`: that one alone."""
    g = torch.Generator().manual_seed(seed)
    n, s = x["z"].shape
    cot = dict(d_rgb=x["d_rgb"], d_third=torch.randn(n, generator=g), d_acc=torch.randn(n, generator=g),
               d_w=torch.randn((n, s), generator=g), d_wlast=torch.randn(n, generator=g))
    return {k: (v if only in (None, k) else None) for k, v in cot.items()}


def _oracle_grads(x, cot, dtype, mode, white):
    """(d_raw, d_bg | None) of L = sum over the outputs of <output, cotangent>, the oracle's own autograd in `dtype` on the CPU."""
    cv = lambda t: None if t is None else t.to(dtype)
    raw = cv(x["raw"]).clone().requires_grad_(True)
    bg = None if x["bg"] is None else cv(x["bg"]).clone().requires_grad_(True)
    if mode == "tiny":
        rgb, third, acc = O.render_volume_density(raw, cv(x["z"]))
        w = None
    else:
        raw_in = raw if bg is None else torch.cat((raw[:, :-1], torch.cat((bg[:, None, :], raw[:, -1:, 3:]), dim=-1)), dim=1)
        rgb, third, acc, w = O.volume_render(raw_in, cv(x["z"]), cv(x["rd"]), cv(x["noise"]), has_background=bg is not None,
                                             white_background=white)
    loss = 0.0
    for name, out in (("d_rgb", rgb), ("d_third", third), ("d_acc", acc), ("d_w", w), ("d_wlast", None if w is None else w[:, -1])):
        if cot[name] is not None and out is not None:
            loss = loss + (out * cv(cot[name])).sum()
    loss.backward()
    return raw.grad, (None if bg is None else bg.grad)


def _product_grads(x, cot, mode, white, gpu):
    from nerf import ops
    dv = lambda t: None if t is None else t.to(gpu).contiguous()
    if mode == "tiny":
        return ops.render_volume_density_bwd_full(dv(x["raw"]), dv(x["z"]), dv(cot["d_rgb"]), dv(cot["d_third"]), dv(cot["d_acc"])).cpu(), None
    d_raw, d_bg = ops.volume_render_bwd_full(dv(x["raw"]), dv(x["z"]), dv(x["rd"]), dv(x["noise"]), dv(x["bg"]), dv(cot["d_rgb"]),
                                             dv(cot["d_third"]), dv(cot["d_acc"]), dv(cot["d_w"]), dv(cot["d_wlast"]), white,
                                             need_d_bg=x["bg"] is not None)
    return d_raw.cpu(), (None if d_bg is None else d_bg.cpu())


def _ray_err(d, g):
    """max |d - g| / max |g| per ray (all trailing dimensions); a ray whose reference gradient is all zero is measured absolutely."""
    dims = tuple(range(1, g.dim()))
    scale = g.abs().amax(dim=dims)
    return (d.double() - g).abs().amax(dim=dims) / torch.where(scale > 0, scale, torch.ones_like(scale))


def _rel_l2(a, b):
    return float((a.double() - b).norm() / (b.norm() + 1e-30))


def _gate(tag, what, got, g64, g32, k_gate):
    """The gate of this file on one gradient tensor; prints every figure before it asserts.  Returns (floor per ray, worst ratio)."""
    assert bool(torch.isfinite(g64).all()) and bool(torch.isfinite(got).all()), (tag, what)
    floor = _ray_err(g32, g64)
    err = _ray_err(got, g64)
    ratio = err / floor.clamp(min=ABS_FLOOR)
    l2, f_l2 = _rel_l2(got, g64), _rel_l2(g32, g64)
    print(f"[render-grads] {tag} {what}: floor {float(floor.max()):.2e} kernel {float(err.max()):.2e} worst ratio {float(ratio.max()):.2f} "
          f"rel_l2 {l2:.2e} (float32 oracle {f_l2:.2e}, kernel / oracle {l2 / max(f_l2, 1e-30):.2f})")
    assert float(ratio.max()) <= k_gate, (tag, what, ratio.tolist())
    assert l2 < L2_GATE, (tag, what, l2)
    return floor, float(ratio.max())


def _check(x, cot, mode, white, gpu, tag, k_gate=K_FULL, k_bg=K_BG, alone=False):
    """`k_gate` holds d_raw and `k_bg` holds d_bg; a regime with a K of its own passes both."""
    g64, b64 = _oracle_grads(x, cot, torch.float64, mode, white)
    g32, b32 = _oracle_grads(x, cot, torch.float32, mode, white)
    got, got_bg = _product_grads(x, cot, mode, white, gpu)
    floor, _ = _gate(tag, "d_raw", got, g64, g32, k_gate)
    if alone:
        # the test has to be able to fail: with the term dropped every element is zero, i.e. e = 1 on every ray with a gradient
        assert float(g64.abs().max()) > 0 and k_gate * float(floor.clamp(min=ABS_FLOOR).min()) < 0.5, (tag, floor.tolist())
    if x["bg"] is not None:
        assert got_bg is not None and b64 is not None
        _gate(tag, "d_bg", got_bg, b64, b32, k_bg)
        assert float(got[:, -1, :3].abs().max()) == 0.0, tag                    # the last sample's colour is the prior, not raw
    else:
        assert got_bg is None
    pre = x["raw"][..., 3].double() + (0.0 if x["noise"] is None else x["noise"].double())
    assert float(got[..., 3][pre <= 0].abs().max() if bool((pre <= 0).any()) else 0.0) == 0.0, tag


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
SWITCHES = [(True, True, False), (False, False, True), (True, False, True)]        # (background prior, density noise, white background)


@pytest.mark.parametrize("with_bg,noisy,white", SWITCHES)
@pytest.mark.parametrize("s", S_FULL)
def test_full_backward_every_template_nerface(hip_lib, gpu, s, with_bg, noisy, white):
    x = _inputs(s, 1000 + s, "nerface", with_bg, noisy)
    _check(x, _cotangents(x, 7000 + s), "nerface", white, gpu, f"nerface S={s} bg={int(with_bg)} noise={int(noisy)} white={int(white)}")


@pytest.mark.parametrize("s", S_FULL)
def test_full_backward_every_template_tiny(hip_lib, gpu, s):
    x = _inputs(s, 2000 + s, "tiny")
    _check(x, _cotangents(x, 8000 + s), "tiny", False, gpu, f"tiny S={s}")


@pytest.mark.parametrize("only", ["d_rgb", "d_third", "d_w", "d_wlast"])
@pytest.mark.parametrize("s", [65, 320])
def test_each_cotangent_alone_nerface(hip_lib, gpu, s, only):
    x = _inputs(s, 1000 + s, "nerface", True, False)
    _check(x, _cotangents(x, 7000 + s, only), "nerface", False, gpu, f"alone {only} nerface S={s}", alone=True)


@pytest.mark.parametrize("s", [65, 320])
def test_acc_cotangent_alone_nerface(hip_lib, gpu, s):
    """d_acc alone.  With a camera's |rd| the far sample is opaque, acc == 1 and its gradient cancels to rounding: a dropped d_acc would
    not show.  The translucent regime is the input on which acc < 1, so that is where this term is tested on its own."""
    x = _inputs(s, 3000 + s, "nerface", False, False, "translucent")
    _check(x, _cotangents(x, 7000 + s, "d_acc"), "nerface", True, gpu, f"alone d_acc nerface translucent S={s}", k_gate=K_FULL_TRANSLUCENT,
           k_bg=K_FULL_TRANSLUCENT, alone=True)


@pytest.mark.parametrize("only", ["d_rgb", "d_third"])
@pytest.mark.parametrize("s", [65, 320])
def test_each_cotangent_alone_tiny(hip_lib, gpu, s, only):
    x = _inputs(s, 2000 + s, "tiny")
    _check(x, _cotangents(x, 8000 + s, only), "tiny", False, gpu, f"alone {only} tiny S={s}", alone=True)


@pytest.mark.parametrize("s", [65, 320])
def test_acc_cotangent_alone_tiny(hip_lib, gpu, s):
    """d_acc alone in tiny mode.  The recipe's rays are opaque (optical depth ~ 25 over depths [2, 6], and a far sample of dist 1e10), so
    acc == 1 and d acc cancels to rounding (the float32 oracle's own error there is 1e-2 .. 1e2 of the gradient: nothing would fail).
    Tiny mode has no |rd| to shorten the ray with, so here the recipe's densities are divided by 32 (optical depth ~ 1) and the far
    sample's is made negative (alpha = 0): acc < 1 on every ray."""
    x = _inputs(s, 2000 + s, "tiny")
    x["raw"][..., 3] /= 32.0
    x["raw"][:, -1, 3] = -x["raw"][:, -1, 3].abs() - 1e-2
    _keep_relu_argument_off_zero(x)
    assert float(O.render_volume_density(x["raw"].double(), x["z"].double())[2].max()) < 0.99
    _check(x, _cotangents(x, 8000 + s, "d_acc"), "tiny", False, gpu, f"alone d_acc tiny thin S={s}", alone=True)


@pytest.mark.parametrize("with_bg,white", [(False, True), (True, False)])
@pytest.mark.parametrize("s", [64, 320])
def test_full_backward_translucent(hip_lib, gpu, s, with_bg, white):
    x = _inputs(s, 3000 + s, "nerface", with_bg, False, "translucent")
    _check(x, _cotangents(x, 9000 + s), "nerface", white, gpu, f"translucent S={s} bg={int(with_bg)} white={int(white)}",
           k_gate=K_FULL_TRANSLUCENT, k_bg=K_FULL_TRANSLUCENT)


def test_full_backward_refusals(hip_lib, gpu):
    from nerf import ops
    z = lambda *s: torch.zeros(s, device=gpu)
    raw, dep, rd, g = z(3, 1025, 4), z(3, 1025), z(3, 3), z(3, 3)
    with pytest.raises(ValueError, match=r"NF_MAX_CHUNKS = 16 chunks of 64 = 1024"):
        ops.volume_render_bwd_full(raw, dep, rd, None, None, d_rgb=g)
    with pytest.raises(ValueError, match=r"NF_MAX_CHUNKS = 16"):
        ops.render_volume_density_bwd_full(raw, dep, d_rgb=g)
    with pytest.raises(ValueError, match="no cotangent"):
        ops.volume_render_bwd_full(raw[:, :8].contiguous(), dep[:, :8].contiguous(), rd, None, None)
    with pytest.raises(ValueError, match="need_d_bg"):
        ops.volume_render_bwd_full(raw[:, :8].contiguous(), dep[:, :8].contiguous(), rd, None, None, d_rgb=g, need_d_bg=True)
    e = lambda *s: torch.empty(s, device=gpu)
    d_raw, d_bg = ops.volume_render_bwd_full(e(0, 8, 4), e(0, 8), e(0, 3), None, e(0, 3), d_rgb=e(0, 3), need_d_bg=True)     # no rays: a no-op
    assert d_raw.shape == (0, 8, 4) and d_bg.shape == (0, 3)


# ------------------------------------------------------------------------------------------------------------------ 2. today's path
@pytest.mark.parametrize("s", [1, 65, 129, 193, 257, 320, 1024])
def test_rgb_only_equals_todays_kernel(hip_lib, gpu, s):
    from nerf import ops
    for mode, with_bg, noisy, white in (("nerface", True, True, False), ("nerface", False, False, True), ("tiny", False, False, False)):
        x = _inputs(s, 1000 + s, mode, with_bg, noisy)
        dv = lambda t: None if t is None else t.to(gpu).contiguous()
        if mode == "tiny":
            old = ops.render_volume_density_bwd(dv(x["raw"]), dv(x["z"]), dv(x["d_rgb"]))
            new = ops.render_volume_density_bwd_full(dv(x["raw"]), dv(x["z"]), d_rgb=dv(x["d_rgb"]))
        else:
            args = (dv(x["raw"]), dv(x["z"]), dv(x["rd"]), dv(x["noise"]), dv(x["bg"]))
            old = ops.volume_render_bwd(*args, dv(x["d_rgb"]), white)
            new, d_bg = ops.volume_render_bwd_full(*args, d_rgb=dv(x["d_rgb"]), white_background=white)
            assert d_bg is None
        e = _rel_l2(new.cpu(), old.cpu().double())
        print(f"[render-grads] rgb only, S={s} {mode}: full kernel against today's rel_l2 {e:.2e}")
        assert e <= 1e-6, (s, mode, e)


def test_volume_render_function_fast_path_and_full_path(hip_lib, gpu, monkeypatch):
    """volume_render_radiance_field: an rgb-only loss returns exactly what today's entry returns (and never launches the full kernel);
    a loss on all four outputs with a prior that requires grad matches the oracle's float64 autograd."""
    import nerf
    from nerf import ops
    x = _inputs(65, 1065, "nerface", True, False)
    dv = lambda t: None if t is None else t.to(gpu).contiguous()
    raw = dv(x["raw"]).requires_grad_(True)
    full_calls = []
    real_full = ops.volume_render_bwd_full
    monkeypatch.setattr(ops, "volume_render_bwd_full", lambda *a, **k: (full_calls.append(1), real_full(*a, **k))[1])
    rgb, disp, acc, w, _ = nerf.volume_render_radiance_field(raw, dv(x["z"]), dv(x["rd"]), background_prior=dv(x["bg"]))
    assert disp.requires_grad and acc.requires_grad and w.requires_grad
    (rgb * dv(x["d_rgb"])).sum().backward()
    want = ops.volume_render_bwd(raw.detach(), dv(x["z"]), dv(x["rd"]), None, dv(x["bg"]), dv(x["d_rgb"]))
    assert torch.equal(raw.grad, want) and not full_calls
    # every output, prior a leaf
    cot = _cotangents(x, 7065)
    x2 = x
    raw2, bg2 = dv(x["raw"]).requires_grad_(True), dv(x["bg"]).requires_grad_(True)
    rgb, disp, acc, w, _ = nerf.volume_render_radiance_field(raw2, dv(x["z"]), dv(x["rd"]), background_prior=bg2)
    (rgb * dv(cot["d_rgb"])).sum().add((disp * dv(cot["d_third"])).sum()).add((acc * dv(cot["d_acc"])).sum()).add(
        (w * dv(cot["d_w"])).sum()).add((w[:, -1] * dv(cot["d_wlast"])).sum()).backward()
    assert len(full_calls) == 1
    g64, b64 = _oracle_grads(x2, cot, torch.float64, "nerface", False)
    g32, b32 = _oracle_grads(x2, cot, torch.float32, "nerface", False)
    _gate("Function, all outputs", "d_raw", raw2.grad.cpu(), g64, g32, K_FULL)
    _gate("Function, all outputs", "d_bg", bg2.grad.cpu(), b64, b32, K_BG)


# ------------------------------------------------------------------------------------------------------------------ 3. end to end
def _run_product(nerf, c, gpu, bg):
    """tests.util.run_product in train mode with gradients, with the caller's background prior (a tensor that may require grad)."""
    mc = U.make_model(nerf, c["p_coarse"], gpu)
    mf = U.make_model(nerf, c["p_fine"], gpu)
    opt = U.make_options(nerf, c["n_coarse"], c["n_fine"], bool(c["stochastic"]), c["noise_std"], 65536, lindisp=bool(c.get("lindisp", False)))
    ex, ed = U.encoders(nerf)
    latent = c["latent"].clone().to(gpu).requires_grad_(True)
    rands, randns = U.case_random_lists(c)
    with torch.enable_grad(), U.injected_random(rands, randns):
        out = nerf.run_one_iter_of_nerf(512, 512, None, mc, mf, c["ro"].to(gpu), c["rd"].to(gpu), opt, mode="train", encode_position_fn=ex,
                                        encode_direction_fn=ed, expressions=c["expr"].to(gpu), background_prior=bg, latent_code=latent)
    return out, mc, mf, latent


def _seven_weights(c, seed=4242):
    g = torch.Generator().manual_seed(seed)
    n = c["ro"].shape[0]
    return [torch.randn(s, generator=g) for s in ((n, 3), (n,), (n,), (n, 3), (n,), (n,), (n,))]


def _oracle_seven(c, ws, dtype):
    """The oracle's autograd in `dtype` of L = sum_i <output_i, ws_i> over the 7-tuple: (parameter grads, latent grad, bg grad)."""
    d = lambda t: None if t is None else t.to(dtype)
    pc = {k: d(v).clone().requires_grad_(True) for k, v in c["p_coarse"].items()}
    pf = {k: d(v).clone().requires_grad_(True) for k, v in c["p_fine"].items()}
    lat, bg = d(c["latent"]).clone().requires_grad_(True), d(c["bg"]).clone().requires_grad_(True)
    o = O.render_rays(pc, pf, d(c["ro"]), d(c["rd"]), d(c["expr"]), lat, bg, O.NEAR, O.FAR, c["n_coarse"], c["n_fine"], t_rand=d(c["t_rand"]),
                      noise_c=d(c["noise_c"]), u=d(c["u"]), noise_f=d(c["noise_f"]))
    sum((a * d(w)).sum() for a, w in zip(o, ws)).backward()
    return pc, pf, lat.grad, bg.grad


_E2E = {}


def _e2e_reference(case):
    if case not in _E2E:                                     # computed once, shared by the three tests of a case, never written to
        c = C.build_case(case)
        ws = _seven_weights(c)
        _E2E[case] = (c, ws, _oracle_seven(c, ws, torch.float64), _oracle_seven(c, ws, torch.float32)[3])
    return _E2E[case]


def _check_e2e(case, out, mc, mf, latent, bg_grad, gpu):
    """Parameter and latent gradients at the gates tests/test_gpu_backward.py holds this case's family to (soft no-flip frame: 1e-4 per
    tensor, NOFLIP_GATE; hard family: 2e-2 per tensor, median 2e-4, at most MAX_LOOSE_TENSORS above 1.5e-3; latent 1e-4); d_bg at the
    integrator gate of this file (K_BG x the float32 oracle's own error per ray, rel_l2 < 2e-5)."""
    c, ws, (pc, pf, lat_g, bg_g), bg_g32 = _e2e_reference(case)
    errs = []
    for tag, m, po in (("coarse", mc, pc), ("fine", mf, pf)):
        for k, v in m.named_parameters():
            if k.startswith("layers_dir.3"):
                assert v.grad is None
                continue
            errs.append(_rel_l2(v.grad.cpu(), po[k].grad))
    errs.sort()
    e_lat = _rel_l2(latent.grad.cpu(), lat_g)
    print(f"[render-grads] e2e {case}: worst param rel_l2 {errs[-1]:.2e} median {errs[len(errs) // 2]:.2e} latent {e_lat:.2e}")
    if case == "soft_train_noflip_64_64":
        assert errs[-1] < 1e-4 and e_lat < 1e-4, (errs[-4:], e_lat)
    else:
        assert errs[-1] < 2e-2 and errs[len(errs) // 2] < 2e-4 and sum(e >= 1.5e-3 for e in errs) <= 4 and e_lat < 1e-4, (errs[-6:], e_lat)
    _gate(f"e2e {case}", "d_bg", bg_grad, bg_g, bg_g32, K_BG)


def _seven_loss(out, ws, gpu):
    return sum((a * w.to(gpu)).sum() for a, w in zip(out, ws))


@pytest.mark.parametrize("prior_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("case", ["soft_train_noflip_64_64", "ragged_5_7"])
def test_train_step_through_all_seven_outputs(hip_lib, gpu, case, prior_dtype):
    import nerf
    c, ws = _e2e_reference(case)[:2]
    bg = c["bg"].to(device=gpu, dtype=prior_dtype).requires_grad_(True)
    out, mc, mf, latent = _run_product(nerf, c, gpu, bg)
    assert all(o.requires_grad for o in out)
    _seven_loss(out, ws, gpu).backward()
    assert bg.grad is not None and bg.grad.dtype == prior_dtype and bg.grad.shape == bg.shape
    _check_e2e(case, out, mc, mf, latent, bg.grad.cpu(), gpu)


@pytest.mark.parametrize("flat", [False, True])
def test_train_step_background_through_get_ray_batch(hip_lib, gpu, flat):
    import nerf
    case = "soft_train_noflip_64_64" if flat else "ragged_5_7"
    c, ws = _e2e_reference(case)[:2]
    n, hw = c["ro"].shape[0], 16
    g = torch.Generator().manual_seed(99)
    pix = torch.randperm(hw * hw, generator=g)[:n]
    image = torch.rand((hw, hw, 3), generator=g)
    image.view(-1, 3)[pix] = c["bg"]
    background = image.to(gpu).requires_grad_(True)
    sel = (pix if flat else torch.stack((pix // hw, pix % hw), dim=1)).to(gpu)
    _, _, _, bg = nerf.get_ray_batch(hw, hw, O.INTRINSICS, O.frame_pose(3).to(gpu), sel, None, background)
    assert bg.requires_grad and torch.equal(bg.detach().cpu(), c["bg"])
    out, mc, mf, latent = _run_product(nerf, c, gpu, bg)
    _seven_loss(out, ws, gpu).backward()
    grad = background.grad.cpu().view(-1, 3)
    off = torch.ones(hw * hw, dtype=torch.bool)
    off[pix] = False
    assert float(grad[off].abs().max()) == 0.0
    _check_e2e(case, out, mc, mf, latent, grad[pix], gpu)


def test_render_chunk_fast_path_rule(hip_lib, gpu, monkeypatch):
    """A pass whose only cotangent is d_rgb, with a prior that needs no gradient, makes exactly today's calls: two launches of
    ops.volume_render_bwd, none of the full kernel, and the gradients it hands on are that entry's own output."""
    import nerf
    from nerf import ops
    c = C.build_case("soft_train_noflip_64_64")
    calls = dict(old=[], full=0)
    real_old, real_full = ops.volume_render_bwd, ops.volume_render_bwd_full

    def old(*a, **k):
        r = real_old(*a, **k)
        calls["old"].append((a, r))
        return r

    def full(*a, **k):
        calls["full"] += 1
        return real_full(*a, **k)

    monkeypatch.setattr(ops, "volume_render_bwd", old)
    monkeypatch.setattr(ops, "volume_render_bwd_full", full)
    seen = []
    real_hb = type(U.make_model(nerf, c["p_coarse"], gpu)).hip_backward
    monkeypatch.setattr(type(U.make_model(nerf, c["p_coarse"], gpu)), "hip_backward",
                        lambda self, state, z, d_raw: (seen.append(d_raw), real_hb(self, state, z, d_raw))[1])
    out, mc, mf, latent = _run_product(nerf, c, gpu, c["bg"].to(gpu))
    O.train_loss(out[0], out[3], c["tgt"].to(gpu), latent).backward()
    assert len(calls["old"]) == 2 and calls["full"] == 0 and len(seen) == 2
    for (a, r), d_raw in zip(calls["old"], seen):
        assert torch.equal(d_raw, real_old(*a)) and d_raw is r                   # a direct call of today's entry on the same inputs
    # the same step with a prior that requires grad takes the full kernel in both passes, and the parameters' gradients agree
    grads = [p.grad.clone() for p in list(mc.parameters()) + list(mf.parameters()) if p.grad is not None]
    calls["old"].clear()
    bg = c["bg"].to(gpu).requires_grad_(True)
    out, mc2, mf2, latent2 = _run_product(nerf, c, gpu, bg)
    O.train_loss(out[0], out[3], c["tgt"].to(gpu), latent2).backward()
    assert calls["full"] == 2 and not calls["old"] and bg.grad is not None
    grads2 = [p.grad for p in list(mc2.parameters()) + list(mf2.parameters()) if p.grad is not None]
    assert len(grads) == len(grads2) and max(_rel_l2(a.cpu(), b.cpu().double()) for a, b in zip(grads2, grads)) <= 1e-6


# ------------------------------------------------------------------------------------------------------------------ 4. the launcher
def _assert_same(a, b, path):
    """Two checkpoints entry by entry: tensors bit for bit, containers by key and length, everything else by ==."""
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b), path
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a.keys()) == list(b.keys()), path
        for k in a:
            _assert_same(a[k], b[k], f"{path}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (u, v) in enumerate(zip(a, b)):
            _assert_same(u, v, f"{path}[{i}]")
    else:
        assert a == b, (path, a, b)


def test_launcher_trains_and_restores_the_background(hip_lib, gpu, tmp_path):
    """5 iterations with a learned, supervised background, a resume, and two runs without the flags.  The last pair is a determinism
    check of the launcher as it stands: two seeded runs write the same checkpoint, every entry of it (both networks, the latent codes,
    the optimizer's moments and groups, iteration, loss and psnr).  It does not by itself tie the flagless launcher to its behaviour
    before the flags existed; the byte-for-byte equality of bench.py's --dump-outputs files in eval and train mode does that for the
    step the launcher drives, and the flagless branch of the launcher builds the optimizer and the loss exactly as before."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))
    import yaml
    import make_synthetic_dataset as MS
    import nerf
    from launch import train_sharded
    base = str(tmp_path)
    MS.write(os.path.join(base, "data"))

    def run(tag, iters, *flags):
        cfg = MS.config(os.path.join(base, "data"), os.path.join(base, "logs_" + tag))
        cfg["experiment"]["train_iters"] = iters
        cfg["experiment"]["validate_every"] = 1000                               # (validation at iteration 0 only)
        path = os.path.join(base, f"config_{tag}_{iters}.yml")
        with open(path, "w") as f:
            yaml.safe_dump(cfg, f)
        logdir = train_sharded.main(["--config", path, *flags])
        return logdir, torch.load(os.path.join(logdir, "checkpoint" + str(iters - 1).zfill(5) + ".ckpt"), map_location="cpu")

    # 5 iterations with a learned, supervised background
    logdir, ck = run("bg", 5, "--train-background", "--supervised-background")
    images = nerf.load_flame_data(os.path.join(base, "data"), half_res=False, testskip=1)
    mean = torch.mean(images[0][torch.as_tensor(np.asarray(images[4][0]), dtype=torch.long)][..., :3].float(), dim=0)
    assert ck["background"].shape == mean.shape and bool(torch.isfinite(ck["background"]).all())
    assert not torch.equal(ck["background"], mean) and float((ck["background"] - mean).abs().max()) < 0.1      # 5 Adam steps from the mean image
    opt = ck["optimizer_state_dict"]
    assert len(opt["param_groups"]) == 2 and len(opt["param_groups"][1]["params"]) == 1
    st = opt["state"][opt["param_groups"][1]["params"][0]]                      # the second group is stepped: it has Adam moments
    assert st["exp_avg"].shape == mean.shape and float(st["exp_avg"].abs().max()) > 0
    # a resume restores the background into the tensor the optimizer owns and goes on training it
    cfg_path = os.path.join(base, "config_bg_5.yml")
    train_sharded.main(["--config", cfg_path, "--load-checkpoint", os.path.join(logdir, "checkpoint00004.ckpt"), "--train-background"])
    ck2 = torch.load(os.path.join(logdir, "checkpoint00004.ckpt"), map_location="cpu")      # rewritten by the resumed iteration
    moved, step = float((ck["background"] - mean).abs().max()), float((ck2["background"] - ck["background"]).abs().max())
    print(f"[render-grads] launcher: background moved {moved:.2e} from the mean image in 5 steps, {step:.2e} in the resumed one")
    assert 0 < step < 0.5 * moved                   # one Adam step (~lr) from the checkpoint; a restart from the mean would be ~4 steps away
    # without the flags the background is the file's, it never moves and its group stays inert
    _, a = run("plain_a", 3)
    _, b = run("plain_b", 3)
    from launch import common as CM
    fixed = CM.load_background(os.path.join(base, "data"), 32, 32, "cpu")
    assert torch.equal(a["background"], fixed) and torch.equal(b["background"], fixed)
    oa = a["optimizer_state_dict"]
    assert oa["param_groups"][1]["params"][0] not in oa["state"]
    _assert_same(a, b, "checkpoint")               # determinism: every entry of the checkpoint (it holds no time stamps)
