"""Every size-dispatched path of the render kernels (csrc/nf_render.hip), per element, against the float64 oracle.  GPU only.

The integrator backward is a template over the number of 64-sample chunks per ray (k_volume_render_bwd<1|2|3|4|8|16>), the sampler,
the row sort and the fused resample + merge size wave-private tables at compile time (NF_MAX_BINS 512, NF_MAX_SORT 1024,
NF_MAX_CHUNKS 16).  This file runs

  A  the integrator, forward and backward, NeRFace mode and tiny mode, at sample counts on both sides of every chunk boundary and
     of every template of the dispatch (S_ALL; chunks per ray = ceil(S / 64): 1 1 1 1 | 2 2 | 3 3 | 4 4 | 5 5 8 -> <8> | 9 16 16 -> <16>),
     with 9 rays (a workgroup holds 4: the last one is partial);
  B  the regimes random densities never reach (an opaque wall, an empty ray, duplicate depths, |rd| of 1e3 and 1e-3, a ray whose far
     sample is translucent, non-finite inputs) at S = 64, 320, 1024;
  C  sampler, row sort and resample + merge AT their limits, and the refusal of every size beyond them: a ValueError that names the
     limit, raised before anything is allocated or launched;
  D  one training step at 64 + 256 samples (fine pass: 320 samples, template <8>) against the oracle's float64 autograd.

The backward gate.  For every ray, e = max |d_raw - g| / max |g| (both maxima over the ray's samples and channels, g = float64
autograd of the oracle).  The yardstick is the oracle itself evaluated in float32 on the CPU on the same inputs (its own autograd):
floor = max(e of the float32 oracle, 1e-7), per ray, and the kernel must stay within K_GATE x floor on every ray (the constants below).  The inputs keep the
ReLU argument away from zero (|raw_sigma + noise| < 1e-2 is replaced by 0.5), so no element is excluded for a rounding flip.
"""
import pytest
import torch

from oracle import cases as C
from oracle import nerface_oracle as O
from tests import util as U

pytestmark = pytest.mark.gpu

S_ALL = [1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 512, 513, 1000, 1024]
S_REGIMES = [64, 320, 1024]
N_RAYS = 9                       # not a multiple of the 4 rays of a workgroup: the `ray >= n_rays` return is taken
ABS_FLOOR = 1e-7                 # floor of the floor: rays on which the float32 oracle happens to be exact
# K_GATE = twice the worst kernel / floor ratio measured on an MI355X over the cases the issue sets, rounded up to an integer.
# Measured worst ratio per case group (per ray; floor = float32 oracle against float64, kernel = HIP against float64):
#   A, NeRFace mode, template <1> 1.9  <2> 1.6  <3> 2.4  <4> 2.4  <8> 3.9  <16> 6.1       A, tiny mode, <1> .. <16>: 1.4 .. 1.8
#   B (S = 64 / 320 / 1024)  wall first 1.2 1.0 1.2 | wall middle 0.9 1.2 1.0 | wall last 1.2 1.0 1.8 | empty <= 1.4 | duplicate 1.4 1.1 1.2
#                            (tiny mode the same within 0.4) | |rd| 1e3: 1.0 1.7 1.2 | |rd| 1e-3: 1.4 1.3 1.3
# |rd| = 1e3 measured 1.0 / 32.1 / 16.4 while the backward formed sum_{j>s} dw_j w_j as total - prefix (rounding error eps |total|
# behind an almost opaque sample, then divided by its b); summed from the far end it is 1.7 at most (csrc/nf_render.hip).
K_GATE = 13
# The translucent ray (a regime of this file's own, not the issue's: the one input on which the white-background term has a gradient)
# measures 3.4 / 7.8 / 16.4 at S = 64 / 320 / 1024 and is gated on its own, again at twice the worst ratio.  Its 16.4 is the device
# expf, not the kernel's sums: every alpha there is 1 - exp(-x) at x ~ 2e-3, which amplifies the rounding of exp 500 times, and the
# float32 oracle runs on the host's exp (test_translucent_ratio_follows_the_rounding_of_exp replays the kernel's arithmetic on the host:
# 1.5 with the host exp, 48 with +-1 ulp on it).
K_TRANSLUCENT = 33
# |rd| = 1e-3: every alpha is 1 - exp(-x) with x ~ 1e-5, of which float32 keeps two digits, so float32 itself misses or grazes two of
# the project's gates: the float32 ORACLE's gradient has a rel_l2 of 8.1e-5 / 4.5e-4 / 1.3e-3 against float64 (gate 2e-5) at S = 64 / 320 /
# 1024, and its weights are 9.3e-8 / 3.2e-7 / 6.7e-7 from float64 on the MI355X machine's host and 2.8e-7 / 9.0e-7 / 1.7e-6 on another
# (gate 2e-6): the far sample's weight is a product of up to 1023 such (1 - alpha), and how exp rounds decides it.  These two outputs
# of this regime alone are gated at a multiple of the float32 oracle's own error (never below the project's gate), twice the worst
# kernel / oracle ratio measured on the MI355X machine, rounded up: weights 5.5 / 6.3 / 6.2 -> 13 (kernel 5.1e-7 / 2.0e-6 / 4.2e-6),
# rel_l2 1.08 / 1.06 / 1.09 -> 3.  Colour, accumulation and disparity keep the project's gates there, as every output does elsewhere.
RD_SHORT_FLOOR_FACTORS = dict(w=13.0, rel_l2=3.0)


# ------------------------------------------------------------------------------------------------------------------ inputs
def _keep_relu_argument_off_zero(x):
    pre = x["raw"][..., 3] + (0.0 if x["noise"] is None else x["noise"])
    x["raw"][..., 3] = torch.where(pre.abs() < 1e-2, 0.5 - (0.0 if x["noise"] is None else x["noise"]), x["raw"][..., 3])
    pre = x["raw"][..., 3] + (0.0 if x["noise"] is None else x["noise"])
    assert float(pre.abs().min()) >= 9e-3          # the share of elements excluded for a rounding flip is zero


def _inputs(s, seed, mode="nerface", with_bg=True, noisy=False, regime=None, n_rays=N_RAYS):
    """float32 CPU tensors of one case.  Densities ~ N(0, 16^2) and depths in [0.2, 0.8] (tiny mode: [2, 6]) as the existing integrator
    tests draw them; `regime` then rewrites what it is about."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn((n_rays, s, 4), generator=g) * 2.0
    raw[..., 3] *= 8.0
    lo, span = (2.0, 4.0) if mode == "tiny" else (0.2, 0.6)
    z = torch.sort(torch.rand((n_rays, s), generator=g) * span + lo, dim=-1)[0]
    rd = torch.randn((n_rays, 3), generator=g)
    bg = torch.rand((n_rays, 3), generator=g)
    noise = torch.randn((n_rays, s), generator=g) * 0.1
    d_rgb = torch.randn((n_rays, 3), generator=g)
    x = dict(raw=raw, z=z, rd=rd, bg=bg if (with_bg and mode == "nerface") else None, noise=noise if (noisy and mode == "nerface") else None,
             d_rgb=d_rgb)
    unit = rd / rd.norm(dim=-1, keepdim=True)
    if regime in ("wall_first", "wall_mid", "wall_last"):
        # every density negative but one of 3e4: evenly spaced depths and 1.5 <= |rd| <= 2.5 make its alpha round to 1.0f at every S
        # (3e4 x 0.6 / 1023 x 1.5 = 26; tiny mode: spacing 4 / 1023), i.e. b = 1e-10 and a transmittance of 1e-10 behind it
        raw[..., 3] = -raw[..., 3].abs() - 1e-2
        at = dict(wall_first=min(3, s - 2), wall_mid=s // 2 + 1, wall_last=s - 2)[regime]
        raw[:, at, 3] = 3e4
        x["z"] = (torch.linspace(lo, lo + span, s)[None, :] * torch.ones((n_rays, 1))).contiguous()
        x["rd"] = unit * (1.5 + torch.rand((n_rays, 1), generator=g))
    elif regime == "empty":
        raw[..., 3] = -raw[..., 3].abs() - 1e-2
    elif regime == "duplicate":
        z[:, 1::2] = z[:, 0:2 * (s // 2):2]                   # every other depth equals its neighbour: dist == 0
    elif regime == "rd_long":
        x["rd"] = unit * 1e3
    elif regime == "rd_short":
        x["rd"] = unit * 1e-3
    elif regime == "translucent":
        # The far sample (dist = 1e10 |rd|) is opaque for any |rd| a camera produces, so acc == 1 and (1 - acc), the white-background
        # term, has no gradient: in the backward it cancels to rounding.  Here it does not: depths over [0, 1e10], |rd| = 2.5e-10 and
        # densities ~ N(0, 1) give a total optical depth near 1 and a far sample of alpha = 1 - exp(-2.5 sigma), so acc < 1 on every ray.
        raw[..., 3] /= 16.0
        raw[:, -1, 3] = raw[:, -1, 3].abs().clamp(min=1e-2)
        x["z"] = torch.sort(torch.rand((n_rays, s), generator=g) * 1e10, dim=-1)[0]
        x["rd"] = unit * 2.5e-10
    else:
        assert regime is None, regime
    _keep_relu_argument_off_zero(x)
    return x


# ------------------------------------------------------------------------------------------------------------------ oracle and product
def _oracle(x, dtype, mode, white, backward=True):
    cv = lambda t: None if t is None else t.to(dtype)
    raw = cv(x["raw"]).clone().requires_grad_(backward)
    if mode == "tiny":
        rgb, third, acc = O.render_volume_density(raw, cv(x["z"]))
        w = None
    else:
        bg, raw_in = cv(x["bg"]), raw
        if bg is not None:                                  # T:95-96: the overwrite kills the gradient of the last colour
            raw_in = torch.cat((raw[:, :-1], torch.cat((bg[:, None, :], raw[:, -1:, 3:]), dim=-1)), dim=1)
        rgb, third, acc, w = O.volume_render(raw_in, cv(x["z"]), cv(x["rd"]), cv(x["noise"]), has_background=bg is not None,
                                            white_background=white)
    out = dict(rgb=rgb.detach(), third=third.detach(), acc=acc.detach(), w=None if w is None else w.detach())
    if backward:
        rgb.backward(cv(x["d_rgb"]))
        out["g"] = raw.grad
    return out


def _product(x, mode, white, gpu, backward=True):
    from nerf import ops
    dv = lambda t: None if t is None else t.to(gpu).contiguous()
    raw, z, d_rgb = dv(x["raw"]), dv(x["z"]), dv(x["d_rgb"])
    if mode == "tiny":
        rgb, third, acc = ops.render_volume_density(raw, z)
        out = dict(rgb=rgb, third=third, acc=acc, w=None)
        if backward:
            out["g"] = ops.render_volume_density_bwd(raw, z, d_rgb)
    else:
        rd, noise, bg = dv(x["rd"]), dv(x["noise"]), dv(x["bg"])
        rgb, third, acc, w = ops.volume_render_fwd(raw, z, rd, noise, bg, white)
        out = dict(rgb=rgb, third=third, acc=acc, w=w)
        if backward:
            out["g"] = ops.volume_render_bwd(raw, z, rd, noise, bg, d_rgb, white)
    return {k: (None if v is None else v.cpu()) for k, v in out.items()}


def _ray_err(d, g):
    """max |d - g| / max |g| per ray; a ray whose reference gradient is all zero is measured absolutely."""
    scale = g.abs().amax(dim=(1, 2))
    return (d.double() - g).abs().amax(dim=(1, 2)) / torch.where(scale > 0, scale, torch.ones_like(scale))


def _check(x, mode, white, gpu, tag, acc_is_one=None, k_gate=None, floor_factors=None):
    """Forward at the project's gates, backward per ray at k_gate x the live float32 floor beside the whole-tensor rel_l2 < 2e-5.
    floor_factors (|rd| = 1e-3 only, see RD_SHORT_FLOOR_FACTORS): outputs whose gate is a multiple of the float32 oracle's own error."""
    k_gate = K_GATE if k_gate is None else k_gate
    ref, ref32, got = _oracle(x, torch.float64, mode, white), _oracle(x, torch.float32, mode, white), _product(x, mode, white, gpu)
    for k, v in ref.items():
        assert v is None or bool(torch.isfinite(v).all()), (tag, "oracle", k)
    for k, v in got.items():
        assert v is None or bool(torch.isfinite(v).all()), (tag, k)
    # ---- forward: the project's gates (tests/test_gpu_kernels.py::test_volume_render_fwd, tests/test_gpu_tiny.py) -----------------
    e_rgb = float((got["rgb"].double() - ref["rgb"]).abs().max())
    e_acc = float((got["acc"].double() - ref["acc"]).abs().max())
    if mode == "tiny":
        e_w, f_w, e_third = 0.0, 0.0, float((got["third"].double() - ref["third"]).abs().max())         # depth map (depths in [2, 6])
        third_gate = 2e-5
    else:
        e_w, f_w = float((got["w"].double() - ref["w"]).abs().max()), float((ref32["w"].double() - ref["w"]).abs().max())
        e_third, third_gate = float(((got["third"].double() - ref["third"]).abs() / ref["third"].abs()).max()), 1e-5     # disparity
    # ---- backward: per ray and element against the live float32 floor ------------------------------------------------------------
    g = ref["g"]
    raw_floor = _ray_err(ref32["g"], g)
    err = _ray_err(got["g"], g)
    ratio = err / raw_floor.clamp(min=ABS_FLOOR)
    l2 = float((got["g"].double() - g).norm() / (g.norm() + 1e-30))
    f_l2 = float((ref32["g"].double() - g).norm() / (g.norm() + 1e-30))
    print(f"[render-sizes] {tag}: fwd w {e_w:.1e} (float32 oracle {f_w:.1e}) rgb {e_rgb:.1e} acc {e_acc:.1e} third {e_third:.1e} | bwd floor "
          f"{float(raw_floor.max()):.2e} kernel {float(err.max()):.2e} worst ratio {float(ratio.max()):.2f} rel_l2 {l2:.1e} (float32 oracle {f_l2:.1e})")
    w_gate, l2_gate = 2e-6, 2e-5
    if floor_factors is not None:
        w_gate, l2_gate = max(w_gate, floor_factors["w"] * f_w), max(l2_gate, floor_factors["rel_l2"] * f_l2)
    assert e_w < w_gate and e_rgb < 5e-6 and e_acc < 5e-6 and e_third < third_gate, (tag, e_w, w_gate, e_rgb, e_acc, e_third)
    if acc_is_one if acc_is_one is not None else x["bg"] is not None:
        assert float((got["acc"] - 1).abs().max()) < 1e-5, tag                  # Q5: alpha_last == 1 -> acc == 1
    assert float(ratio.max()) <= k_gate, (tag, ratio.tolist())
    assert l2 < l2_gate, (tag, l2, l2_gate)
    if x["bg"] is not None:
        assert float(got["g"][:, -1, :3].abs().max()) == 0.0, tag               # the background sample's colour is a constant
    pre = x["raw"][..., 3].double() + (0.0 if x["noise"] is None else x["noise"].double())
    assert float(got["g"][..., 3][pre <= 0].abs().max() if bool((pre <= 0).any()) else 0.0) == 0.0, tag
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------------------------ A
# (background prior, density noise, white background): each value of each switch runs at every S, hence with every template
SWITCHES = [(True, True, False), (False, False, True), (True, False, True)]


@pytest.mark.parametrize("with_bg,noisy,white", SWITCHES)
@pytest.mark.parametrize("s", S_ALL)
def test_integrator_every_chunk_template_nerface(hip_lib, gpu, s, with_bg, noisy, white):
    x = _inputs(s, 1000 + s, "nerface", with_bg, noisy)
    _check(x, "nerface", white, gpu, f"A nerface S={s} bg={int(with_bg)} noise={int(noisy)} white={int(white)}")


@pytest.mark.parametrize("s", S_ALL)
def test_integrator_every_chunk_template_tiny(hip_lib, gpu, s):
    x = _inputs(s, 2000 + s, "tiny")
    _check(x, "tiny", False, gpu, f"A tiny S={s}")


# ------------------------------------------------------------------------------------------------------------------ B
REGIMES = ([("nerface", r, True, False) for r in ("wall_first", "wall_mid", "wall_last", "duplicate", "rd_long", "rd_short")]
           + [("nerface", "empty", False, False), ("nerface", "empty", True, True), ("nerface", "translucent", False, True)]
           + [("tiny", r, False, False) for r in ("wall_first", "wall_mid", "wall_last", "empty", "duplicate")])


@pytest.mark.parametrize("mode,regime,with_bg,white", REGIMES)
@pytest.mark.parametrize("s", S_REGIMES)
def test_integrator_regimes(hip_lib, gpu, s, mode, regime, with_bg, white):
    x = _inputs(s, 3000 + s, mode, with_bg, False, regime)
    if regime.startswith("wall") or regime == "empty":
        pre = x["raw"][..., 3]
        assert int((pre > 0).sum()) == (N_RAYS if regime != "empty" else 0)
    if regime == "duplicate":
        assert int((x["z"][:, 1:] == x["z"][:, :-1]).sum()) >= N_RAYS * (s // 2)
    _check(x, mode, white, gpu, f"B {mode} {regime} S={s} bg={int(with_bg)} white={int(white)}",
           acc_is_one=False if regime in ("translucent", "rd_short") else None,      # (rd_short: the far sample's alpha is 1 - exp(-10))
           k_gate=K_TRANSLUCENT if regime == "translucent" else K_GATE,
           floor_factors=RD_SHORT_FLOOR_FACTORS if regime == "rd_short" else None)


def _replay_backward_f32(x, white, exp_ulp=0):
    """The arithmetic of k_volume_render_bwd (NeRFace mode, no noise) replayed in float32 torch on the host, sums in sequence instead
    of wave scans.  exp_ulp > 0 adds a seeded error of up to that many units in the last place to every exp (drawn from -ulp .. ulp)
    on top of a correctly rounded one."""
    raw, z, grad = x["raw"], x["z"], x["d_rgb"]
    n = raw.shape[0]

    def exp(t):
        e = torch.exp(t.double()).float()
        if exp_ulp:
            k = torch.randint(-exp_ulp, exp_ulp + 1, e.shape, generator=torch.Generator().manual_seed(5))
            e = (e.view(torch.int32) + k.to(torch.int32)).view(torch.float32)
        return e if exp_ulp else torch.exp(t)

    dist = torch.cat((z[:, 1:] - z[:, :-1], torch.full((n, 1), 1e10)), -1) * x["rd"].norm(dim=-1, keepdim=True)
    c = 1.0 / (1.0 + exp(-raw[..., :3]))
    if x["bg"] is not None:
        c[:, -1] = x["bg"]
    pre = raw[..., 3]
    sigma = torch.relu(pre).clone()
    sigma[:, -1] += 1e-6
    alpha = 1.0 - exp(-sigma * dist)
    b = 1.0 - alpha + 1e-10
    t_incl = torch.cumprod(b, -1)
    trans = torch.cat((torch.ones(n, 1), t_incl[:, :-1]), -1)
    w = alpha * trans
    dw = (c * grad[:, None, :]).sum(-1) - (grad.sum(-1, keepdim=True) if white else 0.0)
    v = dw * w
    suffix = torch.cat((torch.flip(torch.cumsum(torch.flip(v[:, 1:], [-1]), -1), [-1]), torch.zeros(n, 1)), -1)
    d_sigma = (dw * trans - suffix / b) * dist * (1.0 - alpha)
    out = torch.zeros_like(raw)
    out[..., :3] = w[..., None] * grad[:, None, :] * c * (1.0 - c)
    if x["bg"] is not None:
        out[:, -1, :3] = 0.0
    out[..., 3] = torch.where(pre > 0, d_sigma, torch.zeros_like(d_sigma))
    return out


def test_translucent_ratio_follows_the_rounding_of_exp():
    """Why the translucent ray has a gate of its own (K_TRANSLUCENT): its ratio is set by how exp rounds, not by how the kernel sums.
    The kernel's formulas in float32 on the host stay within K_GATE of the float32 oracle with the host's exp and leave 16 behind as
    soon as exp is allowed one unit in the last place, which is what the device's expf is specified to."""
    x = _inputs(1024, 3000 + 1024, "nerface", False, False, "translucent")
    g = _oracle(x, torch.float64, "nerface", True)["g"]
    floor = _ray_err(_oracle(x, torch.float32, "nerface", True)["g"], g).clamp(min=ABS_FLOOR)
    worst = {ulp: float((_ray_err(_replay_backward_f32(x, True, ulp), g) / floor).max()) for ulp in (0, 1)}
    print(f"[render-sizes] B translucent S=1024, host replay of the kernel's arithmetic: worst ratio {worst[0]:.1f} with the host exp, "
          f"{worst[1]:.1f} with +-1 ulp on exp")
    assert worst[0] <= K_GATE and worst[1] > 16.0, worst


@pytest.mark.parametrize("s", S_REGIMES)
def test_integrator_nonfinite_inputs_forward(hip_lib, gpu, s):
    """One +inf and one NaN in raw (the density channel: what a diverged model produces) and in z: weights and colours are non-finite
    exactly where the float32 oracle's are (torch.relu keeps a NaN).  No values compared, no backward, on such rows."""
    x = _inputs(s, 4000 + s, "nerface", True, False)
    x["raw"][0, s // 3, 3] = float("inf")
    x["raw"][1, s // 2, 3] = float("nan")
    x["z"][2, s // 2] = float("inf")
    x["z"][3, 5] = float("nan")
    x["raw"][4, s // 4, 1] = float("nan")                       # and a NaN colour: the ray's green only
    ref32 = _oracle(x, torch.float32, "nerface", False, backward=False)
    got = _product(x, "nerface", False, gpu, backward=False)
    for k in ("w", "rgb"):
        assert torch.equal(torch.isnan(got[k]), torch.isnan(ref32[k])), (k, torch.isnan(got[k]).sum(), torch.isnan(ref32[k]).sum())
    assert bool(torch.isnan(ref32["w"][1]).any()) and bool(torch.isnan(ref32["rgb"][4, 1])) and not bool(torch.isnan(ref32["rgb"][4, 0]))
    clean = ~(torch.isnan(ref32["w"]).any(-1) | torch.isnan(ref32["rgb"]).any(-1) | torch.isinf(x["z"]).any(-1))
    assert int(clean.sum()) >= N_RAYS - 5
    ref = _oracle(x, torch.float64, "nerface", False, backward=False)
    assert float((got["w"][clean].double() - ref["w"][clean]).abs().max()) < 2e-6
    assert float((got["rgb"][clean].double() - ref["rgb"][clean]).abs().max()) < 5e-6


# ------------------------------------------------------------------------------------------------------------------ C: at the limits
def _near_knot(u, cdf, tol=4e-7):
    """u within tol of a table entry (the nearest entry is one of the two around its insertion point)."""
    hi = torch.searchsorted(cdf.contiguous(), u.contiguous()).clamp(max=cdf.shape[-1] - 1)
    lo = (hi - 1).clamp(min=0)
    return torch.minimum((u - cdf.gather(1, lo)).abs(), (u - cdf.gather(1, hi)).abs()) <= tol


def _pdf_inputs(n_bins, n_out):
    n_rays = 300 if n_out >= 64 else 20000                      # enough draws that the knot share is not a handful of them
    g = torch.Generator().manual_seed(900 + n_bins + n_out)
    bins = torch.sort(torch.rand((n_rays, n_bins), generator=g) * 0.6 + 0.2, dim=-1)[0]
    w = torch.rand((n_rays, n_bins - 1), generator=g) ** 4
    u = torch.rand((n_rays, n_out), generator=g)
    return bins, w, u


@pytest.mark.parametrize("n_out", [1, 64, 1000])
@pytest.mark.parametrize("n_bins", [2, 3, 256, 511, 512])
def test_sample_pdf_up_to_the_table_limit(hip_lib, gpu, n_bins, n_out):
    """The live-oracle half of test_sample_pdf_bit_exact at table widths up to NF_MAX_BINS: table within 2.4e-7, indices equal away
    from the knots, samples within 2e-6; the share of abscissae near a knot (expected n_bins x 8e-7) stays below 1e-3."""
    from nerf import ops
    bins, w, u = _pdf_inputs(n_bins, n_out)
    t = {}
    z_o = O.sample_pdf(bins, w, n_out, u, table=t)
    z, inds, cdf = ops.sample_pdf(bins.to(gpu), w.to(gpu), n_out, u.to(gpu), want_table=True)
    near = _near_knot(u, t["cdf"])
    share = float(near.float().mean())
    print(f"[render-sizes] C sample_pdf bins={n_bins} n_out={n_out}: table {float((cdf.cpu() - t['cdf']).abs().max()):.1e} knot share {share:.1e}")
    assert share < 1e-3
    assert float((cdf.cpu() - t["cdf"]).abs().max()) <= 2.4e-7
    assert torch.equal(inds.cpu().long()[~near], t["inds"][~near])
    assert float((z.cpu() - z_o)[~near].abs().max()) < 2e-6


def _same_sorted(got, want):
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(want, nan=-1.0))


@pytest.mark.parametrize("n_cols", [1, 2, 63, 64, 65, 513, 1000, 1023, 1024])
def test_sort_rows_up_to_the_row_limit(hip_lib, gpu, n_cols):
    """7 rows (one partial workgroup) with ties, negative zero, +inf and NaNs: torch.sort's order, NaNs last."""
    from nerf import ops
    g = torch.Generator().manual_seed(50 + n_cols)
    x = torch.rand((7, n_cols), generator=g) - 0.5
    x[:, ::5] = x[:, :1].clone()                                # ties
    x[1, n_cols // 2] = -0.0
    x[1, n_cols // 3] = 0.0
    x[2, n_cols // 2] = float("inf")
    x[3, n_cols // 3] = float("nan")
    x[4, ::3] = float("nan")
    x[5, -1], x[5, 0] = float("nan"), float("inf")
    x[6] = float("nan")
    got = ops.sort_rows(x.to(gpu)).cpu()
    assert _same_sorted(got, torch.sort(x, dim=-1)[0])


@pytest.mark.parametrize("nc,nf", [(513, 511), (256, 768), (140, 884), (3, 1021), (128, 128), (129, 128), (128, 129)])
def test_resample_merge_general_kernel_at_its_limits(hip_lib, gpu, nc, nf):
    """check() of test_resample_merge_fast_path_is_bit_identical at NF_MAX_BINS bins / NF_MAX_SORT merged depths, and on both sides of
    the fast path's border (<= 128 + 128): samples EQUAL ops.sample_pdf's, the merged row EQUALS torch.sort(cat)."""
    from nerf import ops
    g = torch.Generator().manual_seed(70 + nc + nf)
    n_rays = 13
    z_c = torch.sort(torch.rand((n_rays, nc), generator=g) * 0.6 + 0.2, dim=-1)[0]
    w_c = torch.rand((n_rays, nc), generator=g) ** 6
    w_c[::7] = 0.0
    w_c[1::7, nc // 2] = 1.0
    u = torch.rand((n_rays, nf), generator=g)
    u[0, :3] = torch.tensor([0.0, 1.0, 0.999999])
    for uu in (u, None):
        z_f, z_s = ops.resample_merge(z_c.to(gpu), w_c.to(gpu), nf, None if uu is None else uu.to(gpu), want_samples=True)
        bins = 0.5 * (z_c[:, 1:] + z_c[:, :-1])
        want_s = ops.sample_pdf(bins.to(gpu), w_c[:, 1:-1].contiguous().to(gpu), nf, None if uu is None else uu.to(gpu))
        assert torch.equal(z_s, want_s)
        assert torch.equal(z_f, ops.sort_rows(torch.cat((z_c.to(gpu), want_s), dim=-1).contiguous()))
        assert torch.equal(z_f.cpu(), torch.sort(torch.cat((z_c, want_s.cpu()), -1), -1)[0])


# ------------------------------------------------------------------------------------------------------------------ C: refusals
def _refused(fn, match, gpu, allocates_inputs=False):
    """fn() raises a ValueError naming the limit, leaves no allocation behind (the traceback keeps every frame's tensors alive: nothing
    was allocated before the raise either), and the stream still computes."""
    from nerf import ops
    import gc
    gc.collect()                                    # (tracebacks of earlier refusals form cycles: free their tensors now, not mid-call)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match=match) as info:
        fn()
    assert allocates_inputs or torch.cuda.memory_allocated() <= before, str(info.value)
    probe = torch.rand((5, 200), generator=torch.Generator().manual_seed(1))
    assert torch.equal(ops.sort_rows(probe.to(gpu)).cpu(), torch.sort(probe, dim=-1)[0])
    return str(info.value)


def test_sizes_beyond_a_limit_are_refused_by_name_before_launch(hip_lib, gpu):
    from nerf import ops
    z = lambda *shape: torch.zeros(shape, device=gpu)
    bins, w = z(5, 513), z(5, 512)
    assert "513 bins" in _refused(lambda: ops.sample_pdf(bins, w, 64, None), r"NF_MAX_BINS = 512", gpu)
    row = z(3, 1025)
    assert "1025 columns" in _refused(lambda: ops.sort_rows(row), r"NF_MAX_SORT = 1024", gpu)
    z_c, w_c = z(5, 513), z(5, 513)
    assert "1025" in _refused(lambda: ops.resample_merge(z_c, w_c, 512, None), r"NF_MAX_SORT = 1024", gpu)
    z_b, w_b = z(5, 514), z(5, 514)
    _refused(lambda: ops.resample_merge(z_b, w_b, 100, None), r"NF_MAX_BINS = 512", gpu)
    raw, dep, rd, d_rgb = z(3, 1025, 4), z(3, 1025), z(3, 3), z(3, 3)
    assert "1025 samples" in _refused(lambda: ops.volume_render_bwd(raw, dep, rd, None, None, d_rgb), r"NF_MAX_CHUNKS = 16 chunks of 64 = 1024", gpu)
    _refused(lambda: ops.render_volume_density_bwd(raw, dep, d_rgb), r"NF_MAX_CHUNKS = 16", gpu)
    # the tiny trainer: a training step at 1025 samples per ray is refused before its MLP forward (the ray bundle and the depths exist
    # by then: what is checked is that no weight image was packed)
    import tiny_nerf as TN
    model = TN.VeryTinyNerfModel(128, 10).to(gpu)
    pose, focal = O.frame_pose(3).to(gpu), torch.tensor(138.88 * 4 / 100.0)
    _refused(lambda: TN.run_one_iter_of_tinynerf(4, 4, focal, pose, 2.0, 6.0, 1025, None, TN.get_minibatches, 16384, model, 10),
             r"NF_MAX_CHUNKS = 16", gpu, allocates_inputs=True)
    assert not model.__dict__.get("_tiny_images")
    with torch.no_grad():                                   # without gradients there is no backward: the same call renders
        assert TN.run_one_iter_of_tinynerf(4, 4, focal, pose, 2.0, 6.0, 1025, None, TN.get_minibatches, 16384, model, 10).shape == (4, 4, 3)
    # the last accepted sizes launch
    assert ops.sort_rows(z(3, 1024)).shape == (3, 1024) and ops.volume_render_bwd(raw[:, :1024].contiguous(), dep[:, :1024].contiguous(), rd,
                                                                                None, None, d_rgb).shape == (3, 1024, 4)


def _pipeline_case(n_coarse, n_fine, n_rays=5):
    name = f"sizes_{n_coarse}_{n_fine}"
    C.CASES[name] = dict(frame=11, n_rays=n_rays, n_coarse=n_coarse, n_fine=n_fine, stochastic=False, noise_std=0.0, boost="survey")
    try:
        return C.build_case(name)
    finally:
        del C.CASES[name]


def _pipeline_args(nerf, c, gpu, white=False):
    """Everything run_one_iter_of_nerf takes, already on the device (so that a refused call has nothing to allocate)."""
    ex, ed = U.encoders(nerf)
    return dict(opt=U.make_options(nerf, c["n_coarse"], c["n_fine"], False, 0.0, white=white), ex=ex, ed=ed,
                **{k: c[k].to(gpu) for k in ("ro", "rd", "expr", "bg", "latent")})


def _run_pipeline(nerf, a, mc, mf, mode):
    return nerf.run_one_iter_of_nerf(512, 512, None, mc, mf, a["ro"], a["rd"], a["opt"], mode=mode, encode_position_fn=a["ex"],
                                     encode_direction_fn=a["ed"], expressions=a["expr"], background_prior=a["bg"], latent_code=a["latent"])


def _weights_built(model):
    hw = model.__dict__.get("_hip_weights")
    return hw is not None and len(hw._cache) > 0


def test_pipeline_refuses_sample_counts_before_any_launch(hip_lib, gpu):
    """run_one_iter_of_nerf at 513 + 512 samples (either mode), and a coarse-only TRAINING step at 1025 samples, whose forward every
    kernel accepts and whose backward none does: refused by name before the coarse MLP's weight image is even packed.  The same
    coarse-only configuration in validation mode under no_grad needs no backward and renders: the one place the forward integrator
    walks 17 chunks, held to the fuzz gates against the float64 oracle."""
    import nerf
    c = _pipeline_case(513, 512)
    mc, mf, a = U.make_model(nerf, c["p_coarse"], gpu), U.make_model(nerf, c["p_fine"], gpu), _pipeline_args(nerf, c, gpu)
    _refused(lambda: _run_pipeline(nerf, a, mc, mf, "train"), r"NF_MAX_SORT = 1024", gpu)

    def no_grad_validation():
        with torch.no_grad():
            _run_pipeline(nerf, a, mc, mf, "validation")
    _refused(no_grad_validation, r"NF_MAX_SORT = 1024", gpu)
    assert not _weights_built(mc) and not _weights_built(mf)

    c = _pipeline_case(1025, 0)
    mc, a = U.make_model(nerf, c["p_coarse"], gpu), _pipeline_args(nerf, c, gpu)
    msg = _refused(lambda: _run_pipeline(nerf, a, mc, None, "train"), r"NF_MAX_CHUNKS = 16 chunks of 64 = 1024", gpu)
    assert "1025 samples" in msg and not _weights_built(mc)
    with torch.no_grad():
        out = _run_pipeline(nerf, a, mc, None, "validation")
    assert _weights_built(mc) and len(out) == 6 and out[3] is None
    d = lambda t: t.double()
    ref = O.render_rays({k: d(v) for k, v in c["p_coarse"].items()}, None, d(c["ro"]), d(c["rd"]), d(c["expr"]), d(c["latent"]), d(c["bg"]),
                        O.NEAR, O.FAR, 1025, 0)
    err = {n: float((got.cpu().double() - want).abs().max()) for n, got, want in zip(("rgb_c", "disp_c", "acc_c"), out, ref)}
    print(f"[render-sizes] C coarse-only validation, 1025 samples (17 chunks): {err}")
    assert all(bool(torch.isfinite(t).all()) for t in out[:3])
    assert err["rgb_c"] <= 2e-5 and err["disp_c"] <= 2e-5 and err["acc_c"] <= 1e-5, err


# ------------------------------------------------------------------------------------------------------------------ D
def test_training_step_at_64_plus_256_white_background(hip_lib, gpu):
    """loss.backward() through run_one_iter_of_nerf (train, exact f32) at 33 rays, 64 + 256 samples -- the fine pass integrates 320
    samples, k_volume_render_bwd<8> -- with a white background, against the oracle's float64 autograd on the same draws, at the gates
    of tests/test_gpu_fuzz.py::test_fuzz_training_step_gradients (median tensor 2e-4, worst 2e-2, at most 4 above 1.5e-3, loss 2e-6,
    latent 1e-4 where no unit flipped, else 2e-3)."""
    import nerf
    name = "sizes_train_64_256"
    C.CASES[name] = dict(frame=23, n_rays=33, n_coarse=64, n_fine=256, stochastic=True, noise_std=0.1, boost="survey")
    try:
        c = C.build_case(name)
    finally:
        del C.CASES[name]
    nc, nf = 64, 256
    mc, mf = U.make_model(nerf, c["p_coarse"], gpu), U.make_model(nerf, c["p_fine"], gpu)
    opt = U.make_options(nerf, nc, nf, True, c["noise_std"], 65536, white=True)
    ex, ed = U.encoders(nerf)
    rands, randns = U.case_random_lists(c)
    latent = c["latent"].clone().to(gpu).requires_grad_(True)
    with U.injected_random(rands, randns):
        out = nerf.run_one_iter_of_nerf(512, 512, None, mc, mf, c["ro"].to(gpu), c["rd"].to(gpu), opt, mode="train", encode_position_fn=ex,
                                        encode_direction_fn=ed, expressions=c["expr"].to(gpu), background_prior=c["bg"].to(gpu),
                                        latent_code=latent)
    loss = O.train_loss(out[0], out[3], c["tgt"].to(gpu), latent)
    loss.backward()
    d = lambda t: None if t is None else t.double()
    pc = {kk: v.double().clone().requires_grad_(True) for kk, v in c["p_coarse"].items()}
    pf = {kk: v.double().clone().requires_grad_(True) for kk, v in c["p_fine"].items()}
    lat = c["latent"].double().clone().requires_grad_(True)
    o = O.render_rays(pc, pf, d(c["ro"]), d(c["rd"]), d(c["expr"]), lat, d(c["bg"]), O.NEAR, O.FAR, nc, nf, t_rand=d(c["t_rand"]),
                      noise_c=d(c["noise_c"]), u=d(c["u"]), noise_f=d(c["noise_f"]), white_background=True)
    ref_loss = O.train_loss(o[0], o[3], d(c["tgt"]), lat)
    ref_loss.backward()
    rel = lambda a, b: float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
    errs = []
    for m, po in ((mc, pc), (mf, pf)):
        for kk, v in m.named_parameters():
            if po[kk].grad is None or float(po[kk].grad.abs().max()) == 0.0:
                assert v.grad is None or float(v.grad.abs().max()) == 0.0, kk           # dead tensors (Q3) stay dead
                continue
            assert v.grad is not None and bool(torch.isfinite(v.grad).all()), kk
            errs.append(rel(v.grad.cpu(), po[kk].grad))
    errs.sort()
    e_lat = rel(latent.grad.cpu(), lat.grad)
    n_loose = sum(e >= 1.5e-3 for e in errs)
    print(f"[render-sizes] D 33 rays 64+256 white: loss {float(loss):.6f} vs {float(ref_loss):.6f}; {len(errs)} tensors, median "
          f"{errs[len(errs) // 2]:.1e}, worst {errs[-1]:.1e}, above 1.5e-3: {n_loose}; latent {e_lat:.1e}")
    assert abs(float(loss) - float(ref_loss)) <= 2e-6 * max(1.0, abs(float(ref_loss)))
    assert errs[len(errs) // 2] < 2e-4 and errs[-1] < 2e-2 and n_loose <= 4, errs[-6:]
    assert e_lat < (1e-4 if errs[-1] < 1e-4 else 2e-3), e_lat
