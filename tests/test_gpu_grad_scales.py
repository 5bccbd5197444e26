"""The backward of the fused MLP families across the exponent range of the upstream gradient.  GPU only.

The fp16 backward chain carries one power-of-two scale per point (nfb_pow2_scale / nfb_pair_max in csrc/nf_mlp_bf16_machinery.inc,
NFB_BWD_RESCALE in csrc/nf_mlp_split_bwd.inc) and leaves one maximum per dZ section for the fp16 weight-gradient kernel
(`gscale`, csrc/nf_mlp_bf16_dw.hip).  Every other backward test feeds d_raw ~ N(0, 1) of one magnitude; here the magnitude moves
-- as a whole by a power of two (the result must move by the same power BIT FOR BIT: every scale is a power of two, so a scale
applied and not taken out, taken from the wrong lane half or from another section's slot shows as a difference, not as a
tolerance), from point to point, through one channel only, and to zero.

Setup as tests/test_gpu_dw_plans.py: its `poisoned_bwd` (NaN-filled, guard-tailed workspace and gradient image), `_family`, `GATE`
and the fp64 oracle at the ReLU masks the HIP forward saved.  259 points (7 rays x 37 samples: two workgroups and three points) and
21 points (3 x 7: one partial wave tile), inputs behind `tailed()` so that a padding lane reads NaN.  One training forward per
(family, arithmetic, size) serves every pattern.

The fp16 chain does not clamp a point's scale while the point's largest |gradient| lies in [2^-47, 2^73)
(tests/test_split_stream_host.py checks that on the fp64 oracle for every k used here): the paper model's smallest per-point maximum
is 2^-10.9, so its fp16 case runs k = -32 where the others run k = -40.

MEASURED on an MI355X (256 CUs).  Bit for bit: every equivariance case (k = -40 / -32, -14, +14, +40 at 259 points, -14 and +14 at 21)
and the 2^-24 rows of the spread against the same rows at scale 1, in every tensor and the latent gradient of all eight (family,
arithmetic) cases; nothing was not bit for bit.  Worst per-tensor rel-L2 / gate over all patterns and both sizes: exact f32 0.020
(2.0e-6 of 1e-4, the smaller paper model, colours only), split-fp16 0.019 (1.9e-6 of 1e-4, paper, colours only), split-bf16 0.070
(2.8e-5 of 4e-4, paper, the 2^-24 rows alone), split-bf16 + exact dW 0.066; the outlier row 9.5e-7 (fp16) and 1.8e-5 (bf16).
Density only: every colour-branch gradient an exact zero, all-zero d_raw: every element an exact zero, in every case.
Sensitivity, on a scratch build: NFB_BWD_RESCALE without nfb_pair_max (a point's two lane halves pick their own scales) fails the
channel-sparse, spread, outlier and 21-point cases of both fp16 chains against the oracle -- and keeps the equivariance, since both
halves still move together.
"""
import functools

import pytest
import torch

from oracle import nerface_oracle as O
from tests import split_stream_ref as R
from tests import test_gpu_dw_plans as DW
from tests.test_gpu_mlp_fwd_edges import tailed

pytestmark = pytest.mark.gpu
CASES = [("nf_paper", "f32", False), ("nf_paper", "bf16", False), ("nf_paper", "bf16", True), ("nf_paper", "f16", False),
         ("nf_lcode", "f32", False), ("nf_lcode", "bf16", False), ("nf_lcode", "f16", False), ("nf_smaller", "f32", False)]
IDS = [f"{p}-{m}{'-exact_dw' if x else ''}" for p, m, x in CASES]
cases = pytest.mark.parametrize("prefix,mode,exact_dw", CASES, ids=IDS)
N, N_SMALL = 259, 21
# The layers a density-only gradient cannot reach.  Paper and smaller paper model: sigma = fc_alpha(feat), so fc_feat lies on the
# density's path and its gradient is rightly NOT zero; second family: fc_alpha reads x, fc_feat feeds the colours only.
COLOUR_BRANCH = {"nf_paper": ("layers_dir.", "fc_rgb."), "nf_smaller": ("layers_dir.", "fc_rgb."),
                 "nf_lcode": ("layers_dir.", "fc_rgb.", "fc_feat.")}


def check_density_only(prefix, got):
    """Every colour-branch gradient an exact zero; the trunk's (and, where fc_alpha reads feat, fc_feat's) are not."""
    for name, g in got.items():
        if name.startswith(COLOUR_BRANCH[prefix]):
            assert float(g.abs().max()) == 0.0, (name, float(g.abs().max()))
    live = ["layers_xyz.0.weight", "layers_xyz.2.weight", "fc_alpha.weight"] + ([] if prefix == "nf_lcode" else ["fc_feat.weight", "fc_feat.bias"])
    for name in live:
        assert float(got[name].abs().max()) > 0.0, name


@functools.lru_cache(maxsize=None)
def _state(prefix, mode, n):
    """Inputs (tailed), training forward, masks and fp64 inputs of one (family, arithmetic, size); B is the dense N(0, 1) d_raw."""
    from nerf import ops
    gpu = torch.device("cuda:0")
    fam, m, p, keys, expr, latent, _ = DW._family(prefix)
    if prefix != "nf_smaller":
        p0 = R.grad_family_params(prefix)[0]
        assert all(torch.equal(p[k], p0[k]) for k in p)          # the parameters the host test's range check ran on
    ro, rd, z, b = R.grad_inputs(n)
    ro, rd, z = (tailed(t, gpu) for t in (ro, rd, z))
    hw = m.hip_weights()
    pk = hw.get()
    cond = ops.mlp_condition(fam, pk, expr.to(gpu), latent.to(gpu), O.NEAR, O.FAR)
    _, (saved_t,) = ops.mlp_fwd_train(fam, pk, cond, ro, rd, z, packed_b=hw.get_bf16() if mode == "bf16" else None,
                                      packed_h=hw.get_f16() if mode == "f16" else None)
    masks = DW._masks(prefix, saved_t, n, mode)
    x64 = O.encode_points(ro.double(), rd.double(), z.double(), O.NEAR, O.FAR)
    return dict(prefix=prefix, mode=mode, fam=fam, hw=hw, pk=pk, cond=cond, z=z, saved_t=saved_t, masks=masks, x64=x64, keys=keys,
                B=b.to(gpu), gpu=gpu, n=n, cache={})


def bwd(st, d_raw, exact_dw):
    """The poisoned backward of d_raw (n_rays, n_samples, 4) -> {name: gradient} with the latent gradient under "latent"."""
    grads, g_lat = DW.poisoned_bwd(st["fam"], st["hw"], st["pk"], st["cond"], st["z"], tailed(d_raw, st["gpu"]), st["saved_t"],
                                   split=DW.SPLIT_ARG[st["mode"]], exact_dw=exact_dw)
    out = {k: g for k, g in zip(st["keys"], grads) if g is not None}
    out["latent"] = g_lat
    return out


def bwd_cached(st, name, d_raw, exact_dw):
    key = (name, exact_dw)
    if key not in st["cache"]:
        st["cache"][key] = {k: v.clone() for k, v in bwd(st, d_raw, exact_dw).items()}
    return st["cache"][key]


def vs_oracle(st, tag, got, d_raw, exact_dw, rows=None):
    """Per-tensor rel-L2 against the masked fp64 oracle fed the same d_raw, at the family's existing gate (printed next to the worst)."""
    prefix, mode = st["prefix"], st["mode"]
    gate = DW.GATE[prefix]["bf16" if exact_dw else mode]
    idx = slice(None) if rows is None else rows
    ref = DW._oracle(prefix, st["x64"][idx], [mk[idx] for mk in st["masks"]], d_raw.reshape(-1, 4)[idx].double(), st["gpu"])
    grads = [got.get(k) for k in st["keys"]]
    DW._compare(f"grad-scales {prefix} {mode}{'+exact_dw' if exact_dw else ''} N={st['n']} {tag}", prefix, grads, got["latent"], ref, gate,
                per_element=False)


def assert_scaled(tag, got, base, k):
    """got == 2^k base, bit for bit, in every tensor."""
    f = 2.0 ** k
    bad = {}
    for name, g in got.items():
        want = base[name] * f
        if not torch.equal(g, want):
            d = g != want
            bad[name] = (int(d.sum()), float(((g.double() - want.double()).abs() / (want.double().abs() + 1e-300))[d].max()))
    print(f"grad-scales {tag}: bwd(2^{k} d) == 2^{k} bwd(d) bit for bit in {len(got) - len(bad)} of {len(got)} tensors")
    assert not bad, (tag, k, "tensor: (elements that differ, worst relative difference)", bad)


def spread(st):
    e = R.spread_exponents(st["n"]).to(st["gpu"])
    return st["B"] * torch.exp2(e.float()).reshape(st["B"].shape[0], st["B"].shape[1], 1), e.reshape(-1)


@cases
def test_power_of_two_equivariance(hip_lib, gpu, prefix, mode, exact_dw):
    st = _state(prefix, mode, N)
    base = bwd_cached(st, "B", st["B"], exact_dw)
    for k in R.equivariance_k(prefix, mode):
        assert_scaled(f"{prefix} {mode}{'+exact_dw' if exact_dw else ''} N={N}", bwd(st, st["B"] * 2.0 ** k, exact_dw), base, k)


@cases
def test_channel_sparse_gradients(hip_lib, gpu, prefix, mode, exact_dw):
    """d_raw through the colours only and through the density only, each against the oracle; density only: the colour branch's
    gradients are exact zeros (the chain starts at the clamp g = 2^60 with zero operands), the trunk's are not."""
    st = _state(prefix, mode, N)
    rgb_only, sigma_only = st["B"].clone(), st["B"].clone()
    rgb_only[..., 3] = 0.0
    sigma_only[..., :3] = 0.0
    vs_oracle(st, "colours only", bwd(st, rgb_only, exact_dw), rgb_only, exact_dw)
    got = bwd(st, sigma_only, exact_dw)
    vs_oracle(st, "density only", got, sigma_only, exact_dw)
    check_density_only(prefix, got)


@cases
def test_per_point_spread(hip_lib, gpu, prefix, mode, exact_dw):
    """Row i times 2^(-8 (i mod 4)): four magnitudes down to 2^-24 in every 32-point tile.  (a) against the oracle; (b) the 2^-24 rows
    alone (zero rows between them): == 2^-24 x the same rows at scale 1 bit for bit, and against the oracle on their own."""
    st = _state(prefix, mode, N)
    r, e = spread(st)
    vs_oracle(st, "spread", bwd(st, r, exact_dw), r, exact_dw)
    keep = (e == R.SPREAD_K).reshape(r.shape[0], r.shape[1], 1)
    assert int(keep.sum()) == N // 4
    r_small, b_small = r * keep, st["B"] * keep
    got = bwd(st, r_small, exact_dw)
    assert_scaled(f"{prefix} {mode}{'+exact_dw' if exact_dw else ''} N={N} small rows", got, bwd(st, b_small, exact_dw), R.SPREAD_K)
    vs_oracle(st, "spread, 2^-24 rows alone", got, r_small, exact_dw, rows=keep.reshape(-1).nonzero().reshape(-1))


@cases
def test_outlier_row(hip_lib, gpu, prefix, mode, exact_dw):
    st = _state(prefix, mode, N)
    d = st["B"].clone()
    d.reshape(-1, 4)[100] *= 2.0 ** 20
    vs_oracle(st, "row 100 x 2^20", bwd(st, d, exact_dw), d, exact_dw)


@cases
def test_all_zero_gradient(hip_lib, gpu, prefix, mode, exact_dw):
    """d_raw = 0: every gradient element and the latent gradient == 0.0 (poisoned_bwd has checked them finite and the guards intact)."""
    for n in (N, N_SMALL):
        st = _state(prefix, mode, n)
        for name, g in bwd(st, torch.zeros_like(st["B"]), exact_dw).items():
            assert float(g.abs().max()) == 0.0, (n, name)


@cases
def test_partial_wave_tile(hip_lib, gpu, prefix, mode, exact_dw):
    """21 points, 11 padding lanes that read NaN: equivariance at k = -14, +14 and the density-only gradient."""
    st = _state(prefix, mode, N_SMALL)
    base = bwd_cached(st, "B", st["B"], exact_dw)
    vs_oracle(st, "dense", base, st["B"], exact_dw)
    for k in (-14, 14):
        assert_scaled(f"{prefix} {mode}{'+exact_dw' if exact_dw else ''} N={N_SMALL}", bwd(st, st["B"] * 2.0 ** k, exact_dw), base, k)
    sigma_only = st["B"].clone()
    sigma_only[..., :3] = 0.0
    got = bwd(st, sigma_only, exact_dw)
    vs_oracle(st, "density only", got, sigma_only, exact_dw)
    check_density_only(prefix, got)
