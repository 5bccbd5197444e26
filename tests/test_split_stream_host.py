"""CPU: the host model of the split-precision weight streams (tests/split_stream_ref.py) against the sources and the library's host
exports, before tests/test_gpu_split_streams.py and tests/test_gpu_grad_scales.py hold the device kernels to it."""
import os
import re

import numpy as np
import torch

from oracle import nerface_oracle as O
from tests import split_stream_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4d-facial-avatars_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_restated_constants_are_the_sources_own():
    brace = lambda v: "{" + ", ".join(str(x) for x in v) + "}"
    for name, s in R.STREAMS.items():
        text = _src(s["src"])
        assert f"constexpr int NL = {s['NL']};" in text, name
        assert f"constexpr int KS[NL] = {brace(s['KS'])};" in text, name
        assert f"constexpr int NO[NL] = {brace(s['NO'])};" in text, name
        assert len(s["KS"]) == len(s["NO"]) == s["NL"]
    pack = _src("nf_pack.h")
    assert f"#define NF_F16_TAIL_BYTES {R.F16_TAIL_BYTES}\n" in pack
    assert re.search(rf"#define NF_F16_FLAG_WORD {R.F16_FLAG_WORD}\s", pack)
    assert 3 * max(s["NL"] for s in R.STREAMS.values()) <= R.F16_FLAG_WORD < R.F16_TAIL_BYTES // 4         # the three arrays end before the flag
    assert f"int e = {R.SCALE_TOP} - k;" in pack
    assert f"e = e < {R.SCALE_E_MIN} ? {R.SCALE_E_MIN} : (e > {R.SCALE_E_MAX} ? {R.SCALE_E_MAX} : e);" in pack
    assert (f"hipLaunchKernelGGL((k_stream_absmax<N, TAG, NL>), dim3({R.ABSMAX_GRID}), dim3({R.ABSMAX_BLOCK}), 0, nf_s(stream), ptrs, table, "
            "n_entries, lp,") in pack
    assert "const int span = (n_entries + gridDim.x - 1) / gridDim.x;" in pack
    assert "const int e0 = blockIdx.x * span, e1 = e0 + span < n_entries ? e0 + span : n_entries;" in pack
    assert (f"for (; e + {R.ABSMAX_UNROLL - 1} * (int)blockDim.x < e1; e += {R.ABSMAX_UNROLL} * blockDim.x)") in pack
    assert "hipMemsetAsync(tail, 0, NF_F16_TAIL_BYTES, nf_s(stream))" in pack                               # pack clears flag and maxima
    assert "constexpr int pair_off(int l) { int o = 0; for (int i = 0; i < l; ++i) o += KS[i] * NO[i]; return o; }" in _src("nf_mlp_split_table.h")
    # act_scale: 2^NFB_ACT_SHIFT forward, 1 backward
    for f in ("nf_mlp_f16.hip", "nf_mlp_lcode_f16.hip"):
        assert "#define NFB_ACT_SHIFT 4\n" in _src(f) and "(float)(1 << NFB_ACT_SHIFT), stream);" in _src(f)
    for f in ("nf_mlp_bf16_bwd.hip", "nf_mlp_lcode_bf16_bwd.hip"):
        assert "nfb::layer_pairs(), 1.0f, stream);" in _src(f)
    # the chain's per-point scale: biased exponent e, se = 267 - e clamped to [67, 187] -> unclamped for 80 <= e <= 200
    mach = _src("nf_mlp_bf16_machinery.inc")
    assert "int se = 267 - e;" in mach and "se = se < 67 ? 67 : (se > 187 ? 187 : se);" in mach
    assert R.CHAIN_UNCLAMPED[0] == 2.0 ** (267 - 187 - 127) and R.CHAIN_UNCLAMPED[1] <= 2.0 ** (267 - 67 + 1 - 127)


def test_stream_sizes_follow_the_layer_tables(hip_lib):
    for name, s in R.STREAMS.items():
        assert getattr(hip_lib, s["table"])(None, 0) == R.n_pairs(name) * 512 == R.n_entries(name), name
        for kind in s["kinds"]:
            assert getattr(hip_lib, f"{s['prefix']}_{R.SIZE_FN[kind]}")() == R.image_bytes(name, kind), (name, kind)
        if name.endswith("fwd"):
            assert getattr(hip_lib, f"{s['prefix']}_f16_flag_offset")() == R.flag_offset(name), name
    assert R.pair_offsets("lcode_fwd") == [0, 32, 160, 288, 416, 432, 560, 632, 640]       # profiles/split_families_shared.md
    assert [R.n_pairs(n) for n in ("paper_fwd", "paper_bwd", "lcode_fwd", "lcode_bwd")] == [994, 920, 640, 600]


def test_every_layer_holds_its_own_tensor_only(hip_lib):
    """The pair offsets cut the table where the tensor ids change: every layer has live entries, they name weight matrices only (one,
    or two where a layer carries a second head: the paper forward's layers_dir.0 + fc_alpha), and no tensor appears in two layers."""
    for name in R.STREAMS:
        tab, off = R.stream_table(hip_lib, name), R.pair_offsets(name)
        ids, _ = R.split_codes(tab)
        owner, seen = [], set()
        for l in range(R.STREAMS[name]["NL"]):
            lo, hi = R.layer_entries(off, l)
            here = set(np.unique(ids[lo:hi]).tolist()) - {0xFF}
            assert 1 <= len(here) <= 2 and all(t % 2 == 0 for t in here), (name, l, sorted(here))    # ABI order: weight 2 i, bias 2 i + 1
            assert not (here & seen), (name, l, sorted(here & seen))
            seen |= here
            owner.append(sorted(here))
        assert sum(len(o) for o in owner) == len(seen)
        print(f"{name}: tensors per layer {owner}")


def test_position_classes_of_the_absmax_kernel(hip_lib):
    """Which position classes of k_stream_absmax each layer of each stream has (what the planted maxima of
    tests/test_gpu_split_streams.py cover); every stream as a whole has every class."""
    for name in R.STREAMS:
        tab, off = R.stream_table(hip_lib, name), R.pair_offsets(name)
        n, span = len(tab), R.absmax_span(len(tab))
        seen = set()
        for l in range(R.STREAMS[name]["NL"]):
            pos = R.absmax_positions(tab, off, l)
            lo, hi = R.layer_entries(off, l)
            for cls, e in pos.items():
                if e is None:
                    continue
                assert lo <= e < hi and (tab[e] >> 24) != 0xFF, (name, l, cls, e)
                seen.add(cls)
            b = (lo // span + 1) * span
            assert pos["before_first_boundary"] is None or pos["before_first_boundary"] < b
            assert pos["after_first_boundary"] is None or pos["after_first_boundary"] >= b
            if pos["remainder"] is not None:
                assert R.in_remainder_loop(pos["remainder"], n)
            if pos["straddle"] is not None:
                assert pos["straddle"] // span == (lo - 1) // span                 # same workgroup as the previous layer's last entry
            print(f"{name} (span {span}) layer {l:2d} [{lo}, {hi}): " + " ".join(f"{c}={e}" for c, e in pos.items() if e is not None)
                  + ("  missing: " + ",".join(c for c, e in pos.items() if e is None) if None in pos.values() else ""))
        assert seen == set(R.CLASSES), (name, sorted(set(R.CLASSES) - seen))


def test_remainder_loop_model_against_a_walk_of_the_kernel():
    """in_remainder_loop against a literal walk of the kernel's two loops for one workgroup, at spans around multiples of 256 and 1024."""
    for span in (1, 255, 256, 257, 1023, 1024, 1025, 1988, 2500):
        n = span * R.ABSMAX_GRID - 3                                              # the last workgroup is three entries short
        for e0 in (0, (R.ABSMAX_GRID - 1) * span):
            e1 = min(e0 + span, n)
            where = {}
            for t in range(R.ABSMAX_BLOCK):
                e = e0 + t
                while e + 3 * R.ABSMAX_BLOCK < e1:
                    for q in range(4):
                        where[e + q * R.ABSMAX_BLOCK] = False
                    e += 4 * R.ABSMAX_BLOCK
                while e < e1:
                    where[e] = True
                    e += R.ABSMAX_BLOCK
            assert sorted(where) == list(range(e0, e1)), span                     # every entry of the span read exactly once
            assert R.absmax_span(n) == span
            for e, rem in where.items():
                assert R.in_remainder_loop(e, n) == rem, (span, e)


def test_reference_split_keeps_the_precision_the_pack_comment_states():
    """10^5 log-uniform weights over 2^-30 .. 2^0 of the layer's largest: the reference split reconstructs w s within 2^-22 |w s| where
    |w s| >= 2^-3 and within 2^-25 absolute (scaled units) below.  For a largest weight at the top of the scale window (amax s just
    under 2^14) that is `every weight down to 2^-17 of the layer's largest`; at the bottom of the window (amax s = 2^13) a weight at
    2^-17 of the largest sits at 2^-4, where lo's subnormal quantum 2^-24 leaves up to 2^-25 = 2^-21 relative: the 2^-17 claim
    holds for the window's top, 2^-16 for every largest weight (csrc/nf_pack.h says so)."""
    g = torch.Generator().manual_seed(4)
    u = torch.rand(100000, generator=g, dtype=torch.float64) * 30.0
    sign = torch.where(torch.rand(100000, generator=g) < 0.5, -1.0, 1.0).double()
    for amax in (float(np.float32(1.0) - np.float32(2.0 ** -24)), 0.7, 0.5):
        s = R.layer_scale(amax)
        assert 2.0 ** 13 <= amax * s < 2.0 ** 14
        w = (sign * amax * torch.exp2(-u)).float()
        ws = w * s
        hi, lo = R.split_f16(ws)
        err = (hi.double() + lo.double() - ws.double()).abs()
        big = ws.abs() >= 2.0 ** -3
        assert bool((w.abs() >= 2.0 ** -16 * amax)[~big].logical_not().all())    # every weight >= 2^-16 amax is `big`
        assert bool((err[big] <= 2.0 ** -22 * ws[big].abs().double()).all()), amax
        assert bool((err[~big] <= 2.0 ** -25).all()), amax
        claim = w.abs().double() >= 2.0 ** -17 * amax
        bad = int((err[claim] > 2.0 ** -22 * ws[claim].abs().double()).sum())
        print(f"amax s = {amax * s:.6g}: worst relative error where |w s| >= 2^-3: 2^{float(torch.log2((err[big] / ws[big].abs().double()).max())):.2f}; "
              f"worst absolute below: 2^{float(torch.log2(err[~big].max())):.2f}; {bad} of {int(claim.sum())} weights >= 2^-17 amax miss 2^-22 relative")
        if amax * s >= 2.0 ** 14 * (1 - 2.0 ** -23):
            assert bad == 0                                                        # the window's top: the 2^-17 claim as stated
        normal = lo.float().abs() >= 2.0 ** -14
        print(f"    lo: {int(normal.sum())} normal, {int(((lo.float() != 0) & ~normal).sum())} subnormal, {int((lo.float() == 0).sum())} zero")


def test_gradient_maxima_stay_inside_the_unclamped_range():
    """The fp64 oracle backward of the paper and second-family networks on the 259-point input of tests/test_gpu_grad_scales.py:
    every point's largest |dZ| per layer (and its rgb gradient), times 2^k, lies inside [2^-47, 2^73) -- where nfb_pow2_scale does
    not clamp -- for every k that module scales the upstream gradient by bit for bit in the fp16 arithmetic.  The paper model's smallest
    maximum is 2^-10.9 (unclamped for -36.1 <= k < 65.5), so k = -40 is not in its set (split_stream_ref.F16_EQUIVARIANCE_K: -32
    instead); the second family's is 2^-6.3 (-40.7 <= k < 67.4) and keeps -40."""
    ro, rd, z, b = R.grad_inputs(259)
    x64 = O.encode_points(ro.double(), rd.double(), z.double(), O.NEAR, O.FAR)
    bad = []
    for prefix in ("nf_paper", "nf_lcode"):
        p, expr, latent, mlp = R.grad_family_params(prefix)
        maxima = R.per_point_dz_maxima(mlp, p, x64, expr, latent, b.reshape(-1, 4).double())
        lo = min(float(m.min()) for m in maxima)
        hi = max(float(m.max()) for m in maxima)
        print(f"{prefix}: per-point per-layer max |dZ| in [{lo:.3e}, {hi:.3e}] = [2^{np.log2(lo):.1f}, 2^{np.log2(hi):.1f}] over {len(maxima)} sections")
        assert lo > 0.0
        print(f"    unclamped for {np.log2(R.CHAIN_UNCLAMPED[0] / lo):.1f} <= k < {np.log2(R.CHAIN_UNCLAMPED[1] / hi):.1f}")
        bad += [(prefix, k) for k in R.equivariance_k(prefix, "f16") + (R.SPREAD_K,)
                if not (R.CHAIN_UNCLAMPED[0] <= lo * 2.0 ** k and hi * 2.0 ** k < R.CHAIN_UNCLAMPED[1])]
    assert not bad, bad
