"""The host model of tests/test_gpu_mlp_fwd_edges.py (tests/mlp_fwd_edges_ref.py) against itself and against the library's size
functions: the point counts sit on the edges they are there for, the never-written table tiles the buffer, the reference restates the
oracle, and -- from the fp64 networks alone -- the gates are ones float32 can meet and the chosen seeds keep the share of ReLU
decisions inside the gate's band under the cap, for every family, arithmetic, layer and case.  No device."""
import pytest
import torch

from oracle import nerface_oracle as O
from tests import mlp_fwd_edges_ref as R


def test_counts_sit_on_the_edges():
    counts = [r * s for r, s in R.COUNTS]
    assert counts == [1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 300, 737]
    samples = {s for _, s in R.COUNTS}
    assert 1 in samples and any(32 % s for s in samples if s < 32) and any(s > 32 for s in samples)
    assert R.SCALE_CASE in R.COUNTS and R.RD_VIEW_CASE in R.COUNTS and R.RD_VIEW_CASE[0] * R.RD_VIEW_CASE[1] == 33
    assert [r * s for r, s in R.BWD_COUNTS] == [1, 17, 31, 33, 129, 300] and set(R.BWD_COUNTS) <= set(R.COUNTS)
    assert all(k in (31, 33, 127, 129) for k in R.PREFIX_KS) and max(R.PREFIX_KS) < R.PREFIX_LAUNCH
    assert R.grid_counts(256) == [32767, 32768, 32769, 65569]
    assert R.hot_rows(1) == [0] and R.hot_rows(17) == [0, 15, 16] and R.hot_rows(33) == [0, 15, 31, 32]
    assert R.hot_rows(129) == [0, 15, 31, 47, 63, 79, 95, 111, 127, 128]
    # every (family, entry) pair of the issue
    assert len(R.PAIRS) == 4 * 7 + 2 and {k for k, *_ in R.PAIRS} == set(R.KINDS)
    assert [(e, a, t) for k, e, a, t in R.PAIRS if k == "smaller"] == [("mlp_fwd", "f32", False), ("mlp_fwd_train", "f32", True)]


def test_size_model_follows_the_library(hip_lib):
    for kind in R.KINDS:
        fn = getattr(hip_lib, R.PREFIX[kind] + "_saved_floats")
        for n in list(range(1, 200)) + [300, 737, 32767, 65569]:
            assert fn(n) == R.saved_floats(kind, n), (kind, n)


def test_never_written_table_is_inside_the_buffer_and_sorted():
    for kind in R.KINDS:
        lay = R.layout(kind)
        secs = sorted(lay["sections"].values())
        assert secs[0][0] == 0 and all(a + w == b for (a, w), (b, _) in zip(secs, secs[1:])) and secs[-1][0] + secs[-1][1] == lay["mask_off"]
        assert [lay["sections"][k][1] for k in lay["acts"]] == [128 if k[0] == "d" else 256 for k in lay["acts"]]
        for arith in R.ARITHMETICS[kind]:
            if arith == "f16x2":
                continue
            for n in [r * s for r, s in R.COUNTS]:
                ranges = R.never_written(kind, arith, n)
                assert all(0 <= lo < hi <= R.saved_floats(kind, n) for lo, hi, _ in ranges), (kind, arith, n)
                assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])), (kind, arith, n)
                assert ranges[-1][1] == R.saved_floats(kind, n)
                if arith != "f32":                      # a count that fills its last 32-point unit has no padding rows
                    assert (len(ranges) == 1) == (n % 32 == 0), (kind, arith, n)


def test_fixtures_have_biases():
    for kind in R.KINDS:
        p = R.model_params(kind)
        assert any(k.endswith(".bias") for k in p)
        for k, v in p.items():
            if k.endswith(".bias"):
                assert float(v.abs().min()) > 0, (kind, k)
    expr, latent = R.conditioning()
    assert expr.shape == (76,) and latent.shape == (32,) and float(expr.abs().max()) > 0 and float(latent.abs().max()) > 0


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_restates_the_oracle(kind):
    """On points that are float32 numbers already the reference is the oracle's own input assembly and network; the hooks return
    what the network computed; rd_view reaches the result through its z-component alone."""
    n_rays, s = R.RD_VIEW_CASE
    ro, rd, z = R.inputs(kind, n_rays, s)
    f = R.forward64(kind, ro, rd, z)
    pts64 = (ro.double()[:, None, :] + rd.double()[:, None, :] * z.double()[:, :, None]).reshape(-1, 3)
    assert float((f["pts32"].double() - pts64).abs().max()) < 2e-7
    p64 = {k: v.double() for k, v in R.model_params(kind).items()}
    expr, latent = (t.double() for t in R.conditioning())
    x87 = O.encode_points(ro.double(), rd.double(), z.double(), O.NEAR, O.FAR)
    assert torch.equal(f["dirs"], x87[:, 63:]) and torch.equal(f["pe"][:, :3], f["pts32"].double())
    assert float((f["pe"] - x87[:, :63]).abs().max()) < 1e-3          # (2^9 times the point's rounding)
    want = R.MLP[kind](p64, torch.cat((f["pe"], f["dirs"]), dim=-1), expr, latent)
    assert torch.equal(f["raw"], want)
    lay = R.layout(kind)
    assert list(f["act"]) == lay["acts"] and list(f["pre"]) == lay["relu"]
    for k, a in f["act"].items():
        assert a.shape == (n_rays * s, lay["sections"][k][1])
        assert torch.equal(a, torch.relu(f["pre"][k])) if k in lay["relu"] else bool((a < 0).any())
    pe = R.pe_in_slot_order(f)
    assert torch.equal(pe[:, 60:63], f["pts32"].double()) and bool((pe[:, 63] == 0).all())
    d = R.dir_slots(f)
    assert torch.equal(d[:, 0], torch.sin(rd[:, 2].double()).repeat_interleave(s)) and bool((d[:, 2::4] == 0).all())
    rv = R.other_view(rd)
    g = R.forward64(kind, ro, rd, z, rd_view=rv)
    assert bool(torch.isfinite(g["raw"]).all()) and torch.equal(g["pe"], f["pe"]) and not torch.equal(g["raw"][:, :3], f["raw"][:, :3])
    assert torch.equal(g["raw"][:, 3], f["raw"][:, 3])                 # the direction does not reach the density


@pytest.mark.parametrize("kind", R.KINDS)
def test_gates_are_ones_float32_can_meet_and_seeds_keep_the_band_small(kind):
    """At the seeds the GPU test uses: torch's own float32 evaluation of the network stays under HALF the f32 gate per channel, and at
    most BAND_CAP of a layer's ReLU inputs lie inside the gate's band around 0 -- per arithmetic, layer and case."""
    refs = {rs: R.forward64(kind, *R.inputs(kind, *rs)) for rs in R.COUNTS}
    big = R.scales(refs[R.SCALE_CASE])
    worst, worst_share = 0.0, {}
    for (n_rays, s), ref in refs.items():
        sc = big if n_rays * s < 128 else R.scales(ref)
        err32 = (R.forward32(kind, *R.inputs(kind, n_rays, s)).double() - ref["raw"]).abs().amax(dim=0)
        ratio = float((err32 / R.raw_gate("f32", sc)).max())
        worst = max(worst, ratio)
        assert ratio < 0.5, (kind, n_rays, s, ratio)
        for arith in R.ARITHMETICS[kind]:
            if arith == "f16x2":
                continue
            for layer, share in R.band_share(arith, ref, sc).items():
                worst_share[arith] = max(worst_share.get(arith, 0.0), share)
                assert share <= R.BAND_CAP, (kind, arith, n_rays, s, layer, share)
    print(f"mlp-fwd-edges host {kind}: float32 torch error / gate at most {worst:.3f}; largest share of a layer's ReLU inputs inside the "
          f"band {', '.join(f'{a} {v:.2e}' for a, v in worst_share.items())} (cap {R.BAND_CAP:g})")
