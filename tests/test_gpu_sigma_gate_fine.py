"""The gated exact-f32 forward (csrc/nf_mlp_gated.hip) at the shapes where its pipelined bound tile, its single last-sample test and
the fine pass's regime can go wrong, against the full forward, through the C entry points with `raw` and `scratch` poisoned.  GPU only;
nothing here has a tolerance.  The contract per point is that of tests/test_gpu_sigma_gate.py: a kept row that is live or last on its
ray is bit-equal in all four channels, a kept row that turns out dead has rgb +0.0 and the bit-equal density, a proven row is
(0, 0, 0, negative finite), and volume_render_fwd of either `raw` is torch.equal in every output.

Shapes: 1, 31, 32, 33, 63, 64, 65 and 737 points at S = 1 (every sample a ray's last: everything is kept); 3 rays x 192 samples (the fine
pass's S, a ray's last sample in the middle of a unit); 2048 points (32 x 64) on one workgroup and on two over the ten fc_alpha biases
of tests/test_gpu_live_fill.py, whose kept share the CPU restatement (tests/sigma_bound_ref.py) puts at 0.03 .. 0.999 with bias 10.5 at
0.87, the fine pass's regime -- checked on the CPU first, then asserted of the kernel's own count.  The schedule cases run at "2048 x 1"
-- 2048 points on ONE workgroup, the reading under which every case can exist: with 2048 rays of one sample each every row is a ray's
last and is kept, so "no run before the flush" has no such shape (that shape is run where it can be, with every pass ending in a run)
-- and at 11 rays x 192 samples."""
import pytest
import torch

from oracle import nerface_oracle as O
from tests import sigma_bound_ref as B
from tests.test_gpu_live_colour import GUARD, NAN_PAYLOAD, _live_mask, _model, _points
from tests.test_gpu_live_fill import BIASES
from tests.test_gpu_sigma_gate import _c, _images, _params

pytestmark = pytest.mark.gpu

# (rays, samples, max_workgroups)
SHAPES = {"1xS1": (1, 1, 0), "31xS1": (31, 1, 0), "32xS1": (32, 1, 0), "33xS1": (33, 1, 0), "63xS1": (63, 1, 0), "64xS1": (64, 1, 0),
          "65xS1": (65, 1, 0), "737xS1": (737, 1, 0), "3x192": (3, 192, 0), "2048_wg1": (32, 64, 1), "2048_wg2": (32, 64, 2),
          "11x192": (11, 192, 0), "2048xS1_wg1": (2048, 1, 1)}
SEEDS = {"1xS1": 61, "31xS1": 62, "32xS1": 63, "33xS1": 64, "63xS1": 65, "64xS1": 66, "65xS1": 67, "737xS1": 68, "3x192": 69, "2048_wg1": 41,
         "2048_wg2": 41, "11x192": 52, "2048xS1_wg1": 70}
SMALL = [(s, b) for s in ("1xS1", "31xS1", "32xS1", "33xS1", "63xS1", "64xS1", "65xS1", "737xS1") for b in (1.0, 8.0)]
FINE = [("3x192", b) for b in (1.0, 8.0, 10.5)]
BIG = [(s, b) for s in ("2048_wg1", "2048_wg2") for b in BIASES]
TWO = ("2048_wg1", "11x192")                                       # the two shapes of the schedule cases
DEAD, LIVE = -1.0e6, 1.0e6                                          # fc_alpha biases: every density on one side
STAT_COLS = 5 + 6                                                  # nf_paper_mlp_fwd_gated_phases: five columns, six sums of clocks

_STATE = {}


def _inputs(gpu, shape):
    if ("in", shape) not in _STATE:
        n_rays, s, _ = SHAPES[shape]
        ro, rd, z = _points(n_rays, s, SEEDS[shape])
        x87 = O.encode_points(ro, rd, z, O.NEAR, O.FAR).reshape(-1, 87)
        _STATE[("in", shape)] = (ro.to(gpu), rd.to(gpu), z.to(gpu), x87)
    return _STATE[("in", shape)]


def _weights(gpu, bias):
    """(packed, bound, cond, params on the CPU) at one fc_alpha bias: built once, never modified."""
    if ("w", bias) not in _STATE:
        _STATE[("w", bias)] = _images(gpu, lambda mm: mm.fc_alpha.bias.fill_(bias))
    return _STATE[("w", bias)]


def _full(gpu, shape, packed, cond, key):
    """The full forward's raw on the shape's points: computed once per (shape, key), shared, never modified."""
    if ("full", shape, key) not in _STATE:
        from nerf import ops
        m, _, _ = _model(gpu)
        ro, rd, z, _ = _inputs(gpu, shape)
        _STATE[("full", shape, key)] = ops.mlp_fwd(m.FAMILY, "f32", packed, cond, ro, rd, z)
    return _STATE[("full", shape, key)]


def _case(gpu, shape, bias):
    packed, bound, cond, p = _weights(gpu, bias)
    return packed, bound, cond, p, _full(gpu, shape, packed, cond, bias)


def _run(gpu, shape, packed, bound, cond, stats=False, stream=None):
    """The C entry point on poisoned buffers -> (raw buffer with its guards, stats or None, the scratch); nothing is synchronised
    here, so whoever launches on a side stream holds on to all three until that stream is through with them."""
    from nerf import _hip as H
    m, _, _ = _model(gpu)
    n_rays, s, wgs = SHAPES[shape]
    ro, rd, z, _ = _inputs(gpu, shape)
    n = n_rays * s
    buf = torch.full((4 * n + 2 * GUARD,), NAN_PAYLOAD, dtype=torch.int32, device=gpu)
    scratch = torch.full((m.FAMILY.fn("mlp_fwd_live_scratch_floats")(wgs),), NAN_PAYLOAD, dtype=torch.int32, device=gpu)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(gpu))                      # (the buffers were filled on the current stream)
    sp = H.stream_ptr(gpu) if stream is None else stream.cuda_stream
    args = (H.ptr(packed), H.ptr(bound), H.ptr(cond), H.ptr(ro), H.ptr(rd), 0, H.ptr(z), n_rays, s, buf.data_ptr() + 4 * GUARD, H.ptr(scratch),
            scratch.numel(), wgs)
    st = None
    if stats:
        rows = scratch.numel() * 4 // (64 * (1024 + 64 + 16))
        st = torch.full((rows + 1, STAT_COLS), -1, dtype=torch.int64, device=gpu)   # (a guard row behind the last)
        m.FAMILY.call("mlp_fwd_gated_phases", *args, st.data_ptr(), rows, sp)
    else:
        m.FAMILY.call("mlp_fwd_gated", *args, sp)
    return buf, st, scratch


def _check(gpu, shape, buf, full):
    """The per-point contract and the integrator's outputs; returns the mask of rows whose density is not the full forward's."""
    from nerf import ops
    n_rays, s, _ = SHAPES[shape]
    n = n_rays * s
    _, rd, z, _ = _inputs(gpu, shape)
    assert bool((buf[:GUARD] == NAN_PAYLOAD).all()) and bool((buf[GUARD + 4 * n:] == NAN_PAYLOAD).all()), shape
    got = buf[GUARD:GUARD + 4 * n].reshape(n_rays, s, 4)
    want = full.view(torch.int32)
    live = _live_mask(full)
    assert torch.equal(got[live], want[live]), shape                            # kept, live or last: all four channels
    assert bool((got[..., :3][~live] == 0).all()), shape                        # +0.0, not merely == 0
    same = got[..., 3] == want[..., 3]
    sig = got[..., 3].view(torch.float32)
    assert bool((same | ((sig < 0) & torch.isfinite(sig)))[~live].all()), shape  # kept and dead: the same density; proven: negative, finite
    raw = got.view(torch.float32).contiguous()
    for a, b in zip(ops.volume_render_fwd(raw, z, rd), ops.volume_render_fwd(full, z, rd)):
        # (the NaN case: torch.equal is false on NaN outputs even of the same `raw`; there the bits must be the same)
        assert torch.equal(a, b) or (bool(torch.isnan(b).any()) and torch.equal(a.view(torch.int32), b.view(torch.int32))), shape
    return ~same


def _stats(shape, st):
    """The statistics rows of a launch, checked: units sum to ceil(n / 32); proven + kept is every in-range row (a run before the flush
    finishes 32 kept rows, the flush its own); the clocks are sums of non-negative spans; nothing is written behind the last row.
    Returns (units, runs, flush rows, proven rows, kept share)."""
    n_rays, s, _ = SHAPES[shape]
    n = n_rays * s
    st = st.cpu()
    assert bool((st[-1] == -1).all()), shape
    st = st[:-1]
    units, runs, flush, proven = (st[:, k] for k in (0, 1, 2, 4))
    assert int(units.sum()) == (n + 31) // 32 and int(units.min()) >= 0, shape
    assert 0 <= int(flush.min()) and int(flush.max()) <= 31 and int(proven.min()) >= 0, shape
    kept = 32 * (int(runs.sum()) - int((flush > 0).sum())) + int(flush.sum())
    assert int(proven.sum()) + kept == n, (shape, int(proven.sum()), kept)
    clocks = st[:, 5:]
    assert bool((clocks >= 0).all()) and bool((clocks[units > 0, 0] > 0).all()) and bool((clocks[units == 0, :3] == 0).all()), shape
    return int(units.sum()), int(runs.sum()), flush, int(proven.sum()), kept / n


def _cpu_kept_share(p, shape):
    _, s, _ = SHAPES[shape]
    h, _ = B.trunk(p, _STATE[("in", shape)][3], _c()["expr"], _c()["latent"])
    proven = B.gate(h.numpy(), *B.bound_vectors(p))[3]
    proven[s - 1::s] = False                                                   # a ray's last sample is never proven
    return 1.0 - float(proven.mean())


@pytest.mark.parametrize("shape,bias", SMALL + FINE, ids=[f"{s}_bias{b}" for s, b in SMALL + FINE])
def test_point_counts_around_a_unit_and_the_fine_sample_count(hip_lib, gpu, shape, bias):
    packed, bound, cond, _, full = _case(gpu, shape, bias)
    buf, _, _ = _run(gpu, shape, packed, bound, cond)
    changed = _check(gpu, shape, buf, full)
    buf2, st, _ = _run(gpu, shape, packed, bound, cond, stats=True)
    assert torch.equal(buf2, buf), shape                                        # the statistics instantiation computes the same
    _, _, _, n_proven, share = _stats(shape, st)
    n_rays, s, _ = SHAPES[shape]
    if s == 1:                                                                  # every sample is its ray's last: nothing is proven
        assert n_proven == 0 and not bool(changed.any()), shape
    else:
        assert not bool(changed[:, -1].any()) and int(changed.sum()) <= n_proven <= int((~_live_mask(full)).sum()), shape
    print(f"{shape} bias {bias}: kept share {share:.3f}, proven {n_proven} of {n_rays * s}")


def test_the_ten_biases_span_the_kept_share_on_the_cpu():
    """tests/sigma_bound_ref.py on the 2048 points: from under 0.05 to over 0.99, with bias 10.5 between 0.75 and 0.9."""
    n_rays, s, _ = SHAPES["2048_wg1"]
    ro, rd, z = _points(n_rays, s, SEEDS["2048_wg1"])
    x87 = O.encode_points(ro, rd, z, O.NEAR, O.FAR).reshape(-1, 87)
    c = _c()
    p = {k: v.clone() for k, v in c["p_fine"].items()}                          # (the weights of tests/test_gpu_live_colour.py's model)
    shares = {}
    for b in BIASES:
        p["fc_alpha.bias"] = torch.full_like(p["fc_alpha.bias"], b)
        h, _ = B.trunk(p, x87, c["expr"], c["latent"])
        proven = B.gate(h.numpy(), *B.bound_vectors(p))[3]
        proven[s - 1::s] = False
        shares[b] = 1.0 - float(proven.mean())
    print("CPU kept shares:", {b: round(v, 3) for b, v in shares.items()})
    assert min(shares.values()) < 0.05 and max(shares.values()) > 0.99 and 0.75 < shares[10.5] < 0.9, shares


@pytest.mark.parametrize("shape", ["2048_wg1", "2048_wg2"])
def test_kept_share_from_zero_to_one(hip_lib, gpu, shape):
    """The ten biases on 2048 points: the contract at each, and the kernel's own kept share spans 0 .. 1 with the fine pass's regime
    (0.75 .. 0.9) among them."""
    shares = {}
    for bias in BIASES:
        packed, bound, cond, p, full = _case(gpu, shape, bias)
        buf, _, _ = _run(gpu, shape, packed, bound, cond)
        changed = _check(gpu, shape, buf, full)
        buf2, st, _ = _run(gpu, shape, packed, bound, cond, stats=True)
        assert torch.equal(buf2, buf), (shape, bias)
        _, _, _, n_proven, shares[bias] = _stats(shape, st)
        live = _live_mask(full)
        assert not bool((changed & live).any()) and int(changed.sum()) <= n_proven <= int((~live).sum()), (shape, bias)
        cpu = _cpu_kept_share(p, shape)
        print(f"{shape} bias {bias}: live {float(live.float().mean()):.3f}, kept share {shares[bias]:.3f} (CPU restatement {cpu:.3f})")
    assert min(shares.values()) < 0.05 and max(shares.values()) > 0.99, shares
    assert any(0.75 < v < 0.9 for v in shares.values()), shares


@pytest.mark.parametrize("shape", TWO)
def test_no_pass_ends_in_a_run_before_the_flush(hip_lib, gpu, shape):
    """Every density far below zero: only a ray's last sample is kept, under one row per pass, and a wave's ring never fills -- its
    only gathered run is the final flush."""
    packed, bound, cond, _, full = _case(gpu, shape, DEAD)
    buf, st, _ = _run(gpu, shape, packed, bound, cond, stats=True)
    _check(gpu, shape, buf, full)
    _, runs, flush, n_proven, share = _stats(shape, st)
    n_rays, s, _ = SHAPES[shape]
    assert n_proven == n_rays * (s - 1) and share < 1.0 / 32, (shape, n_proven, share)
    assert runs == int((flush > 0).sum()) and int(flush.sum()) == n_rays, (shape, runs, flush.tolist())


@pytest.mark.parametrize("shape", TWO + ("2048xS1_wg1",))
def test_every_pass_ends_in_a_run(hip_lib, gpu, shape):
    """Every density far above zero (or, at S = 1, every sample a ray's last): all 32 rows of every pass are kept, every pass runs
    fc_feat and the colour layers on its own rows, and nothing is left for a flush."""
    packed, bound, cond, _, full = _case(gpu, shape, LIVE if SHAPES[shape][1] > 1 else 8.0)
    buf, st, _ = _run(gpu, shape, packed, bound, cond, stats=True)
    changed = _check(gpu, shape, buf, full)
    units, runs, flush, n_proven, share = _stats(shape, st)
    assert n_proven == 0 and share == 1.0 and not bool(changed.any()), shape
    assert runs == units and int(flush.sum()) == 0, (shape, runs, units)


@pytest.mark.parametrize("shape", TWO)
def test_three_launches_without_a_synchronise(hip_lib, gpu, shape):
    packed, bound, cond, _, full = _case(gpu, shape, 10.5)
    outs = [_run(gpu, shape, packed, bound, cond) for _ in range(3)]
    torch.cuda.synchronize()
    for buf, _, _ in outs:
        _check(gpu, shape, buf, full)
        assert torch.equal(buf, outs[0][0])


@pytest.mark.parametrize("shape", TWO)
def test_two_streams_in_flight_together(hip_lib, gpu, shape):
    a = _case(gpu, shape, 4.5)
    b = _case(gpu, shape, 10.5)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
    outs = []
    for _ in range(2):
        outs.append((a[4], _run(gpu, shape, *a[:3], stream=s1)))
        outs.append((b[4], _run(gpu, shape, *b[:3], stream=s2)))
    s1.synchronize()
    s2.synchronize()
    for full, (buf, _, _) in outs:
        _check(gpu, shape, buf, full)


@pytest.mark.parametrize("shape", TWO)
def test_cancelling_net_is_never_proven_wrongly(hip_lib, gpu, shape):
    """fc_alpha x 1e-3 with the bias at minus the median density: densities crowd around zero, half of them on either side."""
    m, _, _ = _model(gpu)
    _, _, _, x87 = _inputs(gpu, shape)
    q = B.cancelling(_params(gpu), x87, _c()["expr"], _c()["latent"])

    def setup(mm):
        mm.fc_alpha.weight.copy_(q["fc_alpha.weight"])
        mm.fc_alpha.bias.copy_(q["fc_alpha.bias"])
    keep = (m.fc_alpha.weight.detach().clone(), m.fc_alpha.bias.detach().clone())
    try:
        packed, bound, cond, _ = _images(gpu, setup)
    finally:
        with torch.no_grad():
            m.fc_alpha.weight.copy_(keep[0])
            m.fc_alpha.bias.copy_(keep[1])
    full = _full(gpu, shape, packed, cond, "cancelling")
    frac = float((~(full[..., 3] <= 0)).float().mean())
    assert 0.3 < frac < 0.7, frac
    buf, st, _ = _run(gpu, shape, packed, bound, cond, stats=True)
    _check(gpu, shape, buf, full)
    _, _, _, n_proven, share = _stats(shape, st)
    print(f"cancelling net, {shape}: live {frac:.3f}, kept share {share:.3f}, proven {n_proven}")


@pytest.mark.parametrize("shape", TWO)
def test_nan_in_fc_alpha_proves_nothing(hip_lib, gpu, shape):
    """A NaN in one weight of fc_alpha (on a copy of the packed image, the bound image built from that copy): no comparison holds, every
    row is gathered, every pass ends in a run and every density is the full forward's NaN, bit for bit."""
    from nerf import ops
    m, _, _ = _model(gpu)
    packed, _, cond, _ = _weights(gpu, 8.0)
    with torch.no_grad():
        m.fc_alpha.bias.fill_(8.0)
    at = (packed == m.fc_alpha.weight.detach()[0, 17]).nonzero().reshape(-1)
    assert 1 <= at.numel() <= 2
    bad = packed.clone()
    bad[at] = float("nan")
    bound = ops.sigma_bound(m.FAMILY, bad)
    full = _full(gpu, shape, bad, cond, "nan")
    assert bool(torch.isnan(full[..., 3]).all())
    buf, st, _ = _run(gpu, shape, bad, bound, cond, stats=True)
    changed = _check(gpu, shape, buf, full)
    _, _, _, n_proven, share = _stats(shape, st)
    assert not bool(changed.any()) and n_proven == 0 and share == 1.0, shape


def test_validation_render_is_the_same_with_both_passes_gated_and_with_none(hip_lib, gpu):
    """run_one_iter_of_nerf(mode="validation") under no_grad, 128 rays, 16 + 32 samples: all seven outputs torch.equal between
    ops.set_sigma_gate(True) -- the coarse and the fine pass both take the gated kernel -- and (False)."""
    import nerf
    from nerf import ops
    from oracle import cases as C
    from tests import util as U
    c = _c()
    mc, mf = U.make_model(nerf, c["p_coarse"], gpu), U.make_model(nerf, c["p_fine"], gpu)
    ro, rd, _, _, _ = C.ray_subset(512, 512, 3, 128, 23)
    ro, rd = ro.reshape(8, 16, 3).to(gpu), rd.reshape(8, 16, 3).to(gpu)
    ex, ed = U.encoders(nerf)
    opt = U.make_options(nerf, 16, 32, True, 0.0)
    nerf.set_mlp_precision("f32")

    def render():
        torch.manual_seed(1234)
        with torch.no_grad():
            return nerf.run_one_iter_of_nerf(8, 16, None, mc, mf, ro, rd, opt, mode="validation", encode_position_fn=ex, encode_direction_fn=ed,
                                             expressions=c["expr"].to(gpu), background_prior=None, latent_code=c["latent"].to(gpu))
    try:
        ops.set_sigma_gate(True)
        n0 = ops.sigma_gate_launches()
        on = render()
        assert ops.sigma_gate_launches() == n0 + 2
        ops.set_sigma_gate(False)
        off = render()
        assert ops.sigma_gate_launches() == n0 + 2
    finally:
        ops.set_sigma_gate(None)
    assert len(on) == len(off) == 7
    for k in range(7):
        assert torch.equal(on[k], off[k]), k
