"""k_paper_mlp_fwd_live with its 32-point units handed out from a counter (csrc/nf_mlp_live_kernel.h) against the full forward, bit
for bit, with `raw` and `scratch` poisoned: which wave takes which unit now depends on timing, so every case must hold for any order.
Point counts around one unit, capped grids on which a wave takes many units and its ring wraps, live fractions from 0.01 to 1.0,
launches back to back on one stream and together on two, and what the waves of the statistics instantiation report about the
schedule.  GPU only; nothing here has a tolerance."""
import pytest
import torch

from oracle import nerface_oracle as O
from tests import test_gpu_live_fill as F
from tests.test_gpu_live_colour import GUARD, NAN_PAYLOAD, _live_mask, _model, _points

pytestmark = pytest.mark.gpu

# (rays, samples, max_workgroups, fc_alpha bias, seed).  1 / 31 / 32 / 33 points: less than a unit, one short of it, exactly one, one
# more; 737 = 23 units + 1 point on six workgroups; S = 1: every point is the last sample of its ray, so all 300 are live whatever
# the (very negative) density says
SMALL = {"1": (1, 1, 0, 4.5, 51), "31": (1, 31, 0, 4.5, 52), "32": (2, 16, 0, 4.5, 53), "33": (3, 11, 0, 4.5, 54), "737": (67, 11, 0, 4.5, 55),
         "S1": (300, 1, 0, -1.0e6, 56)}
BIG = [(s, b) for s in ("2048_wg1", "2048_wg2") for b in F.BIASES]

_STATE = {}


def _small(gpu, name):
    """(n_rays, s, wgs, inputs, packed image, bias table, the full kernel's raw) of a SMALL case: computed once, never modified."""
    import nerf
    from nerf import ops
    if name not in _STATE:
        m, expr, latent = _model(gpu)
        nerf.set_mlp_precision("f32")
        n_rays, s, wgs, bias, seed = SMALL[name]
        with torch.no_grad():
            m.fc_alpha.bias.fill_(bias)
        ro, rd, z = (t.to(gpu) for t in _points(n_rays, s, seed))
        packed = m.hip_weights().get().clone()
        cond = ops.mlp_condition(m.FAMILY, packed, expr, latent, O.NEAR, O.FAR)
        _STATE[name] = (n_rays, s, wgs, ro, rd, z, packed, cond, ops.mlp_fwd(m.FAMILY, "f32", packed, cond, ro, rd, z))
    return _STATE[name]


def _big(gpu, shape, bias):
    """The same tuple for a case of tests/test_gpu_live_fill.py (its reference, shared)."""
    ro, rd, z, packed, cond, full, _ = F._full(gpu, shape, bias)
    n_rays, s, wgs = F.SHAPES[shape]
    return n_rays, s, wgs, ro, rd, z, packed, cond, full


def _launch(gpu, case, entry="mlp_fwd_live", stream=None):
    """One launch through the C entry point on poisoned buffers -> (buf, scratch, stats or None); nothing is read back here."""
    from nerf import _hip as H
    m, _, _ = _model(gpu)
    n_rays, s, wgs, ro, rd, z, packed, cond, _ = case
    buf = torch.full((4 * n_rays * s + 2 * GUARD,), NAN_PAYLOAD, dtype=torch.int32, device=gpu)
    scratch = torch.full((m.FAMILY.fn("mlp_fwd_live_scratch_floats")(wgs),), NAN_PAYLOAD, dtype=torch.int32, device=gpu)
    args = [H.ptr(packed), H.ptr(cond), H.ptr(ro), H.ptr(rd), 0, H.ptr(z), n_rays, s, buf.data_ptr() + 4 * GUARD, H.ptr(scratch), scratch.numel(), wgs]
    stats = None
    if entry == "mlp_fwd_live_stats":
        waves = scratch.numel() * 4 // (64 * 1104)
        stats = torch.full((waves, 4), -1, dtype=torch.int64, device=gpu)
        args += [stats.data_ptr(), waves]
    m.FAMILY.call(entry, *args, stream if stream is not None else H.stream_ptr(gpu))
    return buf, scratch, stats


def _assert_full(case, buf):
    """sigma bits at every point, rgb bits at every live point, +0.0 at every dead one, nothing written beside raw."""
    n_rays, s, _, _, _, _, _, _, full = case
    n = n_rays * s
    live = _live_mask(full)
    got = buf[GUARD:GUARD + 4 * n].reshape(n_rays, s, 4)
    want = full.view(torch.int32)
    assert torch.equal(got[..., 3], want[..., 3])
    assert torch.equal(got[..., :3][live], want[..., :3][live])
    assert bool((got[..., :3][~live] == 0).all())                             # +0.0, not merely == 0
    assert bool((buf[:GUARD] == NAN_PAYLOAD).all()) and bool((buf[GUARD + 4 * n:] == NAN_PAYLOAD).all())


def _assert_stats(case, stats):
    """Units sum to ceil(n / 32); no wave took more than there are; a wave that took live_w live points ran ceil(live_w / 32) colour
    runs (its last one the flush), so the runs lie between ceil(live / 32) and ceil(live / 32) + waves - 1, over the waves that were
    started; the flush rows are a ring's (at most 31); rows of workgroups that were not started stay zero."""
    n_rays, s, _, _, _, _, _, _, full = case
    n = n_rays * s
    st = stats.cpu()
    started = min((n + 127) // 128, st.shape[0] // 4) * 4
    units, runs, flush, clock = (st[:, i] for i in range(4))
    total, live = (n + 31) // 32, int(_live_mask(full).sum())
    print(f"{n} points, {started} waves: units {units[:started].tolist()}, runs {int(runs.sum())} for {live} live points")
    assert int(units.sum()) == total and int(units.max()) <= total and int(units.min()) >= 0
    assert (live + 31) // 32 <= int(runs.sum()) <= (live + 31) // 32 + started - 1
    assert int(flush.min()) >= 0 and int(flush.max()) <= 31
    assert bool((clock[:started] > 0).all())
    assert bool((st[started:] == 0).all())


@pytest.mark.parametrize("name", list(SMALL))
def test_point_counts_around_a_unit(hip_lib, gpu, name):
    case = _small(gpu, name)
    if name == "S1":
        assert not bool((~(case[8][..., 3] <= 0)).any()) and bool(_live_mask(case[8]).all())     # live only as last samples
    _assert_full(case, _launch(gpu, case)[0])


@pytest.mark.parametrize("shape,bias", BIG, ids=[f"{s}_bias{b}" for s, b in BIG])
def test_many_units_per_wave_over_the_live_fractions(hip_lib, gpu, shape, bias):
    """2048 points = 64 units on four and on eight waves: a wave takes about 16 or 8 units and its ring wraps; live fraction about
    0.01 (bias -1.5) to 1.0 (bias 16.5)."""
    case = _big(gpu, shape, bias)
    _assert_full(case, _launch(gpu, case)[0])


def test_the_biases_span_the_live_fractions(hip_lib, gpu):
    fracs = [float((~(_big(gpu, "2048_wg1", b)[8][..., 3] <= 0)).float().mean()) for b in F.BIASES]
    assert min(fracs) < 0.05 and max(fracs) > 0.95, fracs


def test_nan_densities_are_live(hip_lib, gpu):
    """A NaN in one weight of fc_alpha makes every density NaN and every point live; sigma_raw is compared as bits."""
    from nerf import ops
    m, _, _ = _model(gpu)
    n_rays, s, wgs, ro, rd, z, packed, cond, _ = _small(gpu, "737")
    at = (packed == m.fc_alpha.weight.detach()[0, 17]).nonzero().reshape(-1)
    assert 1 <= at.numel() <= 2
    bad = packed.clone()
    bad[at] = float("nan")
    full = ops.mlp_fwd(m.FAMILY, "f32", bad, cond, ro, rd, z)
    assert bool(torch.isnan(full[..., 3]).all()) and not bool(torch.isnan(full[..., :3]).any())
    case = (n_rays, s, wgs, ro, rd, z, bad, cond, full)
    _assert_full(case, _launch(gpu, case)[0])


def test_three_launches_back_to_back_on_one_stream(hip_lib, gpu):
    """No synchronise between them: each finds its counter at zero, and each gives the full forward's bits."""
    case = _big(gpu, "2048_wg2", 8.0)
    bufs = [_launch(gpu, case)[0] for _ in range(3)]
    for buf in bufs:
        _assert_full(case, buf)
    assert torch.equal(bufs[0], bufs[1]) and torch.equal(bufs[0], bufs[2])


def test_two_streams_in_flight_together(hip_lib, gpu):
    """One workgroup each, 16 units per wave: the two launches overlap on the device, each with its own scratch and its own counter."""
    cases = [_big(gpu, "2048_wg1", 8.0), _big(gpu, "2048_wg1", 2.5)]
    alone = [_launch(gpu, c)[0] for c in cases]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=gpu) for _ in cases]
    together = []
    for c, st in zip(cases, streams):
        with torch.cuda.stream(st):
            together.append(_launch(gpu, c, stream=st.cuda_stream))
    torch.cuda.synchronize()
    for c, a, t in zip(cases, alone, together):
        _assert_full(c, t[0])
        assert torch.equal(a, t[0])


STAT_CASES = [("big", "2048_wg1", 2.5), ("big", "2048_wg2", 8.0), ("big", "2048_wg2", 16.5), ("small", "737", None), ("small", "1", None),
              ("small", "S1", None)]


@pytest.mark.parametrize("kind,name,bias", STAT_CASES, ids=[f"{n}" + (f"_bias{b}" if b is not None else "") for _, n, b in STAT_CASES])
def test_what_the_waves_report(hip_lib, gpu, kind, name, bias):
    """The statistics instantiation: the same bits in raw, and a schedule that adds up."""
    case = _big(gpu, name, bias) if kind == "big" else _small(gpu, name)
    buf, _, stats = _launch(gpu, case, entry="mlp_fwd_live_stats")
    _assert_full(case, buf)
    _assert_stats(case, stats)


def test_ops_binding_of_the_statistics_entry(hip_lib, gpu):
    from nerf import ops
    m, _, _ = _model(gpu)
    case = _small(gpu, "737")
    n_rays, s, _, ro, rd, z, packed, cond, full = case
    raw, stats = ops.mlp_fwd_live_stats(m.FAMILY, packed, cond, ro, rd, z)
    live = _live_mask(full)
    assert torch.equal(raw[..., 3], full[..., 3]) and torch.equal(raw[..., :3][live], full[..., :3][live])
    assert stats.shape[1] == len(ops.LIVE_STAT_COLUMNS)
    _assert_stats(case, stats)
