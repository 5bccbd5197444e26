"""k_paper_mlp_fwd_live with its holes filled in place (csrc/nf_mlp_live.hip) against the full forward, bit for bit, on liveness
patterns that drive every branch of a pass: fill / append / flush, rows from the prefetch registers and rows loaded behind the ballot,
ring reuse over many passes, block rotation, out-of-range rows as holes, NaN densities.  GPU only; nothing here has a tolerance.

Liveness is steered by fc_alpha.bias on the model of tests/test_gpu_live_colour.py (seed 1): on these points the CPU oracle puts the
raw density at bias 0 between -17.1 and +5.6 (quantiles 3 % / 50 % / 97 %: -13.4 / -6.9 / +0.2), so the biases below give live
fractions from 0.01 to 0.998.  Every case feeds the FULL kernel's live mask to the host model of the schedule
(tests/live_schedule_ref.py); the cases together must hit every branch named in its REQUIRED.  The biases were picked with the CPU
oracle and that model so that each branch is hit by at least three cases: a density that rounds to the other side of zero on the
device moves a case, not the coverage."""
import numpy as np
import pytest
import torch

from oracle import nerface_oracle as O
from tests import live_schedule_ref as M
from tests.test_gpu_live_colour import GUARD, NAN_PAYLOAD, _live_mask, _model, _points

pytestmark = pytest.mark.gpu

# (rays, samples, max_workgroups): 2048 points on one and on two workgroups -- 16 and 8 passes per wave, a pass is half a ray, so a
# pass can be all dead; 737 points = 23 x 32 + 1 on six workgroups: out-of-range rows are holes; one point; 15 points (NaN case)
SHAPES = {"2048_wg1": (32, 64, 1), "2048_wg2": (32, 64, 2), "737": (67, 11, 0), "1": (1, 1, 0), "15": (3, 5, 0)}
BIASES = [-1.5, 1.0, 2.5, 4.5, 6.0, 8.0, 10.5, 11.5, 13.5, 16.5]
CASES = ([(s, b) for s in ("2048_wg1", "2048_wg2") for b in BIASES] + [("737", b) for b in (1.0, 8.0, 12.0)] + [("1", -1.5), ("1", 16.5)])
SEEDS = {"2048_wg1": 41, "2048_wg2": 41, "737": 43, "1": 44, "15": 45}

_STATE = {}


def _full(gpu, shape, bias):
    """(inputs, packed image, bias table, the full kernel's raw, the schedule's passes) of a case: computed once, never modified."""
    import nerf
    from nerf import ops
    key = (shape, bias)
    if key not in _STATE:
        m, expr, latent = _model(gpu)
        nerf.set_mlp_precision("f32")
        with torch.no_grad():
            m.fc_alpha.bias.fill_(bias)
        n_rays, s, wgs = SHAPES[shape]
        ro, rd, z = (t.to(gpu) for t in _points(n_rays, s, SEEDS[shape]))
        packed = m.hip_weights().get().clone()
        cond = ops.mlp_condition(m.FAMILY, packed, expr, latent, O.NEAR, O.FAR)
        full = ops.mlp_fwd(m.FAMILY, "f32", packed, cond, ro, rd, z)
        sig_pos = (~(full[..., 3] <= 0)).reshape(-1).cpu().numpy()
        cus = torch.cuda.get_device_properties(gpu).multi_processor_count
        passes, coloured = M.replay(sig_pos, n_rays * s, s, wgs if wgs else cus)
        assert np.array_equal(coloured, _live_mask(full).reshape(-1).cpu().numpy().astype(np.int64))
        _STATE[key] = (ro, rd, z, packed, cond, full, passes)
    return _STATE[key]


def _check(gpu, m, shape, ro, rd, z, packed, cond, full):
    """The live kernel through the C entry point on a buffer with poisoned guards: sigma bits at every point, rgb bits at every live
    point, +0.0 at every dead one, nothing written beside raw."""
    from nerf import _hip as H
    n_rays, s, wgs = SHAPES[shape]
    n = n_rays * s
    live = _live_mask(full)
    buf = torch.full((4 * n + 2 * GUARD,), NAN_PAYLOAD, dtype=torch.int32, device=gpu)
    scratch = torch.full((m.FAMILY.fn("mlp_fwd_live_scratch_floats")(wgs),), NAN_PAYLOAD, dtype=torch.int32, device=gpu)
    m.FAMILY.call("mlp_fwd_live", H.ptr(packed), H.ptr(cond), H.ptr(ro), H.ptr(rd), 0, H.ptr(z), n_rays, s, buf.data_ptr() + 4 * GUARD,
                  H.ptr(scratch), scratch.numel(), wgs, H.stream_ptr(gpu))
    got = buf[GUARD:GUARD + 4 * n].reshape(n_rays, s, 4)
    want = full.view(torch.int32)
    assert torch.equal(got[..., 3], want[..., 3]), shape
    assert torch.equal(got[..., :3][live], want[..., :3][live]), shape
    assert bool((got[..., :3][~live] == 0).all()), shape                       # +0.0, not merely == 0
    assert bool((buf[:GUARD] == NAN_PAYLOAD).all()) and bool((buf[GUARD + 4 * n:] == NAN_PAYLOAD).all()), shape


@pytest.mark.parametrize("shape,bias", CASES, ids=[f"{s}_bias{b}" for s, b in CASES])
def test_filled_in_place_is_the_full_forward(hip_lib, gpu, shape, bias):
    m, _, _ = _model(gpu)
    ro, rd, z, packed, cond, full, passes = _full(gpu, shape, bias)
    frac = float((~(full[..., 3] <= 0)).float().mean())
    print(f"{shape} bias {bias}: live fraction {frac:.3f}, branches {sorted(M.branches(passes))}")
    _check(gpu, m, shape, ro, rd, z, packed, cond, full)


def test_the_cases_cover_every_branch_of_the_schedule(hip_lib, gpu):
    """A condition on the cases, not a measurement: fill with R == D, append to R + L == 31, an all-live pass with R > 0, a pass with
    L == 0 and R > 0, more holes than the prefetch depth, a final flush of one row and of at least 30."""
    hit, fracs = set(), []
    for shape, bias in CASES:
        full, passes = _full(gpu, shape, bias)[5:]
        hit |= M.branches(passes)
        if full.numel() > 4:
            fracs.append(float((~(full[..., 3] <= 0)).float().mean()))
    assert M.REQUIRED <= hit, M.REQUIRED - hit
    assert min(fracs) < 0.05 and max(fracs) > 0.95, (min(fracs), max(fracs))


@pytest.mark.parametrize("shape", ["737", "15"])
def test_nan_densities_are_live_and_cross_the_ring_intact(hip_lib, gpu, shape):
    """A NaN in one weight of fc_alpha (on a copy of the packed image) makes every density NaN: every point is live.  737 points: full
    passes touch no ring, the last block's lone row is appended and flushed; 15 points: all are appended, and the flush takes eight from
    the prefetch registers and seven behind them.  sigma_raw is compared as bits (the NaN's payload), and rgb, which fc_alpha does
    not reach, stays the full forward's."""
    from nerf import ops
    m, _, _ = _model(gpu)
    ro, rd, z, packed, cond, _, _ = _full(gpu, shape, 4.5)
    w = m.fc_alpha.weight.detach()[0, 17]
    at = (packed == w).nonzero().reshape(-1)
    assert 1 <= at.numel() <= 2                                                 # layers_dir.0's alpha row, in its one or two sections
    bad = packed.clone()
    bad[at] = float("nan")
    full = ops.mlp_fwd(m.FAMILY, "f32", bad, cond, ro, rd, z)
    assert bool(torch.isnan(full[..., 3]).all()) and not bool(torch.isnan(full[..., :3]).any())
    _check(gpu, m, shape, ro, rd, z, bad, cond, full)
