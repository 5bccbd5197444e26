"""Exact-f32 inference forward with the colour layers on live samples only (k_paper_mlp_fwd_live, ops.mlp_fwd_live) against the full
forward on the same inputs, bit for bit, and the validation render with the path on against the path off, bit for bit.  GPU only;
nothing here has a tolerance.

A point is live when !(sigma_raw <= 0) or it is the last sample of its ray, with sigma_raw taken from the FULL kernel."""
import pytest
import torch

from oracle import cases as C
from oracle import nerface_oracle as O
from tests import util as U

pytestmark = pytest.mark.gpu

# (rays, samples, max_workgroups): one point; 15 points; ragged, no multiple of 16, 32 or 128, 290 workgroups' worth; a whole number of
# workgroups; 2048 points on two workgroups -- eight passes per wave, so that a wave's 64-row ring wraps
SHAPES = [(1, 1, 0), (3, 5, 0), (1000, 37, 0), (64, 64, 0), (32, 64, 2)]
# fc_alpha.bias of the three liveness regimes.  The hard-head weights of seed 1 give raw densities within +-16 at bias 5 on these
# points (CPU oracle): +-1e6 puts every density on one side
REGIMES = {"dead": -1.0e6, "live": 1.0e6, "mixed": 5.0}
NAN_PAYLOAD = 0x7FC0BEEF
GUARD = 64

_STATE = {}


def _model(gpu):
    import nerf
    if "m" not in _STATE:
        c = C.build_case("eval_det_64_128")
        m = U.make_model(nerf, c["p_fine"], gpu).eval()             # seed 1: the mixed regime's live fraction is 0.35 .. 0.47 (asserted below)
        assert m.fused_supported()
        _STATE.update(m=m, expr=c["expr"].to(gpu), latent=c["latent"].to(gpu))
    return _STATE["m"], _STATE["expr"], _STATE["latent"]


def _points(n_rays, s, seed):
    g = torch.Generator().manual_seed(seed)
    ro, rd, _, _, _ = C.ray_subset(512, 512, 3, n_rays, seed + 7)
    z = torch.sort(torch.rand((n_rays, s), generator=g) * 0.6 + 0.2, dim=-1)[0]
    return ro, rd, z


def _full(gpu, regime, i):
    """(inputs, packed image, bias table, the full kernel's raw) of shape i in a regime: computed once, shared, never modified."""
    import nerf
    from nerf import ops
    key = (regime, i)
    if key not in _STATE:
        m, expr, latent = _model(gpu)
        nerf.set_mlp_precision("f32")
        with torch.no_grad():
            m.fc_alpha.bias.fill_(REGIMES[regime])
        n_rays, s, _ = SHAPES[i]
        ro, rd, z = (t.to(gpu) for t in _points(n_rays, s, 31 + i))
        packed = m.hip_weights().get().clone()
        cond = ops.mlp_condition(m.FAMILY, packed, expr, latent, O.NEAR, O.FAR)
        _STATE[key] = (ro, rd, z, packed, cond, ops.mlp_fwd(m.FAMILY, "f32", packed, cond, ro, rd, z))
    return _STATE[key]


def _live_mask(raw):
    live = ~(raw[..., 3] <= 0)
    live[:, -1] = True
    return live


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[f"{r}x{s}" + (f"_wg{w}" if w else "") for r, s, w in SHAPES])
@pytest.mark.parametrize("regime", list(REGIMES))
def test_live_kernel_is_the_full_forward_where_colour_counts(hip_lib, gpu, regime, i):
    """sigma torch.equal at every point; rgb torch.equal at every live point and exactly 0.0 at every dead one; nothing written outside
    raw.  "dead": no colour run before a wave's final flush; "live": one on every pass; "mixed": the live fraction is asserted to lie
    in [0.2, 0.8] for every shape of 1000 points or more (a single point has no fraction)."""
    from nerf import _hip as H
    from nerf import ops
    m, _, _ = _model(gpu)
    n_rays, s, wgs = SHAPES[i]
    ro, rd, z, packed, cond, full = _full(gpu, regime, i)
    sig_pos = ~(full[..., 3] <= 0)
    if regime == "dead":
        assert not bool(sig_pos.any())
    elif regime == "live":
        assert bool(sig_pos.all())
    elif n_rays * s >= 1000:
        frac = float(sig_pos.float().mean())
        print(f"mixed {n_rays}x{s}: live fraction {frac:.3f}")
        assert 0.2 <= frac <= 0.8
    live = _live_mask(full)
    before = ops.live_colour_launches()
    got = ops.mlp_fwd_live(m.FAMILY, packed, cond, ro, rd, z, max_workgroups=wgs)
    assert ops.live_colour_launches() == before + 1
    assert got.shape == full.shape and got.dtype == torch.float32
    assert torch.equal(got[..., 3], full[..., 3]), (regime, n_rays, s)
    assert torch.equal(got[..., :3][live], full[..., :3][live]), (regime, n_rays, s)
    dead_rgb = got[..., :3][~live]
    assert bool((dead_rgb.view(torch.int32) == 0).all()), (regime, n_rays, s)                  # +0.0, not merely == 0
    # the C entry point on a buffer with poisoned guards: every point written, nothing beside them
    n = n_rays * s
    buf = torch.full((4 * n + 2 * GUARD,), NAN_PAYLOAD, dtype=torch.int32, device=gpu)
    scratch = torch.empty(m.FAMILY.fn("mlp_fwd_live_scratch_floats")(wgs), dtype=torch.float32, device=gpu)
    m.FAMILY.call("mlp_fwd_live", H.ptr(packed), H.ptr(cond), H.ptr(ro), H.ptr(rd), 0, H.ptr(z), n_rays, s, buf.data_ptr() + 4 * GUARD,
                  H.ptr(scratch), scratch.numel(), wgs, H.stream_ptr(gpu))
    assert torch.equal(buf[GUARD:GUARD + 4 * n].view(torch.float32).reshape(n_rays, s, 4), got), (regime, n_rays, s)
    assert bool((buf[:GUARD] == NAN_PAYLOAD).all()) and bool((buf[GUARD + 4 * n:] == NAN_PAYLOAD).all()), (regime, n_rays, s)


def test_entry_refuses_a_short_or_missing_scratch(hip_lib, gpu):
    from nerf import _hip as H
    m, _, _ = _model(gpu)
    ro, rd, z, packed, cond, full = _full(gpu, "mixed", 1)
    need = m.FAMILY.fn("mlp_fwd_live_scratch_floats")(2)
    assert need == 2 * 4 * (64 * (1024 + 64 + 16) // 4)
    scratch = torch.empty(need, dtype=torch.float32, device=gpu)
    raw = torch.empty_like(full)
    args = (H.ptr(packed), H.ptr(cond), H.ptr(ro), H.ptr(rd), 0, H.ptr(z), 3, 5, H.ptr(raw))
    fn = m.FAMILY.fn("mlp_fwd_live")
    assert fn(*args, 0, need, 2, H.stream_ptr(gpu)) != 0
    assert fn(*args, H.ptr(scratch), need - 1, 2, H.stream_ptr(gpu)) != 0
    assert fn(*args, H.ptr(scratch), need, -1, H.stream_ptr(gpu)) != 0
    assert fn(*args, H.ptr(scratch), need, 2, H.stream_ptr(gpu)) == 0
    torch.cuda.synchronize(gpu)


def _render(gpu, noise_std=0.0, bg=None, white=False, grad=False):
    import nerf
    c = C.build_case("eval_det_64_128")
    if "mc" not in _STATE:
        _STATE["mc"] = U.make_model(nerf, c["p_coarse"], gpu)
        _STATE["mf"] = U.make_model(nerf, c["p_fine"], gpu)
    ro, rd, _, _, _ = C.ray_subset(512, 512, 3, 256, 21)
    ro, rd = ro.reshape(16, 16, 3).to(gpu), rd.reshape(16, 16, 3).to(gpu)
    ex, ed = U.encoders(nerf)
    opt = U.make_options(nerf, 64, 128, True, noise_std, white=white)
    nerf.set_mlp_precision("f32")
    torch.manual_seed(1234)
    with torch.enable_grad() if grad else torch.no_grad():
        return nerf.run_one_iter_of_nerf(16, 16, None, _STATE["mc"], _STATE["mf"], ro, rd, opt, mode="validation", encode_position_fn=ex,
                                         encode_direction_fn=ed, expressions=c["expr"].to(gpu), background_prior=bg,
                                         latent_code=c["latent"].to(gpu))


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("with_bg", [False, True])
def test_validation_render_is_the_same_with_the_path_on_and_off(hip_lib, gpu, with_bg, white):
    """run_one_iter_of_nerf(mode="validation") under no_grad, 256 rays, 64 + 128 samples: all seven outputs torch.equal between
    ops.set_live_colour(True) and (False); on, both passes run the live kernel, off, none does."""
    from nerf import ops
    bg = torch.rand((256, 3), generator=torch.Generator().manual_seed(3)).to(gpu) if with_bg else None
    try:
        ops.set_live_colour(True)
        n0 = ops.live_colour_launches()
        on = _render(gpu, bg=bg, white=white)
        assert ops.live_colour_launches() == n0 + 2                       # the coarse and the fine pass of the one chunk
        ops.set_live_colour(False)
        off = _render(gpu, bg=bg, white=white)
        assert ops.live_colour_launches() == n0 + 2
    finally:
        ops.set_live_colour(None)
    assert len(on) == len(off) == 7
    for k in range(7):
        assert on[k].shape == off[k].shape and torch.equal(on[k], off[k]), (with_bg, white, k)


def test_noise_or_grad_keeps_the_full_kernel(hip_lib, gpu):
    """With radiance_field_noise_std > 0 the ReLU argument is sigma + noise, and with grad enabled the training forward runs: the
    live kernel is not launched (its launch counter stands still) although the switch is on."""
    from nerf import ops
    try:
        ops.set_live_colour(True)
        n0 = ops.live_colour_launches()
        _render(gpu, noise_std=1.0)
        assert ops.live_colour_launches() == n0
        out = _render(gpu, grad=True)
        assert out[3].requires_grad and ops.live_colour_launches() == n0
        _render(gpu)
        assert ops.live_colour_launches() == n0 + 2                       # (the counter does move when the path is taken)
        ops.set_live_colour(True, passes=("coarse",))
        _render(gpu)
        assert ops.live_colour_launches() == n0 + 3                       # (and the switch is per pass)
    finally:
        ops.set_live_colour(None)
