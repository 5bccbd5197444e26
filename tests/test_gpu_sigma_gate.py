"""The gated exact-f32 forward (csrc/nf_mlp_gated.hip: fc_feat, too, only where a bound on sigma cannot prove the sample dead) against
the full forward, through the C entry points with `raw` and `scratch` poisoned.  GPU only; nothing here has a tolerance.

Per point, with sigma_raw taken from the FULL kernel: where !(sigma <= 0), or on a ray's last sample, all four channels are the full
forward's bits; elsewhere rgb is +0.0 and sigma is the full forward's bits or < 0.  volume_render_fwd of either `raw` is torch.equal in
every output.  From the statistics instantiation: the units sum to ceil(n / 32), no proven row is live, and the kernel proves every row
that the CPU restatement (tests/sigma_bound_ref.py) proves with the coefficient doubled to 2^-12 -- a condition with a wide margin (the
two sum the same terms in different orders and from trunks that differ by rounding), not a tolerance.

Model, points and the ten fc_alpha biases are those of tests/test_gpu_live_fill.py (live fractions 0.01 .. 0.998)."""
import pytest
import torch

from oracle import cases as C
from oracle import nerface_oracle as O
from tests import sigma_bound_ref as B
from tests.test_gpu_live_colour import GUARD, NAN_PAYLOAD, _live_mask, _model, _points
from tests.test_gpu_live_fill import BIASES

pytestmark = pytest.mark.gpu

# (rays, samples, max_workgroups): 1, 31, 32, 33 and 737 points; 2048 points on one workgroup and on two; S = 1 (every sample a last one)
SHAPES = {"1": (1, 1, 0), "31": (1, 31, 0), "32": (2, 16, 0), "33": (3, 11, 0), "737": (67, 11, 0), "2048_wg1": (32, 64, 1),
          "2048_wg2": (32, 64, 2), "S1": (40, 1, 0)}
SEEDS = {"1": 44, "31": 46, "32": 47, "33": 48, "737": 43, "2048_wg1": 41, "2048_wg2": 41, "S1": 49}
CASES = ([(s, b) for s in ("2048_wg1", "2048_wg2") for b in BIASES] + [(s, b) for s in ("1", "31", "32", "33", "737", "S1") for b in (1.0, 8.0)])

_STATE = {}


def _c():
    if "c" not in _STATE:
        _STATE["c"] = C.build_case("eval_det_64_128")
    return _STATE["c"]


def _params(gpu):
    """The model's weights as the oracle's dict (CPU), with the fc_alpha head as the model has it now."""
    m, _, _ = _model(gpu)
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def _inputs(gpu, shape):
    if ("in", shape) not in _STATE:
        n_rays, s, _ = SHAPES[shape]
        ro, rd, z = _points(n_rays, s, SEEDS[shape])
        x87 = O.encode_points(ro, rd, z, O.NEAR, O.FAR).reshape(-1, 87)
        _STATE[("in", shape)] = (ro.to(gpu), rd.to(gpu), z.to(gpu), x87)
    return _STATE[("in", shape)]


def _images(gpu, setup):
    """(packed, bound, cond, params on the CPU) with the model's head changed by `setup(m)` -- copies: the model is shared."""
    import nerf
    from nerf import ops
    m, expr, latent = _model(gpu)
    nerf.set_mlp_precision("f32")
    with torch.no_grad():
        setup(m)
    packed = m.hip_weights().get().clone()
    return packed, ops.sigma_bound(m.FAMILY, packed), ops.mlp_condition(m.FAMILY, packed, expr, latent, O.NEAR, O.FAR), _params(gpu)


def _case(gpu, shape, bias):
    key = (shape, bias)
    if key not in _STATE:
        from nerf import ops
        m, _, _ = _model(gpu)
        packed, bound, cond, p = _images(gpu, lambda mm: mm.fc_alpha.bias.fill_(bias))
        ro, rd, z, _ = _inputs(gpu, shape)
        _STATE[key] = (packed, bound, cond, p, ops.mlp_fwd(m.FAMILY, "f32", packed, cond, ro, rd, z))
    return _STATE[key]


def _run(gpu, shape, packed, bound, cond, stats=False, stream=None):
    """The C entry point on poisoned buffers -> (raw buffer with its guards, stats or None); nothing is synchronised here."""
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
        st = torch.full((rows, 5), -1, dtype=torch.int64, device=gpu)
        m.FAMILY.call("mlp_fwd_gated_stats", *args, st.data_ptr(), rows, sp)
    else:
        m.FAMILY.call("mlp_fwd_gated", *args, sp)
    return (buf, scratch), st


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
    assert torch.equal(got[live], want[live]), shape
    assert bool((got[..., :3][~live] == 0).all()), shape                        # +0.0, not merely == 0
    same = got[..., 3] == want[..., 3]
    neg = got[..., 3].view(torch.float32) < 0
    assert bool((same | neg)[~live].all()), shape
    raw = got.view(torch.float32).contiguous()
    for a, b in zip(ops.volume_render_fwd(raw, z, rd), ops.volume_render_fwd(full, z, rd)):
        # (the NaN case: torch.equal is false on NaN outputs even of the same `raw`; there the bits must be the same)
        assert torch.equal(a, b) or (bool(torch.isnan(b).any()) and torch.equal(a.view(torch.int32), b.view(torch.int32))), shape
    return ~same


def _cpu_proves(p, shape, coef):
    _, s, _ = SHAPES[shape]
    x87 = _STATE[("in", shape)][3]
    h, _ = B.trunk(p, x87, _c()["expr"], _c()["latent"])
    proven = B.gate(h.numpy(), *B.bound_vectors(p), coef=coef)[3]
    proven[s - 1::s] = False                                                   # a ray's last sample is never proven
    return proven


@pytest.mark.parametrize("shape,bias", CASES, ids=[f"{s}_bias{b}" for s, b in CASES])
def test_gated_kernel_is_the_full_forward_where_it_counts(hip_lib, gpu, shape, bias):
    packed, bound, cond, p, full = _case(gpu, shape, bias)
    (buf, _), _ = _run(gpu, shape, packed, bound, cond)
    changed = _check(gpu, shape, buf, full)
    (buf2, _), st = _run(gpu, shape, packed, bound, cond, stats=True)
    assert torch.equal(buf2, buf), shape                                        # the statistics instantiation computes the same
    n_rays, s, wgs = SHAPES[shape]
    n = n_rays * s
    st = st.cpu().numpy()
    used = st[:, 0] >= 0
    assert int(st[used, 0].sum()) == (n + 31) // 32, shape
    n_proven = int(st[used, 4].sum())
    live = _live_mask(full).reshape(-1).cpu().numpy()
    changed = changed.reshape(-1).cpu().numpy()
    assert not bool((changed & live).any()) and int(changed.sum()) <= n_proven <= int((~live).sum()), shape
    # every row the restatement proves at 2^-12 is among the kernel's (a proven row whose bound equals its density bit for bit
    # cannot be told from a gathered one: the count allows for those)
    cpu = _cpu_proves(p, shape, 2.0 ** -12)
    print(f"{shape} bias {bias}: live {live.mean():.3f}, kernel proves {n_proven} of {int((~live).sum())} dead rows, CPU at 2^-12 {int(cpu.sum())}")
    assert not bool((cpu & live).any()), shape
    assert int((cpu & ~changed).sum()) <= n_proven - int(changed.sum()), shape


def test_cancelling_net_is_never_proven_wrongly(hip_lib, gpu):
    """fc_alpha x 1e-3 with the bias at minus the median density: densities crowd around zero, half of them on either side.  The
    kernel's contract holds whatever it proves there (it still proves most dead rows: the share is printed, not asserted)."""
    from nerf import ops
    m, expr, latent = _model(gpu)
    ro, rd, z, x87 = _inputs(gpu, "737")
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
    full = ops.mlp_fwd(m.FAMILY, "f32", packed, cond, ro, rd, z)
    frac = float((~(full[..., 3] <= 0)).float().mean())
    assert 0.3 < frac < 0.7, frac
    (buf, _), st = _run(gpu, "737", packed, bound, cond, stats=True)
    _check(gpu, "737", buf, full)
    print(f"cancelling net: live {frac:.3f}, proven {int(st[st[:, 0] >= 0, 4].sum())} of 737")


@pytest.mark.parametrize("shape", ["737", "33"])
def test_nan_in_fc_alpha_proves_nothing(hip_lib, gpu, shape):
    """A NaN in one weight of fc_alpha (on a copy of the packed image, the bound image built from that copy): w and v are NaN, no
    comparison holds, every row is gathered and every density is the full forward's NaN, bit for bit."""
    from nerf import ops
    m, _, _ = _model(gpu)
    packed, _, cond, _, _ = _case(gpu, shape, 8.0)
    ro, rd, z, _ = _inputs(gpu, shape)
    with torch.no_grad():
        m.fc_alpha.bias.fill_(8.0)
    w = m.fc_alpha.weight.detach()[0, 17]
    at = (packed == w).nonzero().reshape(-1)
    assert 1 <= at.numel() <= 2
    bad = packed.clone()
    bad[at] = float("nan")
    bound = ops.sigma_bound(m.FAMILY, bad)
    assert bool(torch.isnan(bound[:4096].reshape(16, 64, 4)[:, ::16]).all())            # rows 0 of every chunk: w
    full = ops.mlp_fwd(m.FAMILY, "f32", bad, cond, ro, rd, z)
    assert bool(torch.isnan(full[..., 3]).all())
    (buf, _), st = _run(gpu, shape, bad, bound, cond, stats=True)
    changed = _check(gpu, shape, buf, full)
    assert not bool(changed.any()) and int(st[st[:, 0] >= 0, 4].sum()) == 0


def test_three_launches_without_a_synchronise(hip_lib, gpu):
    packed, bound, cond, _, full = _case(gpu, "2048_wg2", 8.0)
    outs = [_run(gpu, "2048_wg2", packed, bound, cond) for _ in range(3)]
    torch.cuda.synchronize()
    for (buf, _), _ in outs:
        _check(gpu, "2048_wg2", buf, full)
        assert torch.equal(buf, outs[0][0][0])


def test_two_streams_in_flight_together(hip_lib, gpu):
    a = _case(gpu, "2048_wg1", 4.5)
    b = _case(gpu, "2048_wg2", 10.5)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
    outs = []
    for _ in range(2):
        outs.append(("2048_wg1", a[4], _run(gpu, "2048_wg1", *a[:3], stream=s1)))
        outs.append(("2048_wg2", b[4], _run(gpu, "2048_wg2", *b[:3], stream=s2)))
    s1.synchronize()
    s2.synchronize()
    for shape, full, ((buf, _), _) in outs:
        _check(gpu, shape, buf, full)


def test_entry_refuses_a_missing_bound_or_scratch(hip_lib, gpu):
    from nerf import _hip as H
    m, _, _ = _model(gpu)
    packed, bound, cond, _, full = _case(gpu, "33", 8.0)
    ro, rd, z, _ = _inputs(gpu, "33")
    assert m.FAMILY.fn("sigma_bound_floats")() == 4096 + 16
    need = m.FAMILY.fn("mlp_fwd_live_scratch_floats")(2)
    scratch = torch.empty(need, dtype=torch.float32, device=gpu)
    raw = torch.empty_like(full)
    fn = m.FAMILY.fn("mlp_fwd_gated")
    tail = (H.ptr(cond), H.ptr(ro), H.ptr(rd), 0, H.ptr(z), 3, 11, H.ptr(raw))
    assert fn(H.ptr(packed), 0, *tail, H.ptr(scratch), need, 2, H.stream_ptr(gpu)) != 0
    assert fn(H.ptr(packed), H.ptr(bound) + 4, *tail, H.ptr(scratch), need, 2, H.stream_ptr(gpu)) != 0
    assert fn(H.ptr(packed), H.ptr(bound), *tail, H.ptr(scratch), need - 1, 2, H.stream_ptr(gpu)) != 0
    assert fn(H.ptr(packed), H.ptr(bound), *tail, H.ptr(scratch), need, 2, H.stream_ptr(gpu)) == 0
    assert m.FAMILY.fn("sigma_bound")(H.ptr(packed), 0, H.stream_ptr(gpu)) != 0
    torch.cuda.synchronize(gpu)


@pytest.mark.parametrize("with_bg", [False, True])
def test_validation_render_is_the_same_with_the_gate_on_and_off(hip_lib, gpu, with_bg):
    """run_one_iter_of_nerf(mode="validation") under no_grad, 256 rays, 64 + 128 samples: all seven outputs torch.equal between
    ops.set_sigma_gate(True) -- both passes run the gated kernel, each model's bound image is built once -- and (False), the live kernel."""
    from nerf import ops
    from tests.test_gpu_live_colour import _render
    bg = torch.rand((256, 3), generator=torch.Generator().manual_seed(3)).to(gpu) if with_bg else None
    try:
        ops.set_sigma_gate(True)
        n0, l0 = ops.sigma_gate_launches(), ops.live_colour_launches()
        on = _render(gpu, bg=bg)
        assert ops.sigma_gate_launches() == n0 + 2 and ops.live_colour_launches() == l0
        ops.set_sigma_gate(True, passes=("coarse",))
        mixed = _render(gpu, bg=bg)
        assert ops.sigma_gate_launches() == n0 + 3 and ops.live_colour_launches() == l0 + 1
        _render(gpu, noise_std=1.0)                                              # noise: the full kernel
        assert ops.sigma_gate_launches() == n0 + 3 and ops.live_colour_launches() == l0 + 1
        ops.set_sigma_gate(False)
        off = _render(gpu, bg=bg)
        assert ops.sigma_gate_launches() == n0 + 3
    finally:
        ops.set_sigma_gate(None)
    assert len(on) == len(off) == len(mixed) == 7
    for k in range(7):
        assert torch.equal(on[k], off[k]) and torch.equal(mixed[k], off[k]), (with_bg, k)
