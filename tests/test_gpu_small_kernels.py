"""The small kernels around the fused MLP and the renderer, at their edges: the ray draw (csrc/nf_choice.hip), the one-launch Adam
step (csrc/nf_optim.hip), the stand-alone positional encoder and the eval post-processing (csrc/nf_rays.hip).  Every reference is
plain torch / numpy on the CPU, in float64 unless stated.  GPU only."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import nerface_oracle as O
from tests import util as U

pytestmark = pytest.mark.gpu

SMALL_SIZES = (1, 63, 64, 255, 256, 257, 1023, 1025)
LADDER_ITEMS = 263000            # > 262,144: 1028 tiles of 256 items on 1024 compaction workgroups, two tiles each, a ragged tail


# =====================================================================================================================
# 1. ray selection
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def _ladder(n_items, mod):
    """w_i = 2^-k_i with k_i = (i * 7919) % mod and u = 0.5: key_i = c * 2^k_i exactly (division by a power of two), c = -logf(0.5).
    Returns (w, u, k, the indices ordered by (k_i, i))."""
    k = (torch.arange(n_items, dtype=torch.int64) * 7919) % mod
    w = torch.pow(torch.tensor(2.0, dtype=torch.float64), -k.double()).float()
    assert bool((w.double().log2() == -k.double()).all())
    return w, torch.full((n_items,), 0.5), k, torch.argsort(k, stable=True)


def _ladder_expected(n_items, mod, n):
    return torch.sort(_ladder(n_items, mod)[3][:n])[0]


def _ladder_ns():
    k = _ladder(LADDER_ITEMS, 97)[2]
    sizes = torch.bincount(k, minlength=97)
    boundary = int(sizes[:41].sum())                       # classes 0..40 taken whole: `remaining` equals the size of class 40
    return {"inside": boundary + 1000, "boundary": boundary, "one": 1, "batch": 2048, "all": LADDER_ITEMS}, int(sizes[41])


@pytest.mark.parametrize("which", ["inside", "boundary", "one", "batch", "all"])
def test_choice_exact_ladder(hip_lib, gpu, which):
    """1a.  263,000 items in 97 tie classes, 97 binades apart at level 0 of the radix select: the draw is exactly the n smallest
    (k_i, i), ascending, and a second call repeats it.  No tolerance.  (The expectation does not depend on the sign of the key of
    u = 0, so this is also the statement that correcting that key changed no other draw.)"""
    from nerf import ops
    ns, next_class = _ladder_ns()
    n = ns[which]
    assert 1000 < next_class                               # "inside" ends inside class 41
    w, u, _, _ = _ladder(LADDER_ITEMS, 97)
    want = _ladder_expected(LADDER_ITEMS, 97, n)
    wd, ud = w.to(gpu), u.to(gpu)
    got = ops.weighted_choice(wd, n, u=ud, check=True).cpu()
    assert got.shape == want.shape and torch.equal(got, want), int((got != want).sum())
    assert torch.equal(ops.weighted_choice(wd, n, u=ud).cpu(), want)


@pytest.mark.parametrize("n_items", SMALL_SIZES)
def test_choice_small_sizes(hip_lib, gpu, n_items):
    """1b.  Fewer items than a tile, a tile, a tile and one, four tiles and one: the ladder with 5 classes, n = 1, half, all."""
    from nerf import ops
    w, u, _, _ = _ladder(n_items, 5)
    for n in sorted({1, n_items // 2, n_items}):
        got = ops.weighted_choice(w.to(gpu), n, u=u.to(gpu), check=True).cpu()
        want = _ladder_expected(n_items, 5, n)
        assert got.shape == (n,) and got.dtype == torch.int64 and torch.equal(got, want), (n_items, n, got.tolist()[:8], want.tolist()[:8])


@pytest.mark.parametrize("n_items", [5000, 70001])
def test_choice_u_zero_selects_the_item(hip_lib, gpu, n_items):
    """1c.  u = 0 is a value torch.rand returns; its key is 0, the smallest possible, so the item is always drawn.  (Before the sign
    bit of the key was cleared it was -0.0 / w = 0x80000000, which the overflow clamp turned into the LARGEST finite key, so
    that the u = 0 items came last among the positive items: on an MI355X, with u = 0 at items 1667 and 3334 of 5000, n = 1 drew
    [4622] and n = 2 drew [3104, 4622], and only the draw of every positive item held the two.)  A
    weight-0 item with u = 0 is still never drawn."""
    from nerf import ops
    g = torch.Generator().manual_seed(31)
    w = torch.rand(n_items, generator=g) + 0.01
    w[::7] = 0.0
    u = torch.rand(n_items, generator=g)
    j1, j2, j0 = n_items // 3 + 1, (2 * n_items) // 3 + 1, 7 * (n_items // 14)
    assert w[j1] > 0 and w[j2] > 0 and w[j0] == 0 and j1 < j2
    u[u == 0] = 0.5
    u[j1] = u[j2] = u[j0] = 0.0
    wd, ud = w.to(gpu), u.to(gpu)
    one = ops.weighted_choice(wd, 1, u=ud, check=True).cpu().tolist()
    two = ops.weighted_choice(wd, 2, u=ud, check=True).cpu().tolist()
    print(f"u = 0 at items {j1}, {j2} (positive weight) and {j0} (weight 0): n = 1 draws {one}, n = 2 draws {two}")
    assert one == [j1], (one, j1)
    assert two == [j1, j2], (two, j1, j2)
    n_pos = int((w > 0).sum())
    for n in (3, 2048, n_pos):
        got = ops.weighted_choice(wd, n, u=ud, check=True).cpu()
        s = set(got.tolist())
        assert len(s) == n and j1 in s and j2 in s and j0 not in s and bool((w[got] > 0).all()), n


def test_choice_key_extremes(hip_lib, gpu):
    """1d.  The ends of the key range.  u = 1 - 2^-24 with weights 1e-38 and (subnormal) 1e-42: the quotient overflows and is clamped to
    the largest finite key, so the item loses to every unclamped key but still beats weight 0, and among clamped keys the lowest
    indices win.  Weights NaN, negative, -0.0 and -inf are never drawn; weight +inf has key 0 and is always drawn."""
    from nerf import ops
    n_items = 3000
    g = torch.Generator().manual_seed(41)
    role = torch.randperm(n_items, generator=g) % 10       # 0-3 ordinary, 4-5 weight 1e-38, 6 weight 1e-42, 7 +inf, 8-9 never chosen
    w = torch.ones(n_items)
    u = torch.rand(n_items, generator=g)
    u[u == 0] = 0.5
    top = float(np.float32(1.0) - np.float32(2.0 ** -24))
    assert top < 1.0 and float(np.nextafter(np.float32(top), np.float32(2.0))) == 1.0
    w[(role == 4) | (role == 5)] = 1e-38
    w[role == 6] = 1e-42
    assert float(w[role == 6][0]) > 0 and float(w[role == 6][0]) < 2.0 ** -126
    u[(role >= 4) & (role <= 6)] = top
    w[role == 7] = float("inf")
    never = torch.nonzero(role >= 8).reshape(-1)
    w[never] = torch.tensor([0.0, -0.0, float("nan"), -1.0, -float("inf"), -1e-42])[torch.arange(never.numel()) % 6]
    inf_i = torch.nonzero(role == 7).reshape(-1)
    ordinary = torch.nonzero(role <= 3).reshape(-1)
    clamped = torch.nonzero((role >= 4) & (role <= 6)).reshape(-1)
    positive = torch.nonzero(role <= 7).reshape(-1)
    wd, ud = w.to(gpu), u.to(gpu)
    draw = lambda n, **kw: ops.weighted_choice(wd, n, u=ud, **kw).cpu()
    assert torch.equal(draw(positive.numel(), check=True), positive)                       # every positive item, no other
    for m in (1, 257, clamped.numel() - 1):                                                # clamped keys: the m lowest indices
        want = torch.sort(torch.cat((inf_i, ordinary, clamped[:m])))[0]
        assert torch.equal(draw(want.numel(), check=True), want), m
    assert torch.equal(draw(inf_i.numel() + ordinary.numel(), check=True), torch.sort(torch.cat((inf_i, ordinary)))[0])
    assert torch.equal(draw(inf_i.numel(), check=True), inf_i)                             # key 0 beats every positive key
    assert torch.equal(draw(5, check=True), inf_i[:5])
    short = draw(positive.numel() + 3)                                                     # the items that can never be drawn stay out
    assert torch.equal(short[:-3], positive) and short[-3:].tolist() == [-1, -1, -1]
    with pytest.raises(ValueError):
        draw(positive.numel() + 1, check=True)


@pytest.mark.parametrize("n_items,n,seed", [(300001, 2048, 11), (5000, 1000, 12)])
def test_choice_wide_range_band(hip_lib, gpu, n_items, n, seed):
    """1e.  Weights log-uniform over 60 decades (every 97th zero), torch.rand for u.  With T the n-th smallest float64 key
    -log(double(float32(1 - u))) / double(w): every item with key < T (1 - d) is drawn, none with key > T (1 + d), n distinct
    ascending indices.  d = tests.util.CHOICE_KEY_D.  The inputs are chosen (and checked here, and beforehand on the CPU) such that
    at most 2 items lie inside the band, the n-th itself included."""
    from nerf import ops
    d = U.CHOICE_KEY_D
    g = torch.Generator().manual_seed(seed)
    w = torch.pow(10.0, torch.rand(n_items, generator=g, dtype=torch.float64) * 60 - 30).float()
    w[::97] = 0.0
    u = torch.rand(n_items, generator=g)
    key = U.choice_reference_keys(w, u)
    T = float(torch.sort(key)[0][n - 1])
    assert 0 < T < float("inf")
    assert int(((key >= T * (1 - d)) & (key <= T * (1 + d))).sum()) <= 2                   # condition on the inputs, not a measurement
    idx = ops.weighted_choice(w.to(gpu), n, u=u.to(gpu), check=True).cpu()
    assert idx.shape == (n,) and bool((idx[1:] > idx[:-1]).all()) and int(idx[0]) >= 0 and int(idx[-1]) < n_items
    chosen = torch.zeros(n_items, dtype=torch.bool)
    chosen[idx] = True
    print(f"{n_items} items, n = {n}: largest chosen key / smallest unchosen key - 1 = {float(key[chosen].max() / key[~chosen].min()) - 1:.3e} "
          f"(<= 0: exactly the n smallest float64 keys)")
    assert bool(chosen[key < T * (1 - d)].all())
    assert not bool(chosen[key > T * (1 + d)].any())


@pytest.mark.parametrize("n_items", SMALL_SIZES + (LADDER_ITEMS,))
def test_choice_too_few_positive_weights(hip_lib, gpu, n_items):
    """1f.  Fewer than n items of positive weight: without the check the first p entries are the positive items in index order and
    the rest is exactly -1; with the check ValueError, as np.random.choice raises."""
    from nerf import ops
    g = torch.Generator().manual_seed(n_items)
    w = torch.rand(n_items, generator=g) + 0.01
    w[torch.arange(n_items) % 3 != 1] = 0.0                # n_items = 1: no positive item at all
    pos = torch.nonzero(w > 0).reshape(-1)
    p = int(pos.numel())
    u = torch.rand(n_items, generator=g)
    for n in sorted({p + 1, min(n_items, p + 1000), n_items}):
        got = ops.weighted_choice(w.to(gpu), n, u=u.to(gpu)).cpu()
        assert got.shape == (n,) and torch.equal(got[:p], pos) and bool((got[p:] == -1).all()), (n_items, n)
        with pytest.raises(ValueError):
            ops.weighted_choice(w.to(gpu), n, u=u.to(gpu), check=True)


@pytest.mark.parametrize("fill", [0xFF, 0x5A])
def test_choice_dirty_workspace_and_output(hip_lib, gpu, fill):
    """1g.  The C entry owes nothing to what its workspace and its output held before: both pre-filled with 0xff bytes (and with
    another pattern), a full draw and a short one (whose missing entries must still come out as -1)."""
    from nerf import _hip as H
    ws_bytes = int(hip_lib.nf_weighted_choice_workspace_bytes())
    g = torch.Generator().manual_seed(51)
    for n_items, n, n_zero_from in ((LADDER_ITEMS, 2048, None), (5000, 1000, None), (5000, 1000, 600)):
        w = torch.rand(n_items, generator=g) + 0.01
        if n_zero_from is not None:
            w[n_zero_from:] = 0.0
        u = torch.rand(n_items, generator=g)
        wd, ud = w.to(gpu), u.to(gpu)
        out = []
        for dirty in (False, True):
            ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=gpu)
            idx = torch.zeros(n, dtype=torch.int64, device=gpu)
            if dirty:
                ws.fill_(fill)
                idx.view(torch.uint8).fill_(fill)
            with torch.cuda.device(gpu):
                H.check(hip_lib.nf_weighted_choice(H.ptr(wd), H.ptr(ud), n_items, n, H.ptr(idx), H.ptr(ws), ws_bytes, H.stream_ptr(gpu)),
                        "nf_weighted_choice")
            out.append((idx.cpu(), int(ws.view(torch.int32)[5].item())))
        assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] == (0 if n_zero_from is None else 1)
        if n_zero_from is not None:
            assert torch.equal(out[1][0][:n_zero_from], torch.arange(n_zero_from)) and bool((out[1][0][n_zero_from:] == -1).all())


# =====================================================================================================================
# 2. Adam
# =====================================================================================================================
ADAM_LR, ADAM_BETAS, ADAM_EPS = 5e-4, (0.9, 0.999), 1e-8
GUARD = 12345.625                       # what the 4 + offset floats before a view and the floats after it hold
ROLES = ("p", "g", "m", "v")


def _adam_constants(step, lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS):
    """The scalars as nf_adam_step forms them: lr, beta1, beta2, eps arrive as C floats; the bias corrections are formed in double
    from those.  Returns the double values (for the float64 reference) and their float32 roundings (what the kernel is handed)."""
    f = lambda x: float(np.float32(x))
    lr, b1, b2, eps = f(lr), f(betas[0]), f(betas[1]), f(eps)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    dbl = dict(w1=1.0 - b1, beta2=b2, w2=1.0 - b2, step_size=lr / bc1, bc2_sqrt=float(np.sqrt(bc2)), eps=eps)
    return dbl, {k: f(v) for k, v in dbl.items()}


def _adam_reference(p, g, m, v, c, dtype):
    """m <- m + (1 - beta1) (g - m);  v <- beta2 v + (1 - beta2) g g;  p <- p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), one
    rounding per operation in `dtype` (float64: the reference; float32: the kernel's own operation sequence on the CPU).  In numpy:
    every numpy operation is the correctly rounded IEEE one, which torch's CPU sqrt (a vector-library routine) is not."""
    np_t = {torch.float64: np.float64, torch.float32: np.float32}[dtype]
    k = {n: np_t(x) for n, x in c.items()}
    p, g, m, v = (t.numpy().astype(np_t) for t in (p, g, m, v))
    with np.errstate(under="ignore", over="ignore"):
        m = m + k["w1"] * (g - m)
        v = k["beta2"] * v + (k["w2"] * g) * g
        denom = np.sqrt(v) / k["bc2_sqrt"] + k["eps"]
        p = p - k["step_size"] * (m / denom)
    assert p.dtype == m.dtype == v.dtype == np_t
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in (p, m, v))


def _adam_tensor(n, seed, g_scale=1.0, offsets=(0, 0, 0, 0), g=None, m=None, v=None):
    """One parameter with its gradient and moments (CPU float32) and the storage offset (in floats, 0-3) of each of the four."""
    gen = torch.Generator().manual_seed(seed)
    t = dict(p=torch.randn(n, generator=gen) * 0.1, g=torch.randn(n, generator=gen) * g_scale,
             m=torch.randn(n, generator=gen) * 0.01 * g_scale, v=torch.rand(n, generator=gen) * 1e-4 * g_scale * g_scale)
    for name, val in (("g", g), ("m", m), ("v", v)):
        if val is not None:
            t[name] = torch.full((n,), float(val))
    t["off"] = dict(zip(ROLES, offsets))
    return t


def _place(t, gpu):
    """Device views of the four tensors, each contiguous at float offset 4 + off of a guarded buffer of its own (torch's allocations
    are at least 16-byte aligned: off = 0 keeps a view aligned, 1-3 put it 4, 8, 12 bytes past a 16-byte boundary)."""
    bufs, views = {}, {}
    for r in ROLES:
        n, o = t[r].numel(), 4 + t["off"][r]
        bufs[r] = torch.full((o + n + 8,), GUARD, dtype=torch.float32, device=gpu)
        views[r] = bufs[r][o:o + n]
        views[r].copy_(t[r])
        assert views[r].is_contiguous() and (n == 0 or views[r].data_ptr() % 16 == 4 * t["off"][r])
    return bufs, views


def _adam_check(tensors, placed, step, stepped=None):
    """Every stepped tensor against the float32 evaluation (bit for bit) and against float64 (figures printed); guards intact;
    tensors that were not stepped bit-unchanged.  Returns the worst kernel-error / float32-evaluation-error ratio seen."""
    c64, c32 = _adam_constants(step)
    worst = 0.0
    for i, (t, (bufs, views)) in enumerate(zip(tensors, placed)):
        for r in ROLES:
            o, n = 4 + t["off"][r], t[r].numel()
            b = bufs[r].cpu()
            assert bool((b[:o] == GUARD).all()) and bool((b[o + n:] == GUARD).all()), (i, r, "guard")
        got = {r: views[r].cpu() for r in ROLES}
        assert torch.equal(got["g"].view(torch.int32), t["g"].view(torch.int32)), (i, "gradient written")
        if stepped is not None and not stepped[i]:
            for r in "pmv":
                assert torch.equal(got[r].view(torch.int32), t[r].view(torch.int32)), (i, r, "not stepped, yet changed")
            continue
        ref64 = _adam_reference(t["p"], t["g"], t["m"], t["v"], c64, torch.float64)
        ref32 = _adam_reference(t["p"], t["g"], t["m"], t["v"], c32, torch.float32)
        for r, r64, r32 in zip("pmv", ref64, ref32):
            e_k = float((got[r].double() - r64).abs().max()) if r64.numel() else 0.0
            e_32 = float((r32.double() - r64).abs().max()) if r64.numel() else 0.0
            if e_k > 0:
                worst = max(worst, e_k / e_32 if e_32 > 0 else float("inf"))
            # ADAM BOUND = BIT EQUALITY with the float32 evaluation of the three update lines, one numpy operation at a time on the CPU.
            # Measured on an MI355X against that evaluation: 0 differing elements of p, m and v on the 20 tensors of
            # test_adam_sizes_and_steps at steps 1 and 1000 (kernel error / float32-evaluation error against float64 = 1.000 for each
            # of p, m, v), so equality is asserted and no ratio constant K is set.  (torch's own CPU float32 ops are NOT such an
            # evaluation: its sqrt differs from the correctly rounded one in 0.6 % of the elements, 1-21 elements of p per tensor.)
            assert torch.equal(got[r].view(torch.int32), r32.view(torch.int32)), \
                (i, r, n, step, "differs from the float32 evaluation", int((got[r] != r32).sum()), e_k, e_32)
    return worst


def _run_optimizer(gpu, tensors, step, no_grad=()):
    """nerf.optim.Adam over the placed views: state preset to `step - 1` steps with the given moments."""
    import nerf
    placed = [_place(t, gpu) for t in tensors]
    params = [torch.nn.Parameter(v["p"]) for _, v in placed]
    for prm, (_, v) in zip(params, placed):
        assert prm.data_ptr() == v["p"].data_ptr()
    opt = nerf.optim.Adam(params, lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS)
    for i, (prm, (_, v)) in enumerate(zip(params, placed)):
        if i in no_grad:
            continue
        prm.grad = v["g"]
        opt.state[prm] = {"step": torch.tensor(float(step - 1), dtype=torch.float32), "exp_avg": v["m"], "exp_avg_sq": v["v"]}
    opt.step()
    torch.cuda.synchronize()
    for i, prm in enumerate(params):
        if i in no_grad:
            assert len(opt.state[prm]) == 0
        else:
            assert float(opt.state[prm]["step"]) == float(step)
    return placed


ADAM_SIZES = tuple(range(1, 10)) + tuple(range(1020, 1029)) + (2047, 2049)


@pytest.mark.parametrize("step", [1, 2, 1000, 10 ** 6])
def test_adam_sizes_and_steps(hip_lib, gpu, step):
    """Sizes around the 4 elements of a lane, the 1024 of a workgroup and 2048, all in one launch, at step counts whose bias
    corrections run from 0.1 / 0.001 to 1: p, m and v per element."""
    tensors = [_adam_tensor(n, 100 + n, g_scale=10.0 ** -(k % 4)) for k, n in enumerate(ADAM_SIZES)]
    placed = _run_optimizer(gpu, tensors, step)
    print(f"step {step}: worst kernel / float32-evaluation error ratio against float64 {_adam_check(tensors, placed, step):.3f}")


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("role", range(4))
def test_adam_misaligned_views(hip_lib, gpu, role, off):
    """Each of p, g, m, v in turn 4, 8 and 12 bytes off a 16-byte boundary: the whole tensor takes the scalar path, beside an
    aligned tensor in the same launch; the floats on either side of every view keep their guard value."""
    offsets = tuple(off if r == role else 0 for r in range(4))
    tensors = [_adam_tensor(n, 200 + n, offsets=offsets) for n in (1, 5, 1024, 1027, 2049)] + [_adam_tensor(1030, 77)]
    placed = _run_optimizer(gpu, tensors, 3)
    _adam_check(tensors, placed, 3)


@pytest.mark.parametrize("n_tensors", [64, 65])
def test_adam_launch_boundary(hip_lib, gpu, n_tensors):
    """64 tensors fill one launch's block table, the 65th opens a second launch."""
    tensors = [_adam_tensor(ADAM_SIZES[k % len(ADAM_SIZES)], 300 + k, offsets=(0, 0, k % 4, 0)) for k in range(n_tensors)]
    placed = _run_optimizer(gpu, tensors, 5)
    _adam_check(tensors, placed, 5)


def test_adam_gradient_extremes_and_missing_gradient(hip_lib, gpu):
    """g = 0 with m = v = 0 leaves p bit-unchanged; g = 1e-30 (g g underflows to 0: the denominator is eps); g = 1e18; a tensor
    without gradient between them is skipped and its neighbours in the block table are stepped correctly."""
    tensors = [_adam_tensor(1027, 1, g=0.0, m=0.0, v=0.0), _adam_tensor(1025, 2, g=1e-30, m=0.0, v=0.0), _adam_tensor(77, 3),
               _adam_tensor(1026, 4, g=1e18, m=0.0, v=0.0), _adam_tensor(9, 5, g=1e-30), _adam_tensor(9, 6, g=-1e18)]
    for step in (1, 1000):
        placed = _run_optimizer(gpu, tensors, step, no_grad=(2,))
        _adam_check(tensors, placed, step, stepped=[True, True, False, True, True, True])
        assert torch.equal(placed[0][1]["p"].cpu().view(torch.int32), tensors[0]["p"].view(torch.int32))      # g = m = v = 0
        c64, _ = _adam_constants(step)
        m1 = c64["w1"] * 1e-30                                                                                 # denominator = eps
        want = tensors[1]["p"].double() - c64["step_size"] * m1 / c64["eps"]
        assert float((placed[1][1]["p"].cpu().double() - want).abs().max()) <= 2.0 ** -24 * float(want.abs().max())
        assert bool((placed[1][1]["v"].cpu() == 0).all())


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_adam_zero_element_tensor_in_the_block_table(hip_lib, gpu, where):
    """The C entry with a zero-element tensor (valid pointers, numel 0) at the head, in the middle and at the end of the block
    table: nothing around it is written and the tensors after it are stepped correctly."""
    from nerf import _hip as H
    tensors = [_adam_tensor(n, 400 + n) for n in (1025, 3, 2049)]
    tensors.insert({"first": 0, "middle": 2, "last": 3}[where], _adam_tensor(0, 9))
    placed = [_place(t, gpu) for t in tensors]
    n = len(tensors)
    arr = lambda r: (ctypes.c_void_p * n)(*[int(b[r].data_ptr()) + 4 * (4 + t["off"][r]) for t, (b, _) in zip(tensors, placed)])
    numel = (ctypes.c_int64 * n)(*[t["p"].numel() for t in tensors])
    with torch.cuda.device(gpu):
        H.check(hip_lib.nf_adam_step(arr("p"), arr("g"), arr("m"), arr("v"), numel, n, ADAM_LR, ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS, 7,
                                     H.stream_ptr(gpu)), "nf_adam_step")
    torch.cuda.synchronize()
    _adam_check(tensors, placed, 7)


# =====================================================================================================================
# 3. positional encoding
# =====================================================================================================================
def _posenc_input(rows, dim, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((rows, dim), generator=g, dtype=torch.float64) * 8 - 4).float()
    pi = np.float32(np.pi)
    special = [0.0, -0.0, pi, np.nextafter(pi, np.float32(4)), np.nextafter(pi, np.float32(0)), -pi, np.float32(np.pi / 2),
               np.nextafter(np.float32(np.pi / 2), np.float32(0)), 4.0, -4.0]
    flat = x.reshape(-1)
    k = min(len(special), flat.numel())
    flat[:k] = torch.tensor([float(s) for s in special[:k]], dtype=torch.float32)
    return x


def _posenc_reference(x, n_freq, include_input):
    """float64 sin / cos of double(float32(x) * 2^k) (the product is exact in float32), in the encoder's column order."""
    parts = [x.double()] if include_input else []
    for k in range(n_freq):
        a = x * float(2.0 ** k)
        assert torch.equal(a.double(), x.double() * 2.0 ** k)
        parts += [torch.sin(a.double()), torch.cos(a.double())]
    return torch.cat(parts, dim=-1) if parts else x.double()[..., :0]


def _posenc_check(gpu, x, n_freq, include_input, stats):
    from nerf import ops
    rows, dim = x.shape
    out = ops.posenc(x.to(gpu), n_freq, include_input).cpu()
    ref = _posenc_reference(x, n_freq, include_input)
    assert out.shape == ref.shape == (rows, dim * (int(include_input) + 2 * n_freq)) and out.dtype == torch.float32
    if include_input:
        assert torch.equal(out[:, :dim].view(torch.int32), x.view(torch.int32))             # bit for bit, the sign of -0.0 included
    if n_freq == 0:
        return
    o, r = out[:, dim * int(include_input):].double(), ref[:, dim * int(include_input):]
    err = (o - r).abs()
    assert float(err.max()) < 2e-6, (rows, dim, n_freq, include_input, float(err.max()))
    arg = torch.cat([(x.double() * 2.0 ** k).abs() for k in range(n_freq) for _ in (0, 1)], dim=-1)
    ulps = err / torch.from_numpy(np.spacing(np.abs(r.numpy()).astype(np.float32)).astype(np.float64))
    ulps[err == 0] = 0.0
    for name, sel in (("small", arg < 8), ("large", arg >= 8)):
        if bool(sel.any()):
            stats[name] = max(stats.get(name, 0.0), float(ulps[sel].max()))
            stats["abs_" + name] = max(stats.get("abs_" + name, 0.0), float(err[sel].max()))


@pytest.mark.parametrize("dim", [1, 2, 3, 5])
def test_posenc_dims_and_frequencies(hip_lib, gpu, dim):
    """Every dim with 0, 1, 10 and 30 frequencies, with and without the input columns, 1 and 33 rows.  Bound: the project's 2e-6
    absolute.  The worst error in float32 ulps of the result is printed, separately for |argument| < 8 and above (up to 2^31):
    the figures of an MI355X run are POSENC_ULPS_SMALL / POSENC_ULPS_LARGE below."""
    from nerf import ops
    stats = {}
    for rows in (1, 33):
        x = _posenc_input(rows, dim, 10 * dim + rows)
        for n_freq in (0, 1, 10, 30):
            for include_input in (True, False):
                _posenc_check(gpu, x, n_freq, include_input, stats)
        assert ops.posenc(x.to(gpu), 0, False).shape == (rows, 0)                           # no frequencies, no input: empty, not an error
        with pytest.raises(RuntimeError):
            ops.posenc(x.to(gpu), 31, True)                                                 # 2^31 is no int shift any more: refused
    print(f"posenc dim {dim}: worst error {stats.get('small', 0):.2f} ulp (abs {stats.get('abs_small', 0):.2e}) for |argument| < 8, "
          f"{stats.get('large', 0):.2f} ulp (abs {stats.get('abs_large', 0):.2e}) above")


# worst error of k_posenc in float32 ulps of the float64 result, measured on an MI355X over the cases of this module against the
# float64 reference above (printed by the tests; the asserted bound is the 2e-6 absolute -- the figures are kept so that a regression
# of the range reduction shows; the worst absolute error seen was 6.4e-8):
POSENC_ULPS_SMALL = 1.53          # |argument| < 8   (66,700 x 3 case; 1.34 over the dim / frequency cases)
POSENC_ULPS_LARGE = 1.57          # |argument| >= 8, up to 2^31   (66,700 x 3 case; 1.34 over the dim / frequency cases)


def test_posenc_beyond_one_grid_pass(hip_lib, gpu):
    """66,700 rows x 63 columns = 4,202,100 outputs, more than the 16384 x 256 threads of the launch: the grid-stride loop."""
    assert 66700 * 63 > 16384 * 256
    stats = {}
    _posenc_check(gpu, _posenc_input(66700, 3, 7), 10, True, stats)
    print(f"posenc 66700 x 3, 10 frequencies: worst error {stats['small']:.2f} ulp for |argument| < 8, {stats['large']:.2f} ulp above")


# =====================================================================================================================
# 4. eval post-processing
# =====================================================================================================================
def _f32_neighbours(v):
    v = np.float32(v)
    return [float(np.nextafter(v, np.float32(-10))), float(v), float(np.nextafter(v, np.float32(10)))]


def _eval_inputs(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    rgb = (torch.rand((h, w, 3), generator=g) * 1.2 - 0.1)                                 # some below 0, some above 1
    special = [0.0, 1.0, 1.0 - 2.0 ** -24, -0.0, -0.25, 1.5, 255.5 / 255.0]
    for k in (1, 2, 3, 51, 85, 127, 128, 170, 254, 255):
        special += _f32_neighbours(np.float32(k) / np.float32(255)) + _f32_neighbours(k / 255.0)
    flat = rgb.reshape(-1)
    special = torch.tensor(special, dtype=torch.float32).roll(seed)
    flat[:min(flat.numel(), special.numel())] = special[:flat.numel()]
    depth = torch.rand((h, w), generator=g) * 0.5 + 1.0
    wts = torch.rand((h, w), generator=g)
    wts[torch.rand((h, w), generator=g) < 0.5] *= 0.3                                       # both sides of the 0.22 threshold
    sw = torch.tensor(_f32_neighbours(0.22) + [0.0, 1.0], dtype=torch.float32).roll(seed)
    wts.reshape(-1)[:min(h * w, sw.numel())] = sw[:h * w]
    return rgb, depth, wts


def _normal_map_ieee_sqrt(depth, weights):
    """oracle.normal_map with torch.sqrt, inside it, replaced by the correctly rounded square root (numpy's).  torch's CPU sqrt is a
    vector-library routine that differs from the correctly rounded value by an ulp in 0.6 % of its results (6,922 of the 1,047,522
    lengths of the 1030 x 1019 case), and which results those are depends on the library and the CPU; the kernel rounds correctly.
    An ulp there survives the truncation to a byte about once in 100,000 values, so the bytes rarely show it -- but they may."""
    ieee = lambda t: torch.from_numpy(np.sqrt(t.numpy()))
    keep = torch.sqrt
    torch.sqrt = ieee
    try:
        return O.normal_map(depth, O.INTRINSICS, weights)
    finally:
        torch.sqrt = keep


@pytest.mark.parametrize("h,w", [(5, 37), (37, 5), (2, 2), (1, 7), (7, 1), (1, 1), (1030, 1019)])
def test_eval_postprocess_shapes_and_values(hip_lib, gpu, h, w):
    """Non-square images (rows and columns, cx and cy, the stride of the (H-1, W-1) normal map cannot be exchanged unnoticed), rows
    or columns of length 1 (an empty normal map, colours still right), more pixels than one grid pass (1030 x 1019 > 4096 x 256),
    colours at the byte boundaries k/255 and their float neighbours, weights at the 0.22 threshold: byte-exact against the oracle's
    cast_to_u8 / normal_map (its square root correctly rounded, see _normal_map_ieee_sqrt), with weights, without, and colours only.
    (The 1030 x 1019 case found the cross product rounded otherwise than torch rounds it: 37 bytes with weights and 87 without
    differed by 1 on an MI355X until k_eval_postprocess formed it as fma(a1, b2, -(a2 * b1)).)"""
    from nerf import ops
    assert (h, w) != (1030, 1019) or h * w > 4096 * 256
    rgb, depth, wts = _eval_inputs(h, w, h + w)
    want_u8 = O.cast_to_u8(rgb)
    for weights in (wts, None):
        u8, nrm = ops.eval_postprocess(rgb.to(gpu), depth.to(gpu), None if weights is None else weights.to(gpu), O.INTRINSICS)
        assert u8.dtype == torch.uint8 and torch.equal(u8.cpu(), want_u8)
        want_n = _normal_map_ieee_sqrt(depth, weights)
        assert nrm.dtype == torch.uint8 and tuple(nrm.shape) == tuple(want_n.shape) == (h - 1, w - 1, 3)
        assert torch.equal(nrm.cpu(), want_n), int((nrm.cpu() != want_n).sum())
    u8, nrm = ops.eval_postprocess(rgb.to(gpu), depth.to(gpu), wts.to(gpu), O.INTRINSICS, want_normals=False)
    assert nrm is None and torch.equal(u8.cpu(), want_u8)
    u8, nrm = ops.eval_postprocess(rgb.to(gpu))
    assert nrm is None and torch.equal(u8.cpu(), want_u8)


def test_eval_postprocess_value_cases_are_present():
    """The value cases of the test above are what they claim: the colours hold exact byte boundaries whose neighbours truncate to
    different bytes, and the weights hold 0.22f and both of its neighbours."""
    rgb, _, wts = _eval_inputs(5, 37, 42)
    u8 = O.cast_to_u8(rgb).reshape(-1)
    flat = rgb.reshape(-1)
    k = (np.float32(128) / np.float32(255))
    below = float(np.nextafter(k, np.float32(0)))
    at = {float(v): int(b) for v, b in zip(flat.tolist(), u8.tolist())}
    assert at[float(k)] == 128 and at[below] == 127
    assert at[1.0] == 255 and at[1.0 - 2.0 ** -24] == 254 and at[0.0] == 0 and at[-0.25] == 0 and at[1.5] == 255
    w = wts.reshape(-1)
    t = float(np.float32(0.22))
    assert int((w == t).sum()) >= 1 and int((w > t).sum()) > 10 and int((w < t).sum()) > 10
    assert float(np.nextafter(np.float32(0.22), np.float32(1))) in w.tolist() and float(np.nextafter(np.float32(0.22), np.float32(0))) in w.tolist()
