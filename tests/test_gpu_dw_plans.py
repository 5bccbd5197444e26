"""The backward of the fused MLP families at every edge of its two slice plans (tests/dw_plan_ref.py is their host model), with
the workspace and the gradient image POISONED before the call.  GPU only.

The weight-gradient GEMMs write one slab of partial sums per point slice and k_grad_reduce sums the slabs; the slabs are not
zero-filled, so correctness rests on every slab element the reduction reads having been written -- also where a group runs fewer
slices than the longest one (NfReduceAlt), where the last slice holds a single row, and at 2, 3, 4, 5 slabs (every tail of the
reduction).  nerf.ops.mlp_bwd allocates with torch.empty, where a slot that is read unwritten usually holds the previous call's value
for it -- close to the right answer in a test that repeats similar calls.  Here such a slot holds a NaN, so a failure does not
depend on a tolerance: `poisoned_bwd` mirrors ops.mlp_bwd call for call on NaN-filled buffers with guard tails behind them, and its
result must equal ops.mlp_bwd's bit for bit (the reduction order is fixed).  The numbers themselves are held to the project's
existing per-tensor gates against fp64 autograd of the oracle, evaluated on the device at the ReLU masks the HIP forward saved,
for a dense upstream gradient and for one that is zero except at the rows where a slice, a 16-row chunk, a wave tile or a
workgroup begins or ends.

Not reached: the zero-fill fallback of nf_bwd_run (nf_dw_reduce_alt returning false) -- no current group table produces a plan with
two distinct short slice counts or a short group whose outputs are not whole rows (tests/test_dw_plan_host.py checks the former)."""
import functools

import pytest
import torch

from oracle import cases as C
from oracle import nerface_oracle as O
from tests import dw_plan_ref as P
from tests import smaller_ref as S
from tests import util as U
from tests.test_gpu_backward import TRAIN_SIZE_GATE, bit_masks, f32_rows, relu_masks
from tests.test_gpu_lcode import LC_MASK_OFF, LC_RELU, LC_SAVED, lmodel
from tests.test_gpu_smaller import SM_RELU, SM_SAVED, smodel

pytestmark = pytest.mark.gpu

GUARD = 1024
GUARD_BITS = 0x5A5A5A5A                 # as a float 1.5e16: finite, not a NaN, and nothing a kernel would write
SPLIT_ARG = {"f32": False, "bf16": True, "f16": "f16"}
# per-tensor rel-L2 gates against the masked fp64 oracle, the ones the project already holds these kernels to: the paper model's
# TRAIN_SIZE_GATE (test_training_kernels_vs_fp64_at_training_size), test_lcode_mlp_bwd_vs_fp64_oracle's 1e-4 / 3e-4 (bf16x3) and
# test_smaller_mlp_bwd_vs_fp64_restatement's 1e-4.  exact_dw (split-bf16 forward and dX chain, exact-f32 dW GEMMs) carries the
# split-bf16 gate: its dZ is the split chain's.
GATE = {"nf_paper": dict(TRAIN_SIZE_GATE), "nf_lcode": {"f32": 1e-4, "f16": 1e-4, "bf16": 3e-4}, "nf_smaller": {"f32": 1e-4}}
# gradient slots a family's unpack kernel never writes (they would still hold the poison).  None today: the paper model's
# layers_dir.3 pair, which autograd leaves None, is written as 0.0 (nf_paper_net_grad_unpack).
NEVER_WRITTEN = {"nf_paper": (), "nf_lcode": (), "nf_smaller": ()}
# (parameter prefix, index of its ReLU mask) of every layer behind a ReLU: rows of dW / db of a unit that is masked off are exact zeros
RELU_LAYERS = {"nf_paper": [(f"layers_xyz.{i}", i) for i in range(6)] + [(f"layers_dir.{i}", 6 + i) for i in range(3)],
               "nf_smaller": [(f"layers_xyz.{i}", i) for i in range(5)] + [(f"layers_dir.{i}", 5 + i) for i in range(3)],
               "nf_lcode": [(f"layers_xyz.{i}", i) for i in range(3)] + [("fc_feat", 3), ("layers_dir.0", 4)]}
MAX_POINTS = 44032


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def poisoned_bwd(fam, weights, packed, cond, z, d_raw, saved_t, split=False, exact_dw=False):
    """nerf.ops.mlp_bwd on poisoned buffers: the same entry points and argument order; workspace and gradient image are filled with
    quiet NaNs and carry a 1024-float guard tail each, the library is told the TRUE workspace size.  Asserts the guards untouched
    and every gradient element written and finite; returns (grads, d_latent) like ops.mlp_bwd."""
    from nerf import _hip as H
    from nerf import ops
    d_raw = d_raw.contiguous()
    dev = H.require_device(packed, cond, saved_t, d_raw)
    n_rays, n_samples = z.shape
    with torch.cuda.device(dev):
        ws_floats = fam.fn("bwd_workspace_floats")(n_rays * n_samples)          # (after any monkeypatched NERFACE_DW_SLICES)
    grad_floats = fam.fn("grad_floats")()
    ws = torch.empty(ws_floats + GUARD, dtype=torch.float32, device=dev)
    flat = torch.empty(grad_floats + GUARD, dtype=torch.float32, device=dev)
    for buf, n in ((ws, ws_floats), (flat, grad_floats)):
        buf[:n].fill_(float("nan"))
        buf[n:].view(torch.int32).fill_(GUARD_BITS)
    args = (H.ptr(cond), H.ptr(saved_t), H.ptr(d_raw), n_rays, n_samples, H.ptr(ws), ws_floats, H.ptr(flat))
    with torch.cuda.device(dev):
        if split == "f16":
            fam.call("mlp_bwd_f16", H.ptr(packed), H.ptr(weights.get_f16_t()), *args, H.stream_ptr(dev))
        elif split:
            packed_bt, exact = weights.get_bf16_t(), ()
            if fam.exact_dw:
                saved_f32 = ops.split_saved_to_f32(saved_t, n_rays * n_samples, False) if exact_dw else None
                exact = (int(bool(exact_dw)), H.ptr(saved_f32))
            fam.call("mlp_bwd_bf16", H.ptr(packed), H.ptr(packed_bt), *args, *exact, H.stream_ptr(dev))
        else:
            fam.call("mlp_bwd", H.ptr(packed), H.ptr(weights.get_t()), *args, H.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    assert bool((ws[ws_floats:].view(torch.int32) == GUARD_BITS).all()), "the backward wrote behind its workspace"
    assert bool((flat[grad_floats:].view(torch.int32) == GUARD_BITS).all()), "the backward wrote behind the gradient image"
    grads, off, live = [], 0, torch.ones(grad_floats, dtype=torch.bool, device=dev)
    for i, p in enumerate(weights._params):
        n = p.numel()
        if i in NEVER_WRITTEN[fam.prefix]:
            assert bool(torch.isnan(flat[off:off + n]).all()), f"slot {i} of {fam.prefix} is documented as never written"
            live[off:off + n] = False
        grads.append(None if i in fam.none_grads else flat[off:off + n].view(p.shape))
        off += n
    assert off + 32 == grad_floats
    bad = (~torch.isfinite(flat[:grad_floats])) & live
    assert not bool(bad.any()), f"{int(bad.sum())} gradient elements unwritten or not finite, first at {int(bad.nonzero()[0])}"
    return grads, flat[off:off + 32]


@functools.lru_cache(maxsize=None)
def _rays():
    ro, rd, _, _, _ = C.ray_subset(512, 512, 9, MAX_POINTS, 29)
    return ro, rd


@functools.lru_cache(maxsize=None)
def _family(prefix):
    """-> (MLPFamily, model on the device, parameters (CPU, f32), parameter names, expression, latent, oracle MLP)."""
    import nerf
    from nerf import ops
    dev = torch.device("cuda:0")
    if prefix == "nf_paper":
        c = C.build_case("train_rand_64_64")
        p = c["p_fine"]
        return ops.PAPER, U.make_model(nerf, p, dev), p, list(ops.PAPER_KEYS), c["expr"], c["latent"], O.paper_mlp
    if prefix == "nf_lcode":
        c = C.build_case("train_rand_64_64")
        p = O.init_lcode_params(6)
        return ops.LCODE, lmodel(nerf, p, dev), p, list(O.LCODE_KEYS), c["expr"], c["latent"], O.lcode_mlp
    c = S.build_case("smaller_soft_train_rand_64_64")
    p = S.init_smaller_params(14)
    return ops.SMALLER, smodel(nerf, p, dev), p, list(S.SMALLER_KEYS), c["expr"], c["latent"], S.smaller_mlp


def _masks(prefix, saved_t, n, mode):
    """The ReLU decisions the training forward saved, in the oracle's order, as boolean (n, width) matrices on the device."""
    from nerf import ops
    if prefix == "nf_paper":
        return relu_masks(f32_rows(saved_t, n, mode), n, mode)
    table, relu = (LC_SAVED, LC_RELU) if prefix == "nf_lcode" else (SM_SAVED, SM_RELU)
    sv = saved_t if mode == "f32" else ops.split_saved_to_f32(saved_t, n, f16=mode == "f16", family="lcode")
    sec = lambda k: sv[table[k][0] * n:(table[k][0] + table[k][1]) * n].view(n, table[k][1])
    signs = [sec(k) > 0 for k in relu]
    if mode == "f32":
        return signs
    # split forwards: the BIT masks are what the chain reads; a positive activation below the (hi, lo) pair's underflow has its bit
    # set and a zero pair.  The decode is checked against the signs: no positive pair without its bit, hardly a bit without one.
    bits = bit_masks(sv, n, LC_MASK_OFF, [table[k][1] for k in relu])
    for b, s in zip(bits, signs):
        assert not bool((s & ~b).any()) and int((b & ~s).sum()) <= 1e-6 * b.numel() + 2
    return bits


def _plans_in_use(prefix, mode, exact_dw, n, n_cu):
    if mode == "f32" or exact_dw:
        plan, _ = P.group_plan(prefix, n, n_cu)
        return sorted({(pps, ns) for _, pps, ns in plan})
    return [P.split_plan(prefix, n)]


def hot_rows(prefix, mode, exact_dw, n, n_cu):
    """Rows at which something begins or ends: points 0 and n - 1, the first and last row of every slice of every distinct plan in
    use, and the two rows either side of the last multiple of 16 (the GEMM's partial chunk), 32 (the chain's wave tile) and 128 (its
    workgroup) below n."""
    rows = {0, n - 1}
    for pps, ns in _plans_in_use(prefix, mode, exact_dw, n, n_cu):
        for a, b in P.slice_rows(n, pps, ns):
            rows.update((a, b))
    for k in (16, 32, 128):
        m = (n - 1) // k * k
        rows.update((m - 1, m))
    return sorted(r for r in rows if 0 <= r < n)


def _oracle(prefix, x64, masks, d_raw64, gpu):
    fam, _, p, keys, expr, latent, mlp = _family(prefix)
    pp = {k: v.to(gpu).double().clone().requires_grad_(True) for k, v in p.items()}
    lat = latent.to(gpu).double().clone().requires_grad_(True)
    out = mlp(pp, x64, expr.to(gpu).double(), lat, masks=masks)
    out.backward(d_raw64)
    ref = {k: pp[k].grad for k in keys}
    ref["latent"] = lat.grad
    return ref


def _compare(tag, prefix, grads, g_lat, ref, gate, per_element):
    _, _, _, keys, _, _, _ = _family(prefix)
    errs, emax = {}, {}
    for k, gh in list(zip(keys, grads)) + [("latent", g_lat)]:
        if gh is None:
            assert ref[k] is None or float(ref[k].abs().max()) == 0.0, k
            continue
        errs[k] = rel_l2(gh, ref[k])
        emax[k] = float((gh.double() - ref[k]).abs().max() / (ref[k].abs().max() + 1e-300))
    wk = max(errs, key=errs.get)
    line = f"dw-plan {tag}: worst rel L2 {errs[wk]:.2e} ({wk}), latent {errs['latent']:.2e}"
    if per_element:
        mk = max(emax, key=emax.get)
        line += f", worst element / max|ref| {emax[mk]:.2e} ({mk})"
    print(line + f"  [gate {gate:g}]")
    for k, v in errs.items():
        assert v < gate, (tag, k, v)
    if per_element:
        for k, v in emax.items():
            assert v <= gate, (tag, k, v)
    return errs


def _setup(prefix, mode, n, gpu):
    """Inputs, training forward and masks of one (family, arithmetic, point count): -> a dict the patterns share."""
    from nerf import ops
    fam, m, p, keys, expr, latent, _ = _family(prefix)
    ro, rd = (t[:n].contiguous().to(gpu) for t in _rays())
    g = torch.Generator().manual_seed(1000 + n)
    z = (torch.rand((n, 1), generator=g) * 0.6 + 0.2).to(gpu)
    hw = m.hip_weights()
    pk = hw.get()
    cond = ops.mlp_condition(fam, pk, expr.to(gpu), latent.to(gpu), O.NEAR, O.FAR)
    _, (saved_t,) = ops.mlp_fwd_train(fam, pk, cond, ro, rd, z, packed_b=hw.get_bf16() if mode == "bf16" else None,
                                      packed_h=hw.get_f16() if mode == "f16" else None)
    masks = _masks(prefix, saved_t, n, mode)
    x64 = O.encode_points(ro.double(), rd.double(), z.double(), O.NEAR, O.FAR)
    return dict(fam=fam, hw=hw, pk=pk, cond=cond, z=z, saved_t=saved_t, masks=masks, x64=x64, g=g)


def _both(st, d_raw, mode, exact_dw):
    """The poisoned backward, and ops.mlp_bwd on the same inputs: bit-identical."""
    from nerf import ops
    kw = dict(split=SPLIT_ARG[mode], exact_dw=exact_dw)
    grads, g_lat = poisoned_bwd(st["fam"], st["hw"], st["pk"], st["cond"], st["z"], d_raw, st["saved_t"], **kw)
    grads_o, g_lat_o = ops.mlp_bwd(st["fam"], st["hw"], st["pk"], st["cond"], st["z"], d_raw, st["saved_t"], **kw)
    assert torch.equal(g_lat, g_lat_o)
    for i, (a, b) in enumerate(zip(grads, grads_o)):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), f"tensor {i} differs from ops.mlp_bwd bit for bit"
    return grads, g_lat


def run_case(gpu, prefix, mode, n, exact_dw=False):
    n_cu = torch.cuda.get_device_properties(gpu).multi_processor_count
    gate = GATE[prefix]["bf16" if exact_dw else mode]
    st = _setup(prefix, mode, n, gpu)
    tag = f"{prefix} {mode}{'+exact_dw' if exact_dw else ''} N={n}"
    # dense: the realistic 1 / (3 N) scale of the training-size tests; a dropped or doubled row moves a tensor by ~ 1 / sqrt(N) >= 5e-3
    d_raw = (torch.randn((n, 1, 4), generator=st["g"]) * (1.0 / (3 * n))).to(gpu)
    grads, g_lat = _both(st, d_raw, mode, exact_dw)
    ref = _oracle(prefix, st["x64"], st["masks"], d_raw.reshape(-1, 4).double(), gpu)
    _compare(tag + " dense", prefix, grads, g_lat, ref, gate, per_element=False)
    del ref, grads, g_lat
    # boundary-hot: zero except at the rows where a slice / chunk / tile begins or ends; the oracle sees those rows only (a point with
    # zero d_raw contributes exactly zero); a hot row skipped, taken twice or paired with another row's activations moves a tensor by per cents
    hot = hot_rows(prefix, mode, exact_dw, n, n_cu)
    assert 2 <= len(hot) <= 160
    idx = torch.tensor(hot, device=gpu)
    d_hot = torch.zeros((n, 1, 4), device=gpu)
    d_hot[idx, 0] = torch.randn((len(hot), 4), generator=st["g"]).to(gpu)
    grads, g_lat = _both(st, d_hot, mode, exact_dw)
    masks_hot = [mk[idx] for mk in st["masks"]]
    ref = _oracle(prefix, st["x64"][idx], masks_hot, d_hot[idx, 0].double(), gpu)
    _compare(tag + f" hot({len(hot)})", prefix, grads, g_lat, ref, gate, per_element=True)
    if mode == "f32":           # exact arithmetic: a unit masked off at every hot point has dZ == 0 there and everywhere else
        _, _, _, keys, _, _, _ = _family(prefix)
        by_key, rows = dict(zip(keys, grads)), 0
        for name, l in RELU_LAYERS[prefix]:
            dead = ~masks_hot[l].any(dim=0)
            rows += int(dead.sum())
            assert float(by_key[name + ".weight"][dead].abs().max() if bool(dead.any()) else 0.0) == 0.0, name
            assert float(by_key[name + ".bias"][dead].abs().max() if bool(dead.any()) else 0.0) == 0.0, name
        print(f"dw-plan {tag} hot: {rows} weight rows of units dead at every hot point are exact zeros")
    del st, ref, grads, g_lat


def _cases():
    """(family, arithmetic, position in dw_plan_ref.edges' list): the point count itself follows the device's CU count."""
    out = []
    for prefix in ("nf_paper", "nf_smaller", "nf_lcode"):
        e = P.edges(prefix, 256)
        out += [(prefix, "f32", False, i) for i in range(len(e["f32"]))]
        for mode in ("bf16", "f16"):
            out += [(prefix, mode, False, i) for i in range(len(e.get("split", ())))]
        out += [(prefix, "bf16", True, i) for i in range(len(e.get("exact_dw", ())))]
    return out


@pytest.mark.parametrize("prefix,mode,exact_dw,k", _cases(),
                         ids=[f"{p}-{m}{'-exact_dw' if x else ''}-edge{k}" for p, m, x, k in _cases()])
def test_backward_at_slice_plan_edges(hip_lib, gpu, prefix, mode, exact_dw, k):
    """One training forward, then the poisoned backward for a dense and a boundary-hot upstream gradient at one edge of the plan in
    use (on 256 CUs: exact f32 paper 1025 2049 3073 4097 15360 15361 15377 30720 30721 30737, smaller 1025 17408 17409 34816 34817,
    second family 1025 4097 43008 43009; split paper 256 257 5888 5889 5905, second family 256 257 8192 8193 8209; paper
    split + exact_dw 15361 30721)."""
    n_cu = torch.cuda.get_device_properties(gpu).multi_processor_count
    e = P.edges(prefix, n_cu)
    ns = e["exact_dw"] if exact_dw else e["f32" if mode == "f32" else "split"]
    if k >= len(ns):            # a CU count at which two edges coincide: the list is shorter and this position is covered by another
        return
    assert ns[k] <= MAX_POINTS
    run_case(gpu, prefix, mode, ns[k], exact_dw)


KNOB_N = 4736


@pytest.mark.parametrize("v", [1, 2, 3, 46])
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_slice_knob(hip_lib, gpu, monkeypatch, mode, v):
    """NERFACE_DW_SLICES (read on every call) = 1, 2, 3, 46 slices wanted at 4736 points, through the poisoned backward: each result
    meets the dense gates against the masked fp64 oracle and agrees with the unset-knob result per tensor -- the slabs are cut
    elsewhere, so partial sums are added in another order, and nothing else differs.  Bound of that agreement: rel-L2 1e-5, or twice
    the exact-f32 backward's own error against fp64 on the same inputs where that is larger (another summation order moves an f32
    sum by about what f32 summation costs it in the first place)."""
    prefix, n = "nf_paper", KNOB_N
    gate = GATE[prefix][mode]
    monkeypatch.delenv("NERFACE_DW_SLICES", raising=False)
    st = _setup(prefix, mode, n, gpu)
    d_raw = (torch.randn((n, 1, 4), generator=st["g"]) * (1.0 / (3 * n))).to(gpu)
    base, base_lat = _both(st, d_raw, mode, False)
    # the f32 backward's own error on these inputs (its own forward and masks)
    st32 = _setup(prefix, "f32", n, gpu)
    g32, l32 = _both(st32, d_raw, "f32", False)
    e32 = _compare(f"{prefix} f32 N={n} dense (knob reference)", prefix, g32, l32,
                   _oracle(prefix, st32["x64"], st32["masks"], d_raw.reshape(-1, 4).double(), gpu), GATE[prefix]["f32"], False)
    ref = _oracle(prefix, st["x64"], st["masks"], d_raw.reshape(-1, 4).double(), gpu)
    monkeypatch.setenv("NERFACE_DW_SLICES", str(v))
    assert P.split_plan(prefix, n) == P.split_plan(prefix, n, target=v)
    grads, g_lat = _both(st, d_raw, mode, False)                      # (the workspace size is asked for with the variable set)
    _compare(f"{prefix} {mode} N={n} dense NERFACE_DW_SLICES={v} {P.split_plan(prefix, n)}", prefix, grads, g_lat, ref, gate, False)
    _, _, _, keys, _, _, _ = _family(prefix)
    diffs = {k: (rel_l2(a, b), max(1e-5, 2 * e32[k])) for k, a, b in list(zip(keys, grads, base)) + [("latent", g_lat, base_lat)]
             if a is not None}
    wk = max(diffs, key=lambda k: diffs[k][0] / diffs[k][1])
    print(f"dw-plan knob {mode} v={v}: vs unset worst {diffs[wk][0]:.2e} at {wk} (bound {diffs[wk][1]:.2e}; "
          f"largest 2 x f32 error {2 * max(e32.values()):.2e})")
    for k, (d, bound) in diffs.items():
        assert d <= bound, (k, d, bound, e32[k])
