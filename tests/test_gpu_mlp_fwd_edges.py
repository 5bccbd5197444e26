"""The fused NeRFace MLP forwards of all five model classes, every inference and training entry, per element at every point-count edge,
on buffers the test owns.  GPU only.

The C entry points are called through MLPFamily.fn / MLPFamily.call as nerf.ops.mlp_fwd and nerf.ops.mlp_fwd_train call them, with `raw`
(4 n floats) and `saved` (<prefix>_saved_floats(n) floats) filled with a quiet NaN of a recognisable payload (tests/test_gpu_density.py's
0x7FC0BEEF: an unwritten element is told from a NaN the kernel computed) and GUARD floats of GUARD_BITS behind each; the library is told
the TRUE sizes and the guards are checked after every call.  tests/mlp_fwd_edges_ref.py is the host model: the point counts on both
sides of a 16-point tile, a 32-point wave and a 128-point workgroup as (rays x samples), the inputs, the five networks in fp64 behind the
float32 point, the gates, and the table of what each `saved` layout never writes.

One test per (family, entry) walks the counts:
  raw      no element unwritten; every element within the arithmetic's existing gate of fp64 per channel (scale: the channel's largest
           magnitude in the reference, below 128 points the 737-point case's); torch's float32 evaluation under half the f32 gate;
           training forward == inference forward bit for bit; the first k points of a 300-point launch == a launch of k points;
           rd_view = rd.clone() == NULL bit for bit, another rd_view (x, y NaN) == fp64 with that direction input; the exact-f32
           inference entries also around one and two laps of the persistent grid, against fp64 on the device
  saved    exactly the elements of the never-written table still hold the poison; every section of rows [0, n) against the reference's
           `acts`: PE 2e-6 (test_posenc's; the raw point bit for bit, the pad slot 0), hidden sections under the gate of raw per unit,
           post-ReLU sections without a negative value or a -0.0, direction slots of the split forwards == the exact-f32 forward's
           bitwise; the ReLU decisions (f32: saved > 0 and the kernel's own mask words; split: the bit masks) == the reference's wherever
           its pre-activation lies outside the gate's band, the share left out at most 0.5 % per layer and case
One test per (family, backward) feeds a poisoned and a zero-filled `saved` of the same training forward to poisoned_bwd
(tests/test_gpu_dw_plans.py), for a dense d_raw and one that is zero except at the first and last row and the last row of every 16-,
32- and 128-point unit: every gradient finite and bit-equal between the two, ops.split_saved_to_f32 of the two bit-equal and finite on
rows [0, n) -- nothing downstream reads what the forward leaves unwritten.

MEASURED on an MI355X (256 CUs), largest error over all counts next to the gate it was held to.  raw: f32 and f16x3 colours 2e-7 .. 9e-7
(gate 2.1e-5 .. 5.7e-5), density 1.7e-6 .. 4.4e-5 (6.8e-5 .. 9.5e-4); bf16x3 colours 4e-6 .. 1e-5 (2.9e-5 .. 5.5e-4), density 1.9e-5 ..
3.4e-4 (7.1e-4 .. 1.4e-2); f16x2 colours 1.8e-4 .. 5.4e-4 (1e-3), density 9.7e-4 .. 2.0e-2 (1.7e-3 .. 4.7e-2); the persistent grid at
32767, 32768, 32769 and 65569 points 2e-7 .. 1.1e-6 / 2.2e-6 .. 5.3e-5.  saved: PE 9.0e-8 and direction slots 9.1e-8 (2e-6); hidden
sections per unit f32 and f16x3 7.5e-8 .. 6.9e-7 (2.1e-5 .. 4.7e-5), bf16x3 4.2e-7 .. 8.6e-6 (1.0e-5 .. 2.3e-4).  ReLU decisions left out:
at most 3.9e-3 of a layer (one unit of 256 at one point; cap 5e-3).  The never-written table held as written at every count."""
import functools

import pytest
import torch

from tests import mlp_fwd_edges_ref as R
from tests import test_gpu_dw_plans as DW
from tests.test_gpu_backward import bit_masks
from tests.test_gpu_density import NAN_PAYLOAD, _model
from tests.test_gpu_dw_plans import GUARD, GUARD_BITS, poisoned_bwd
from tests.test_gpu_tiny_edges import bits_equal, guard_untouched

pytestmark = pytest.mark.gpu
DEVICE = "cuda:0"
# the two blendshape classes run the second family's backward with their own gradient scatter (csrc/nf_mlp_bshape.h), which writes every
# slot: poisoned_bwd's table of gradient slots that are never written has no entry for them yet, and none is needed
for _prefix in ("nf_bshape", "nf_cbshape"):
    DW.NEVER_WRITTEN.setdefault(_prefix, ())
SPLIT_ARG = {"f32": False, "bf16x3": True, "f16x3": "f16"}


# ---------------------------------------------------------------------------------------------------------------- plumbing
def poisoned(n, dev, fill=NAN_PAYLOAD):
    """n floats of the poison (or of `fill` bits) with GUARD floats of GUARD_BITS behind them."""
    buf = torch.empty(n + GUARD, dtype=torch.int32, device=dev)
    buf[:n].fill_(fill)
    buf[n:].fill_(GUARD_BITS)
    return buf.view(torch.float32)


def unwritten(t):
    return t.view(torch.int32) == NAN_PAYLOAD


def tailed(t, dev):
    """`t` on the device with GUARD floats of the poison behind it: an input read past its end (the point of a partial tile's padding
    lane that is not clamped to n - 1, a d_raw row past n) is a NaN, not whatever the allocator left there."""
    buf = poisoned(t.numel() + GUARD, dev)
    buf[:t.numel()].copy_(t.reshape(-1))
    return buf[:t.numel()].view(t.shape)


def ranges_of(mask, limit=6):
    """A boolean vector's runs of True as 'lo:hi' strings, for an assertion's message."""
    idx = mask.nonzero().reshape(-1)
    if idx.numel() == 0:
        return []
    brk = (idx[1:] != idx[:-1] + 1).nonzero().reshape(-1) + 1
    lo = torch.cat((idx[:1], idx[brk])).tolist()
    hi = torch.cat((idx[brk - 1], idx[-1:])).tolist()
    return [f"{a}:{b + 1}" for a, b in zip(lo, hi)][:limit] + (["..."] if len(lo) > limit else [])


@functools.lru_cache(maxsize=None)
def _family(kind):
    """-> (MLPFamily, MLPWeights, per-call bias table): the model of tests/test_gpu_density.py, its parameters checked against the
    host model's."""
    from nerf import ops
    from oracle import nerface_oracle as O
    dev = torch.device(DEVICE)
    m, expr, latent = _model(kind, dev)
    p = R.model_params(kind)
    sd = m.state_dict()
    assert list(sd) == list(p) and all(torch.equal(sd[k].cpu(), p[k]) for k in p), kind
    for k, v in sd.items():
        if k.endswith(".bias"):
            assert float(v.abs().min()) > 0, (kind, k)               # a zero bias would hide a dropped one
    e0, l0 = R.conditioning()
    assert torch.equal(expr.cpu(), e0) and torch.equal(latent.cpu(), l0)
    fam, hw = m.FAMILY, m.hip_weights()
    assert fam.prefix == R.PREFIX[kind] and fam.precisions == R.ARITHMETICS[kind]
    return fam, hw, ops.mlp_condition(fam, hw.get(), expr, latent, O.NEAR, O.FAR)


def _image(hw, arith):
    return {"f32": hw.get, "bf16x3": hw.get_bf16, "f16x3": hw.get_f16, "f16x2": hw.get_f16}[arith]()


def run_entry(kind, entry, arith, train, ro, rd, z, rd_view=None, saved_fill=NAN_PAYLOAD):
    """<prefix>_<entry> on poisoned buffers -> (raw (n, 4), the whole `saved` buffer or None); the guards are checked."""
    from nerf import _hip as H
    fam, hw, cond = _family(kind)
    dev = ro.device
    n_rays, n_samples = z.shape
    n = n_rays * n_samples
    raw = poisoned(4 * n, dev)
    n_saved = fam.fn("saved_floats")(n)
    assert n_saved == R.saved_floats(kind, n)
    saved = poisoned(n_saved, dev, saved_fill) if train else None
    args = (H.ptr(_image(hw, arith)), H.ptr(cond), H.ptr(ro), H.ptr(rd), H.ptr(rd_view), H.ptr(z), n_rays, n_samples, H.ptr(raw))
    with torch.cuda.device(dev):
        if train:
            fam.call(entry, *args, H.ptr(saved), H.stream_ptr(dev))
        else:
            fam.call(entry, *args, H.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    assert guard_untouched(raw, 4 * n), (kind, entry, n, "the forward wrote behind raw")
    assert saved is None or guard_untouched(saved, n_saved), (kind, entry, n, "the forward wrote behind saved")
    return raw[:4 * n].view(n, 4), None if saved is None else saved[:n_saved]


@functools.lru_cache(maxsize=None)
def _case(kind, n_rays, n_samples):
    """One (model, size): the inputs on the device, the fp64 reference (computed once on the device, never modified), what its gates
    are relative to, torch's float32 evaluation, and the direction slots the exact-f32 training forward saves."""
    dev = torch.device(DEVICE)
    cpu_in = R.inputs(kind, n_rays, n_samples)
    ro, rd, z = (tailed(t, dev) for t in cpu_in)
    ref = R.forward64(kind, ro, rd, z)
    n = n_rays * n_samples
    sc = R.scales(ref) if n >= 128 else _case(kind, *R.SCALE_CASE)["sc"]
    err32 = (R.forward32(kind, ro, rd, z).double() - ref["raw"]).abs().amax(dim=0)
    assert bool((err32 <= 0.5 * R.raw_gate("f32", sc)).all()), (kind, n, err32.tolist(), R.raw_gate("f32", sc).tolist())
    _, saved = run_entry(kind, "mlp_fwd_train", "f32", True, ro, rd, z)
    off = R.layout(kind)["sections"]["dirf"][0]
    return dict(ro=ro, rd=rd, z=z, ref=ref, sc=sc, n=n, err32=err32, dirf32=saved[off * n:(off + 16) * n].view(n, 16).clone())


class Worst:
    """The largest error / gate seen per name, with the error and the gate it was seen at."""

    def __init__(self):
        self.w = {}

    def add(self, name, err, gate):
        ratio = err / gate
        k = int(ratio.reshape(-1).argmax()) if ratio.numel() > 1 else 0
        r, e, g = float(ratio.reshape(-1)[k]), float(err.reshape(-1)[k]), float(gate.reshape(-1)[k] if gate.numel() > 1 else gate)
        if name not in self.w or r > self.w[name][0]:
            self.w[name] = (r, e, g)

    def line(self):
        return ", ".join(f"{k} {e:.2e} ({g:.2e})" for k, (_, e, g) in self.w.items())


def check_raw(tag, raw, ref, gate, worst):
    """Nothing of raw[:n] unwritten; every element inside its channel's gate."""
    assert not bool(unwritten(raw).any()), (tag, "raw elements unwritten", ranges_of(unwritten(raw).reshape(-1)))
    err = (raw.double() - ref["raw"]).abs().amax(dim=0)
    for c, name in enumerate(("r", "g", "b", "sigma")):
        worst.add("raw." + name, err[c], gate[c])
    assert bool((err <= gate).all()), (tag, "raw", err.tolist(), gate.tolist())


def f32_tile_masks(saved, kind, n):
    """The exact-f32 kernels' own mask words ([layer][16-point tile][64 lanes][2 dwords]; bit 4 no + r of lane (g, c) <-> feature
    16 no + 4 g + r of point 16 tile + c: csrc/nf_mlp_dev.h) -> one boolean (n, width) matrix per ReLU layer."""
    lay = R.layout(kind)
    tiles = (n + 15) // 16
    words = saved[lay["mask_off"] * n:lay["mask_off"] * n + 128 * len(lay["relu"]) * tiles].view(torch.int32).view(len(lay["relu"]), tiles, 4, 16, 2)
    out = []
    for l, name in enumerate(lay["relu"]):
        width = lay["sections"][name][1]
        m = torch.zeros((tiles, 16, width), dtype=torch.bool, device=saved.device)        # (tile, c, feature)
        for no in range(width // 16):
            w = words[l, :, :, :, no >> 3]                                                 # (tile, g, c)
            for r in range(4):
                bit = ((w >> (4 * (no & 7) + r)) & 1).bool()
                for g in range(4):
                    m[:, :, 16 * no + 4 * g + r] = bit[:, g, :]
        out.append(m.reshape(tiles * 16, width)[:n])
    return out


def check_saved(tag, kind, arith, c, saved, worst, shares):
    """`saved` of one training forward: the never-written table, then every section of rows [0, n) against the reference."""
    from nerf import ops
    n, ref, sc, lay = c["n"], c["ref"], c["sc"], R.layout(kind)
    # what the forward leaves unwritten: exactly the table
    want = torch.zeros(saved.numel(), dtype=torch.bool, device=saved.device)
    for lo, hi, _ in R.never_written(kind, arith, n):
        want[lo:hi] = True
    got = unwritten(saved)
    assert not bool((got & ~want).any()), (tag, "unwritten elements outside the never-written table", ranges_of(got & ~want))
    assert not bool((want & ~got).any()), (tag, "the never-written table names elements that are written", ranges_of(want & ~got))
    sv = saved if arith == "f32" else ops.split_saved_to_f32(saved, n, f16=arith == "f16x3", family="paper" if kind == "paper" else "lcode")
    sec = lambda k: sv[lay["sections"][k][0] * n:(lay["sections"][k][0] + lay["sections"][k][1]) * n].view(n, lay["sections"][k][1])
    rows = sv[:(lay["mask_off"] + (0 if arith == "f32" else 8 * len(lay["relu"]))) * n]
    assert not bool(unwritten(rows).any()) and bool(torch.isfinite(rows[:lay["mask_off"] * n]).all()), (tag, "rows [0, n) of saved")
    if arith != "f32" and n % 32:
        # the hidden sections are fragment streams over pad32(n) points: the padding points hold copies of point n - 1 (the clamp of the
        # split forward's input read), which the converter shows when it is asked for pad32(n) points of the same buffer
        p = R.pad32(n)
        assert R.saved_floats(kind, p) == saved.numel()
        full = ops.split_saved_to_f32(saved, p, f16=arith == "f16x3", family="paper" if kind == "paper" else "lcode")
        for k in lay["acts"]:
            off, w = lay["sections"][k]
            r = full[off * p:(off + w) * p].view(p, w)
            assert bits_equal(r[:n], sec(k)), (tag, k)
            assert bits_equal(r[n:], r[n - 1:n].expand(p - n, w)), (tag, k, "a padding point of the fragment stream is not a copy of point n - 1")
    # PE: slot order, the raw point bit for bit, the pad slot 0
    pe = sec("pe")
    e_pe = (pe.double() - R.pe_in_slot_order(ref)).abs().max()
    worst.add("pe", e_pe, torch.tensor(R.PE_GATE))
    assert float(e_pe) <= R.PE_GATE, (tag, "pe", float(e_pe))
    assert bits_equal(pe[:, 60:63], ref["pts32"]), (tag, "PE slots 60..62 are not the float32 point")
    assert bool((pe[:, 63].view(torch.int32) == 0).all()), (tag, "PE pad slot")
    # direction slots: (sin, cos, 0, 0)(rd_z 2^g); the split forwards' equal the exact-f32 forward's bitwise
    dirf = sec("dirf")
    e_dir = (dirf.double() - R.dir_slots(ref)).abs().max()
    worst.add("dirf", e_dir, torch.tensor(R.PE_GATE))
    assert float(e_dir) <= R.PE_GATE and bool((dirf.view(n, 4, 4)[:, :, 2:].view(torch.int32) == 0).all()), (tag, "dirf", float(e_dir))
    assert bits_equal(dirf, c["dirf32"]), (tag, "direction slots differ from the exact-f32 forward's")
    # hidden sections per unit; post-ReLU sections; the ReLU decisions
    if arith == "f32":
        decisions = dict(zip(lay["relu"], f32_tile_masks(saved, kind, n)))
    else:
        decisions = dict(zip(lay["relu"], bit_masks(sv, n, lay["mask_off"], [lay["sections"][k][1] for k in lay["relu"]])))
    for k in lay["acts"]:
        got_k, a = sec(k), ref["act"][k]
        g_k = R.gate(arith, sc["act"][k])
        e_k = (got_k.double() - a).abs().amax(dim=0)
        worst.add(k, e_k, g_k)
        assert bool((e_k <= g_k).all()), (tag, k, float((e_k / g_k).max()), int((e_k / g_k).argmax()))
        if k not in lay["relu"]:
            continue
        assert not bool((got_k.view(torch.int32) < 0).any()), (tag, k, "a negative value or -0.0 behind a ReLU")
        zk = ref["pre"][k]
        outside = zk.abs() > R.gate(arith, sc["pre"][k])
        share = 1.0 - float(outside.double().mean())
        shares[k] = max(shares.get(k, 0.0), share)
        assert share <= R.BAND_CAP, (tag, k, share)
        assert bool(((decisions[k] == (zk > 0)) | ~outside).all()), (tag, k, "ReLU decision differs from the reference outside the band")
        if arith == "f32":                          # the sign of the saved activation and the mask word the chain reads say the same
            assert torch.equal(decisions[k], got_k > 0), (tag, k, "mask words differ from saved > 0")
        else:                                       # a positive pair has its bit (a bit without one: an activation below the pair's underflow)
            assert not bool(((got_k > 0) & ~decisions[k]).any()), (tag, k, "a positive activation without its mask bit")
            assert bool((((got_k > 0) == (zk > 0)) | ~outside).all()), (tag, k, "sign of the saved activation differs outside the band")


# ---------------------------------------------------------------------------------------------------------------- forward
IDS = [f"{k}-{e}" for k, e, _, _ in R.PAIRS]


@pytest.mark.parametrize("kind,entry,arith,train", R.PAIRS, ids=IDS)
def test_forward_at_point_count_edges(hip_lib, gpu, kind, entry, arith, train):
    import nerf
    try:
        _forward_at_point_count_edges(gpu, kind, entry, arith, train)
    finally:
        nerf.set_mlp_precision("f32")


def _forward_at_point_count_edges(gpu, kind, entry, arith, train):
    worst, shares = Worst(), {}
    head = f"mlp-fwd-edges {kind} {entry}"
    for n_rays, s in R.COUNTS:
        c = _case(kind, n_rays, s)
        tag = f"{head} {n_rays}x{s}={c['n']}"
        raw, saved = run_entry(kind, entry, arith, train, c["ro"], c["rd"], c["z"])
        check_raw(tag, raw, c["ref"], R.raw_gate(arith, c["sc"]), worst)
        if train:                                   # one forward, two routes: the inference entry of the arithmetic returns the same bits
            raw_inf, _ = run_entry(kind, R.INFERENCE_ENTRY[arith], arith, False, c["ro"], c["rd"], c["z"])
            assert bits_equal(raw_inf, raw), (tag, "inference and training forward differ")
            check_saved(tag, kind, arith, c, saved, worst, shares)
    # the first k points of a larger launch equal a launch of those k points alone
    ro, rd, z = (tailed(t, gpu) for t in R.inputs(kind, R.PREFIX_LAUNCH, 1))
    big, _ = run_entry(kind, entry, arith, train, ro, rd, z)
    assert not bool(unwritten(big).any())
    for k in R.PREFIX_KS:
        part, _ = run_entry(kind, entry, arith, train, ro[:k].contiguous(), rd[:k].contiguous(), z[:k].contiguous())
        assert bits_equal(part, big[:k]), (head, f"the first {k} points of {R.PREFIX_LAUNCH} differ from a launch of {k}")
    # rd_view: a copy of rd is NULL bit for bit; another one reaches the result through its z-component alone
    c = _case(kind, *R.RD_VIEW_CASE)
    base, _ = run_entry(kind, entry, arith, train, c["ro"], c["rd"], c["z"])
    same, _ = run_entry(kind, entry, arith, train, c["ro"], c["rd"], c["z"], rd_view=tailed(c["rd"], gpu))
    assert bits_equal(same, base), (head, "rd_view = rd.clone() differs from NULL")
    rv = tailed(R.other_view(c["rd"]), gpu)
    other, sv_other = run_entry(kind, entry, arith, train, c["ro"], c["rd"], c["z"], rd_view=rv)
    ref_v = R.forward64(kind, c["ro"], c["rd"], c["z"], rd_view=rv)
    w_view = Worst()
    check_raw(head + " rd_view", other, ref_v, R.raw_gate(arith, c["sc"]), w_view)
    assert not bits_equal(other[:, :3], base[:, :3]) and bits_equal(other[:, 3], base[:, 3])     # the colours moved, the density did not
    if train:
        off = R.layout(kind)["sections"]["dirf"][0]
        nn = c["n"] if arith == "f32" else R.pad32(c["n"])
        dirf = sv_other[off * nn:off * nn + 16 * c["n"]].view(c["n"], 16)
        assert float((dirf.double() - R.dir_slots(ref_v)).abs().max()) <= R.PE_GATE, (head, "direction slots under rd_view")
    lines = [f"{head}: largest error (its gate) over {len(R.COUNTS)} counts: {worst.line()}; rd_view: {w_view.line()}"]
    if train:
        lines.append(f"{head}: largest share of a layer's ReLU decisions left out "
                     f"{max(shares.values()):.2e} ({max(shares, key=shares.get)}) (cap {R.BAND_CAP:g})")
    # the persistent grid of the exact-f32 inference kernels: one point below, at and above a lap, and a partial block on the second lap
    if entry == "mlp_fwd":
        counts = R.grid_counts(torch.cuda.get_device_properties(gpu).multi_processor_count)
        ro, rd, z = (tailed(t, gpu) for t in R.grid_inputs(kind, counts[-1]))
        ref = R.forward64(kind, ro, rd, z)
        w_grid = Worst()
        for n in counts:
            raw, _ = run_entry(kind, entry, arith, False, ro[:n].contiguous(), rd[:n].contiguous(), z[:n].contiguous())
            part = {"raw": ref["raw"][:n]}
            check_raw(f"{head} grid {n}", raw, part, R.gate("f32", part["raw"].abs().amax(dim=0)), w_grid)
        lines.append(f"{head}: persistent grid at {counts} points: {w_grid.line()}")
    print("\n".join(lines))


# ---------------------------------------------------------------------------------------------------------------- backward
BWD = [(k, a, False) for k in R.KINDS for a in R.ARITHMETICS[k] if a != "f16x2"] + [("paper", "bf16x3", True)]


@pytest.mark.parametrize("kind,arith,exact_dw", BWD, ids=[f"{k}-{a}{'-exact_dw' if x else ''}" for k, a, x in BWD])
def test_nothing_downstream_reads_what_the_forward_leaves_unwritten(hip_lib, gpu, kind, arith, exact_dw):
    import nerf
    try:
        _nothing_downstream(gpu, kind, arith, exact_dw)
    finally:
        nerf.set_mlp_precision("f32")


def _nothing_downstream(gpu, kind, arith, exact_dw):
    from nerf import ops
    fam, hw, cond = _family(kind)
    entry = {"f32": "mlp_fwd_train", "bf16x3": "mlp_fwd_train_bf16", "f16x3": "mlp_fwd_train_f16"}[arith]
    lay = R.layout(kind)
    done = []
    for n_rays, s in R.BWD_COUNTS:
        c = _case(kind, n_rays, s)
        n = c["n"]
        tag = f"mlp-fwd-edges bwd {kind} {arith}{'+exact_dw' if exact_dw else ''} {n_rays}x{s}={n}"
        raw_p, saved_p = run_entry(kind, entry, arith, True, c["ro"], c["rd"], c["z"])
        raw_z, saved_z = run_entry(kind, entry, arith, True, c["ro"], c["rd"], c["z"], saved_fill=0)
        assert bits_equal(raw_p, raw_z)
        n_poison = int(unwritten(saved_p).sum())
        assert n_poison == sum(hi - lo for lo, hi, _ in R.never_written(kind, arith, n)) and not bool(unwritten(saved_z).any())
        if arith != "f32":
            f16 = arith == "f16x3"
            family = "paper" if kind == "paper" else "lcode"
            rows = (lay["mask_off"] + 8 * len(lay["relu"])) * n
            a, b = (ops.split_saved_to_f32(sv, n, f16=f16, family=family)[:rows] for sv in (saved_p, saved_z))
            assert bits_equal(a, b), (tag, "split_saved_to_f32 read an element the forward never wrote")
            assert bool(torch.isfinite(a[:lay["mask_off"] * n]).all()) and not bool(unwritten(a).any()), tag
        g = torch.Generator().manual_seed(7000 + n)
        dense = tailed(torch.randn((n_rays, s, 4), generator=g), gpu)
        hot = R.hot_rows(n)
        d_hot = torch.zeros((n, 4))
        d_hot[torch.tensor(hot)] = torch.randn((len(hot), 4), generator=g)
        for name, d_raw in (("dense", dense), (f"hot({len(hot)})", tailed(d_hot.view(n_rays, s, 4), gpu))):
            res = [poisoned_bwd(fam, hw, hw.get(), cond, c["z"], d_raw, sv, split=SPLIT_ARG[arith], exact_dw=exact_dw) for sv in (saved_p, saved_z)]
            (gp, lp), (gz, lz) = res                                   # (poisoned_bwd asserts every gradient element written and finite)
            assert bool(torch.isfinite(lp).all()) and bits_equal(lp, lz), (tag, name, "d_latent")
            live = 0
            for i, (x, y) in enumerate(zip(gp, gz)):
                assert (x is None) == (y is None), (tag, name, i)
                if x is not None:
                    assert bool(torch.isfinite(x).all()) and bits_equal(x, y), (tag, name, fam.keys[i], "differs between a poisoned and a zero-filled saved")
                    live += int(float(x.abs().max()) > 0)
            assert live > 0, (tag, name)                                # (the gradients are not all zero: the comparison says something)
        done.append(f"{n} ({n_poison} poisoned floats)")
    print(f"mlp-fwd-edges bwd {kind} {arith}{'+exact_dw' if exact_dw else ''}: gradients of a poisoned and a zero-filled saved bit-equal at " + ", ".join(done))
