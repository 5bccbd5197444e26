"""The packed weight images read back per element: the exact-f32 fragment image, the split-bf16 streams and the scaled split-fp16 streams
with their tails, of the paper and the second family (forward and transposed), against tests/split_stream_ref.py.  GPU only.

The pack entry points are called as nerf.ops.MLPWeights._get calls them, on a buffer the test owns: exactly the reported size, filled
with 0xA5, GUARD_BYTES of 0x5A behind it that every call must leave alone.  Weight sets: `survey` (init_*_params(boost="survey"), what
the forward tests use), `wide` (every weight times 2^u, u in [-28, 0]: `lo` parts in fp16's normal, subnormal and zero ranges),
`planted maxima` (one element at 4 x the layer's largest |w| in every position class of k_stream_absmax, every layer, every stream:
only that layer's scale, inverse scale and maximum move) and `extremes` (an all-zero layer, the two clamps of the layer scale, inf and
NaN among the weights).  Every comparison is bit for bit; the one forward at the end holds test_f16x3_raw_outputs_meet_the_f32_gate's
gate.

MEASURED on an MI355X.  Everything was bit for bit, the subnormal `lo` parts of `wide` included (paper forward: 229210 normal, 186570
subnormal, 93148 zero, where `survey` has 492357 normal, 251 subnormal and 16320 zero, zero codes included; the build keeps fp16
subnormals).  Position classes (spans: paper forward 1988 entries, transposed 1840, second
family 1280 and 1200): every stream has every class; first, last, before-first-boundary, before-last-boundary and remainder exist in
every layer; a straddling workgroup in every layer but the first (second family forward: layers 1, 3, 4, 5, 7); no live entry at or
after the last boundary where a layer ends in zero codes (paper forward layer 7, transposed 0 and 3, second family forward 6,
transposed 0 and 2), none at or after the first in the paper's transposed layer 0.  75 / 64 / 54 / 38 planted packs; the whole stream
re-checked at the before-last-boundary plant of layers 1 / 4 / 1 / 3.  Forward with a planted maximum: colours 8e-8 .. 4.5e-7 (gate
2.1e-5 .. 5.6e-5), density 1.1e-6 and 1.2e-6 (5.1e-5, 3.7e-5), range flag 0.  Sensitivity, on scratch builds: k_stream_absmax
dropping each span's last entry fails the planted maxima of all four streams and nothing else here; `15 - k` in nf_f16_layer_scale
fails the survey tails, the planted maxima and the forward.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from oracle import cases as C
from oracle import nerface_oracle as O
from tests import smaller_ref as S
from tests import split_stream_ref as R
from tests import util as U
from tests.test_gpu_lcode import lmodel

pytestmark = pytest.mark.gpu
GUARD_BYTES = 4096
FILL, GUARD_FILL = 0xA5, 0x5A
STREAM_NAMES = tuple(R.STREAMS)


@functools.lru_cache(maxsize=None)
def survey(prefix):
    """-> (MLPFamily, parameter names in ABI order, the survey parameters as a list of CPU tensors in that order)."""
    from nerf import ops
    if prefix == "nf_paper":
        fam, p = ops.PAPER, O.init_paper_params(3, boost="survey")
    elif prefix == "nf_lcode":
        fam, p = ops.LCODE, O.init_lcode_params(6, boost="survey")
    else:
        fam, p = ops.SMALLER, S.init_smaller_params(14)
    assert set(fam.keys) == set(p)
    return fam, list(fam.keys), [p[k].clone() for k in fam.keys]


def wide(params, seed=77):
    """Every weight matrix times 2^u elementwise, u uniform integers in [-28, 0]."""
    g = torch.Generator().manual_seed(seed)
    return [p * torch.exp2(-torch.randint(0, 29, p.shape, generator=g).float()) if p.dim() == 2 else p.clone() for p in params]


class Packer:
    """The device copies of one family's parameters and one owned, guarded buffer per image kind."""

    def __init__(self, prefix, gpu):
        self.fam, self.keys, base = survey(prefix)
        self.gpu = gpu
        self.dev = [p.to(gpu).contiguous() for p in base]
        self.arr = (ctypes.c_void_p * len(self.dev))(*[int(p.data_ptr()) for p in self.dev])
        self.buf = {}

    def load(self, params):
        for d, p in zip(self.dev, params):
            d.copy_(p)

    def poke(self, tid, offset, value):
        self.dev[tid].view(-1)[offset] = value

    def pack(self, kind, fresh=True):
        """<prefix>_<pack entry>(params, buffer, stream) -> the buffer (uint8, on the device) without its guard."""
        from nerf import _hip as H
        from nerf.ops import MLPWeights
        size_fn, pack_fn, dtype = MLPWeights._KINDS[kind]
        size = self.fam.fn(size_fn)() * (4 if dtype == torch.float32 else 1)
        if kind not in self.buf:
            self.buf[kind] = torch.empty(size + GUARD_BYTES, dtype=torch.uint8, device=self.gpu)
            self.buf[kind][size:].fill_(GUARD_FILL)
            fresh = True
        buf = self.buf[kind]
        if fresh:
            buf[:size].fill_(FILL)
        with torch.cuda.device(self.gpu):
            self.fam.call(pack_fn, self.arr, H.ptr(buf), H.stream_ptr(self.gpu))
        torch.cuda.synchronize(self.gpu)
        assert bool((buf[size:] == GUARD_FILL).all()), (self.fam.prefix, kind, "the pack wrote behind its image")
        return buf[:size]


@functools.lru_cache(maxsize=None)
def packer(prefix):
    return Packer(prefix, torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def table_of(name):
    from nerf import _hip as H
    return R.stream_table(H.lib(), name)


def first_diff(got, want):
    bad = (got != want).nonzero().reshape(-1)
    return None if bad.numel() == 0 else (int(bad.numel()), int(bad[0]), int(got[bad[0]]) & 0xFFFF, int(want[bad[0]]) & 0xFFFF)


def check_stream(tag, image, name, kind, params):
    """The whole image of one stream against the reference: every 16-bit element, and for fp16 all 64 tail words."""
    tab, off = table_of(name), R.pair_offsets(name)
    img = image.cpu()
    assert img.numel() == R.image_bytes(name, kind), tag
    hi, lo = R.unpack(img, tab)
    if kind.startswith("bf16"):
        whi, wlo = R.expected_bf16(params, tab)
    else:
        whi, wlo, wtail, _ = R.expected_f16(params, tab, off, R.STREAMS[name]["act_scale"])
        tail = img[R.stream_bytes(name):].view(torch.int32)
        assert torch.equal(tail, wtail), (tag, "tail", tail.tolist(), wtail.tolist())
        assert int(tail[R.F16_FLAG_WORD]) == 0
    assert first_diff(hi, whi) is None, (tag, "hi: (count, first entry, got, want)", first_diff(hi, whi))
    d = first_diff(lo, wlo)
    if d is not None:                                   # a mismatch confined to subnormal lo values would mean the build flushes them
        bad = lo != wlo
        sub = (wlo[bad].view(torch.float16).float().abs() < 2.0 ** -14) if kind.startswith("f16") else None
        assert False, (tag, "lo: (count, first entry, got, want)", d, "all subnormal in the reference" if sub is not None and bool(sub.all()) else "")
    return lo.view(torch.float16) if kind.startswith("f16") else None


def _kinds():
    return [(n, k) for n in STREAM_NAMES for k in R.STREAMS[n]["kinds"]]


@pytest.mark.parametrize("name,kind", _kinds(), ids=[f"{n}-{k}" for n, k in _kinds()])
def test_survey_and_wide_images_bit_for_bit(hip_lib, gpu, name, kind):
    """Every element of the stream, hi and lo, == the reference; fp16: the three tail arrays, the flag word and the zeroed rest."""
    pk = packer(R.STREAMS[name]["prefix"])
    _, _, base = survey(pk.fam.prefix)
    for label, params in (("survey", base), ("wide", wide(base))):
        pk.load(params)
        lo = check_stream(f"{name} {kind} {label}", pk.pack(kind), name, kind, params)
        if lo is not None:
            a = lo.float().abs()
            n_sub, n_zero = int(((a > 0) & (a < 2.0 ** -14)).sum()), int((a == 0).sum())
            print(f"{name} {kind} {label}: bit-equal; lo parts {int((a >= 2.0 ** -14).sum())} normal, {n_sub} subnormal, {n_zero} zero")
            assert label != "wide" or (n_sub > 1000 and n_zero > 1000)          # the set reaches fp16's subnormals and zeros
    pk.load(base)


@pytest.mark.parametrize("prefix", ["nf_paper", "nf_smaller"])
def test_f32_image_is_the_gathered_parameters(hip_lib, gpu, prefix):
    """k_pack_f32: every element of the exact-f32 image bit-equal to the parameter its gather-table code names, +0.0 at a zero code."""
    pk = packer(prefix)
    _, _, base = survey(prefix)
    n = pk.fam.fn("packed_floats")()
    tab = np.zeros(n, dtype=np.uint32)
    assert getattr(hip_lib, f"{prefix}_gather_table")(tab.ctypes.data_as(ctypes.c_void_p), n) == 0
    for label, params in (("survey", base), ("wide", wide(base))):
        pk.load(params)
        got = pk.pack("f32").cpu().view(torch.int32)
        want = R.gather(params, tab).view(torch.int32)
        assert got.numel() == n and torch.equal(got, want), (prefix, label, first_diff(got, want))
        print(f"{prefix} f32 {label}: {n} elements bit-equal, {int((tab >> 24 == 0xFF).sum())} zero codes")
    pk.load(base)


def _tail(image, name):
    return image[R.stream_bytes(name):].cpu().view(torch.int32)


def f16_kind(name):
    return R.STREAMS[name]["kinds"][1]


@pytest.mark.parametrize("name", STREAM_NAMES)
def test_planted_maxima_move_their_layers_scale_only(hip_lib, gpu, name):
    """For every layer and position class of k_stream_absmax: survey with the ONE parameter element behind that entry at 4 x (odd
    classes: -4 x) the layer's largest |w|.  The tail follows the plant in that layer and in no other; for one plant per stream the
    whole stream is checked as well."""
    pk = packer(R.STREAMS[name]["prefix"])
    _, _, base = survey(pk.fam.prefix)
    kind, tab, off, act = f16_kind(name), table_of(name), R.pair_offsets(name), R.STREAMS[name]["act_scale"]
    ids, offs = R.split_codes(tab)
    amax0 = R.layer_amax(R.gather(base, tab), off)
    pk.load(base)
    assert torch.equal(_tail(pk.pack(kind), name), R.f16_tail(amax0, act))
    packs, full, have = 0, None, {c: [] for c in R.CLASSES}
    for l in range(R.STREAMS[name]["NL"]):
        pos = R.absmax_positions(tab, off, l)
        by_entry = {}
        for i, (cls, e) in enumerate(pos.items()):
            if e is not None:
                have[cls].append(l)
                by_entry.setdefault(e, (cls, i))
        for e, (cls, i) in by_entry.items():
            tid, o = int(ids[e]), int(offs[e])
            old = float(base[tid].view(-1)[o])
            plant = float(np.float32(4.0 * amax0[l])) * (-1.0 if i % 2 else 1.0)
            pk.poke(tid, o, plant)
            amax = list(amax0)
            amax[l] = abs(plant)
            assert R.layer_scale(amax[l]) == R.layer_scale(amax0[l]) / 4.0
            image = pk.pack(kind, fresh=False)
            got, want = _tail(image, name), R.f16_tail(amax, act)
            assert torch.equal(got, want), (name, "layer", l, cls, "entry", e, got[:3 * len(amax)].tolist(), want[:3 * len(amax)].tolist())
            packs += 1
            if full is None and cls == "before_last_boundary" and R.STREAMS[name]["KS"][l] * R.STREAMS[name]["NO"][l] >= 128:
                params = [p.clone() for p in base]
                params[tid].view(-1)[o] = plant
                check_stream(f"{name} {kind} planted layer {l} {cls}", image, name, kind, params)
                full = (l, cls, e)
            pk.poke(tid, o, old)
    assert full is not None
    assert torch.equal(_tail(pk.pack(kind, fresh=False), name), R.f16_tail(amax0, act))           # every plant taken back
    print(f"{name}: {packs} planted packs; whole stream checked at {full}; layers per class: " + ", ".join(f"{c} {v}" for c, v in have.items()))


@pytest.mark.parametrize("name", STREAM_NAMES)
def test_extreme_layers(hip_lib, gpu, name):
    """An all-zero layer (s = 1, zeros, maximum bits 0), a layer whose largest |w| is 2^-40 (clamp e = 40) and one whose largest is
    1.5 x 2^39 (clamp e = -24, every hi finite), a layer holding +inf and a NaN (scale from the largest finite element; the two
    entries hold what the conversion gives: hi = +inf / NaN, lo = NaN; every other entry == the reference)."""
    pk = packer(R.STREAMS[name]["prefix"])
    _, _, base = survey(pk.fam.prefix)
    kind, tab, off, nl = f16_kind(name), table_of(name), R.pair_offsets(name), R.STREAMS[name]["NL"]
    ids, offs = R.split_codes(tab)

    def tensors_of(l):
        lo, hi = R.layer_entries(off, l)
        return sorted(set(np.unique(ids[lo:hi]).tolist()) - {0xFF})

    def live_entry(l, k):
        lo, hi = R.layer_entries(off, l)
        return int(lo + np.flatnonzero(ids[lo:hi] != 0xFF)[k])

    def run(l, params):
        pk.load(params)
        image = pk.pack(kind)
        tail = _tail(image, name)
        lo, hi = R.layer_entries(off, l)
        return image, tail.view(torch.float32), tail, slice(lo, hi)

    # all zeros
    l = 1
    params = [p.clone() for p in base]
    for t in tensors_of(l):
        params[t].zero_()
    image, tf, ti, rng = run(l, params)
    check_stream(f"{name} zeros", image, name, kind, params)
    hi, lo = R.unpack(image.cpu(), tab)
    assert float(tf[l]) == R.STREAMS[name]["act_scale"] and float(tf[nl + l]) == 1.0 and int(ti[2 * nl + l]) == 0
    assert not bool(hi[rng].any()) and not bool(lo[rng].any())
    # largest |w| = 2^-40: e = 14 + 39 = 53 clamps to 40
    l = 2
    params = [p.clone() for p in base]
    for t in tensors_of(l):
        params[t].mul_(2.0 ** -45)
    e = live_entry(l, 5)
    params[int(ids[e])].view(-1)[int(offs[e])] = 2.0 ** -40
    image, tf, ti, rng = run(l, params)
    check_stream(f"{name} tiny", image, name, kind, params)
    assert float(tf[nl + l]) == 2.0 ** -40 and int(ti[2 * nl + l]) == int(np.float32(2.0 ** -40).view(np.int32))
    assert float(R.unpack(image.cpu(), tab)[0][e].view(torch.float16)) == 1.0                    # 2^-40 x 2^40
    # largest |w| = 1.5 x 2^39: e = 14 - 40 = -26 clamps to -24, 1.5 x 2^15 is finite in fp16
    l = nl - 1
    params = [p.clone() for p in base]
    e = live_entry(l, -3)
    params[int(ids[e])].view(-1)[int(offs[e])] = -1.5 * 2.0 ** 39
    image, tf, ti, rng = run(l, params)
    check_stream(f"{name} huge", image, name, kind, params)
    hi, _ = R.unpack(image.cpu(), tab)
    assert float(tf[nl + l]) == 2.0 ** 24 and bool(torch.isfinite(hi[rng].view(torch.float16).float()).all())
    assert float(hi[e].view(torch.float16)) == -1.5 * 2.0 ** 15
    # +inf and NaN: skipped by the maximum
    l = 0
    params = [p.clone() for p in base]
    e_inf, e_nan = live_entry(l, 3), live_entry(l, -7)
    params[int(ids[e_inf])].view(-1)[int(offs[e_inf])] = float("inf")
    params[int(ids[e_nan])].view(-1)[int(offs[e_nan])] = float("nan")
    image, tf, ti, rng = run(l, params)
    hi, lo = R.unpack(image.cpu(), tab)
    whi, wlo, wtail, amax = R.expected_f16(params, tab, off, R.STREAMS[name]["act_scale"])
    assert math.isfinite(amax[l]) and amax[l] > 0 and torch.equal(ti, wtail)
    others = torch.ones(len(tab), dtype=torch.bool)
    others[[e_inf, e_nan]] = False
    assert torch.equal(hi[others], whi[others]) and torch.equal(lo[others], wlo[others])
    f = lambda t, i: float(t[i].view(torch.float16))
    assert f(hi, e_inf) == float("inf") and math.isnan(f(lo, e_inf)) and math.isnan(f(hi, e_nan)) and math.isnan(f(lo, e_nan))
    pk.load(base)
    print(f"{name}: zeros / 2^-40 / 1.5 x 2^39 / inf + NaN layers as the reference")


@pytest.mark.parametrize("name", STREAM_NAMES)
def test_repack_clears_the_flag_and_takes_no_stale_maximum(hip_lib, gpu, name):
    """Flag word set to 1 and the maxima to 0xFFFFFFFF by hand, then survey x 2^-3 packed into the SAME buffer: flag 0, the smaller
    weights' scales, the whole image == the reference."""
    pk = packer(R.STREAMS[name]["prefix"])
    _, _, base = survey(pk.fam.prefix)
    kind, nl = f16_kind(name), R.STREAMS[name]["NL"]
    pk.load(base)
    image = pk.pack(kind)
    before = _tail(image, name).clone()
    words = image[R.stream_bytes(name):].view(torch.int32)
    words[R.F16_FLAG_WORD] = 1
    words[2 * nl:3 * nl] = -1
    small = [p * 0.125 for p in base]
    pk.load(small)
    image = pk.pack(kind, fresh=False)
    after = _tail(image, name)
    assert int(after[R.F16_FLAG_WORD]) == 0
    check_stream(f"{name} repack", image, name, kind, small)
    assert torch.equal(after.view(torch.float32)[:nl], before.view(torch.float32)[:nl] * 8.0)
    pk.load(base)


@pytest.mark.parametrize("prefix", ["nf_paper", "nf_lcode"])
def test_forward_with_a_planted_maximum_meets_the_f32_gate(hip_lib, gpu, prefix):
    """mlp_fwd in f16x3 on 35 points (5 x 7) of a model whose widest hidden layer carries a planted maximum at a span boundary, against
    the float64 network on the same weights: 2e-5 scale + 2e-5 per channel (test_f16x3_raw_outputs_meet_the_f32_gate's gate); the
    range flag stays 0."""
    import nerf
    from nerf import ops
    name = "paper_fwd" if prefix == "nf_paper" else "lcode_fwd"
    fam, keys, base = survey(prefix)
    tab, off = table_of(name), R.pair_offsets(name)
    ids, offs = R.split_codes(tab)
    sizes = [k * n for k, n in zip(R.STREAMS[name]["KS"], R.STREAMS[name]["NO"])]
    l = sizes.index(max(sizes))
    e = R.absmax_positions(tab, off, l)["after_first_boundary"]
    amax = R.layer_amax(R.gather(base, tab), off)
    p = {k: v.clone() for k, v in zip(keys, base)}
    p[keys[int(ids[e])]].view(-1)[int(offs[e])] = 4.0 * amax[l]
    c = C.build_case("eval_det_64_128")
    ro, rd, _, _, _ = C.ray_subset(512, 512, 3, 5, 5)
    z = torch.sort(torch.rand((5, 7), generator=torch.Generator().manual_seed(5)) * 0.6 + 0.2, dim=-1)[0]
    m = (U.make_model if prefix == "nf_paper" else lmodel)(nerf, p, gpu)
    hw = m.hip_weights()
    cond = ops.mlp_condition(fam, hw.get(), c["expr"].to(gpu), c["latent"].to(gpu), O.NEAR, O.FAR)
    raw = ops.mlp_fwd(fam, "f16x3", hw.get_f16(), cond, ro.to(gpu), rd.to(gpu), z.to(gpu)).cpu().reshape(-1, 4)
    got_tail = hw.get_f16()[R.stream_bytes(name):].cpu().view(torch.int32)
    amax[l] *= 4.0
    assert torch.equal(got_tail, R.f16_tail(amax, 16.0))
    mlp = O.paper_mlp if prefix == "nf_paper" else O.lcode_mlp
    ref = mlp({k: v.double() for k, v in p.items()}, O.encode_points(ro.double(), rd.double(), z.double(), O.NEAR, O.FAR),
              c["expr"].double(), c["latent"].double())
    err, scale = (raw.double() - ref).abs().amax(dim=0), ref.abs().amax(dim=0)
    gate = 2e-5 * scale + 2e-5
    print(f"{prefix} f16x3 planted layer {l} entry {e}: max|err| {['%.2e' % v for v in err.tolist()]}  [gate {['%.2e' % v for v in gate.tolist()]}]")
    assert bool((err <= gate).all())
    assert int(hw.f16_range_flag()) == 0
