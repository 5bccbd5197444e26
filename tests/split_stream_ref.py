"""Host model of the split-precision weight streams (csrc/nf_pack.h, csrc/nf_mlp_split_table.h) and the shared inputs of the
gradient-scale tests.  NumPy / torch on the CPU; tests/test_split_stream_host.py checks it against the sources and the library's
host exports, tests/test_gpu_split_streams.py and tests/test_gpu_grad_scales.py hold the device kernels to it.

A stream is a run of (hi, lo) 1-KiB block pairs, 512 16-bit elements per block, ordered by layer: layer l owns the pairs
[off[l], off[l + 1]), off[l] = sum_{i < l} KS[i] NO[i].  Entry e of the stream's gather table (tensor id << 24 | element offset,
0xFF000000 = zero) is the element at position e & 511 of pair e >> 9.  The fp16 streams carry a 256-byte tail of 64 dwords behind
the blocks: [NL] bias scales s act_scale | [NL] 1 / s | [NL] bits of the layer's largest finite non-zero |w| | zeros, dword 48 the
forward kernel's range flag."""
import ctypes
import functools
import math

import numpy as np
import torch

ZERO_CODE = 0xFF000000
BLOCK = 512                             # 16-bit elements per block; a pair is two blocks
F16_TAIL_BYTES = 256
F16_FLAG_WORD = 48
SCALE_E_MIN, SCALE_E_MAX, SCALE_TOP = -24, 40, 14          # nf_f16_layer_scale: e = clamp(14 - k, -24, 40)
ABSMAX_GRID, ABSMAX_BLOCK, ABSMAX_UNROLL = 256, 256, 4     # k_stream_absmax as nf_pack_split_f16 launches it

# the four layer tables: the source that states them, its table export, and what the stream serves
STREAMS = {
    "paper_fwd": dict(prefix="nf_paper", src="nf_mlp_bf16_common.h", table="nf_paper_stream_table_bf16", kinds=("bf16", "f16"), act_scale=16.0,
                      NL=11, KS=(4, 16, 16, 20, 16, 16, 16, 18, 8, 8, 8), NO=(8, 8, 8, 8, 8, 8, 8, 5, 4, 4, 1)),
    "paper_bwd": dict(prefix="nf_paper", src="nf_mlp_bf16_bwd.hip", table="nf_paper_stream_table_bwd_bf16", kinds=("bf16_t", "f16_t"), act_scale=1.0,
                      NL=10, KS=(2, 8, 8, 10, 16, 16, 16, 16, 16, 16), NO=(4, 4, 4, 8, 8, 8, 8, 8, 8, 8)),
    "lcode_fwd": dict(prefix="nf_lcode", src="nf_mlp_lcode_bf16_common.h", table="nf_lcode_stream_table_bf16", kinds=("bf16", "f16"), act_scale=16.0,
                      NL=8, KS=(4, 16, 16, 16, 16, 16, 18, 8), NO=(8, 8, 8, 8, 1, 8, 4, 1)),
    "lcode_bwd": dict(prefix="nf_lcode", src="nf_mlp_lcode_bf16_bwd.hip", table="nf_lcode_stream_table_bwd_bf16", kinds=("bf16_t", "f16_t"), act_scale=1.0,
                      NL=6, KS=(2, 8, 18, 16, 16, 16), NO=(4, 8, 8, 8, 8, 8)),
}
# size entry points per image kind (names after the family prefix), as nerf.ops.MLPWeights._KINDS
SIZE_FN = {"bf16": "packed_bf16_bytes", "bf16_t": "packed_bwd_bf16_bytes", "f16": "packed_f16_bytes", "f16_t": "packed_bwd_f16_bytes"}
CLASSES = ("first", "last", "after_first_boundary", "before_first_boundary", "after_last_boundary", "before_last_boundary", "remainder",
           "straddle")


def stream_table(hip_lib, name):
    """The gather table of stream `name` from the library's host export (uint32 codes, one per entry)."""
    fn = getattr(hip_lib, STREAMS[name]["table"])
    n = fn(None, 0)
    assert n > 0
    tab = np.zeros(n, dtype=np.uint32)
    assert fn(tab.ctypes.data_as(ctypes.c_void_p), n) == n
    return tab


def pair_offsets(name):
    s = STREAMS[name]
    off = [0]
    for ks, no in zip(s["KS"], s["NO"]):
        off.append(off[-1] + ks * no)
    return off


def n_pairs(name):
    return pair_offsets(name)[-1]


def n_entries(name):
    return n_pairs(name) * BLOCK


def stream_bytes(name):
    return n_pairs(name) * 2 * BLOCK * 2


def image_bytes(name, kind):
    return stream_bytes(name) + (F16_TAIL_BYTES if kind.startswith("f16") else 0)


def flag_offset(name):
    return stream_bytes(name) + 4 * F16_FLAG_WORD


def layer_entries(off, l):
    """[lo, hi): the table entries of layer l."""
    return off[l] * BLOCK, off[l + 1] * BLOCK


def split_codes(table):
    table = np.asarray(table, dtype=np.uint32)
    return (table >> 24).astype(np.int64), (table & 0xFFFFFF).astype(np.int64)


def gather(params, table):
    """The parameter element behind every table entry (float32), 0.0 at a zero code.  params: the family's tensors in ABI order."""
    ids, offs = split_codes(table)
    w = torch.zeros(len(ids), dtype=torch.float32)
    for tid in np.unique(ids):
        if tid == 0xFF:
            continue
        sel = torch.from_numpy(ids == tid)
        w[sel] = params[int(tid)].detach().reshape(-1).float()[torch.from_numpy(offs[ids == tid])]
    return w


def unpack(stream_bytes_, table):
    """stream_bytes_: the image's bytes (uint8, CPU); -> (hi, lo) per table entry as int16 bit patterns."""
    e = np.arange(len(table), dtype=np.int64)
    at = (2 * (e >> 9)) * BLOCK + (e & 511)
    el = stream_bytes_[:len(table) * 4].contiguous().view(torch.int16)
    at = torch.from_numpy(at)
    return el[at], el[at + BLOCK]


def expected_bf16(params, table):
    """(hi, lo) bit patterns per entry: hi = bf16_rn(w), lo = bf16_rn(w - hi)."""
    w = gather(params, table)
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return hi.view(torch.int16), lo.view(torch.int16)


def layer_scale(amax):
    """nf_f16_layer_scale: 2^clamp(14 - k, -24, 40) with amax = m 2^k, m in [0.5, 1); 1 for amax == 0."""
    if not amax > 0.0:
        return 1.0
    _, k = math.frexp(amax)
    return math.ldexp(1.0, min(max(SCALE_TOP - k, SCALE_E_MIN), SCALE_E_MAX))


def layer_amax(w, off):
    """Per layer the largest finite non-zero |w| among its entries (0.0 where there is none), as float32 values."""
    out = []
    for l in range(len(off) - 1):
        lo, hi = layer_entries(off, l)
        a = w[lo:hi].abs()
        a = a[torch.isfinite(a) & (a > 0)]
        out.append(float(a.max()) if a.numel() else 0.0)
    return out


def split_f16(ws):
    """The reference split of scaled float32 values: hi = f16_rn(ws), lo = f16_rn(ws - hi), in float32 then .to(float16)."""
    hi = ws.to(torch.float16)
    lo = (ws - hi.float()).to(torch.float16)
    return hi, lo


def f16_tail(amax, act_scale):
    """The 64 tail words (int32) of a freshly packed fp16 stream whose layers' largest |w| are `amax`."""
    scales = np.array([layer_scale(a) for a in amax], dtype=np.float32)
    nl = len(amax)
    tail = np.zeros(F16_TAIL_BYTES // 4, dtype=np.int32)
    tail[:nl] = (scales * np.float32(act_scale)).view(np.int32)
    tail[nl:2 * nl] = (np.float32(1.0) / scales).view(np.int32)
    tail[2 * nl:3 * nl] = np.array(amax, dtype=np.float32).view(np.int32)
    return torch.from_numpy(tail)


def expected_f16(params, table, off, act_scale):
    """-> (hi bits, lo bits, tail as 64 int32 words, per-layer amax)."""
    w = gather(params, table)
    amax = layer_amax(w, off)
    s_entry = torch.ones_like(w)
    for l, a in enumerate(amax):
        lo, hi = layer_entries(off, l)
        s_entry[lo:hi] = layer_scale(a)
    hi, lo = split_f16(w * s_entry)
    return hi.view(torch.int16), lo.view(torch.int16), f16_tail(amax, act_scale), amax


def absmax_span(n):
    return (n + ABSMAX_GRID - 1) // ABSMAX_GRID


def in_remainder_loop(e, n):
    """Does the thread of k_stream_absmax that reads entry e reach it in the remainder loop (not in the four-at-a-time loop)?"""
    span = absmax_span(n)
    e0 = e // span * span
    e1 = min(e0 + span, n)
    t, j = (e - e0) % ABSMAX_BLOCK, (e - e0) // ABSMAX_BLOCK
    trips, first = 0, e0 + t
    while first + (ABSMAX_UNROLL - 1) * ABSMAX_BLOCK < e1:              # for (; e + 3 * blockDim.x < e1; e += 4 * blockDim.x)
        trips += 1
        first += ABSMAX_UNROLL * ABSMAX_BLOCK
    return j >= ABSMAX_UNROLL * trips


def absmax_positions(table, off, l):
    """The live entries of layer l in each position class of k_stream_absmax (CLASSES): {class: entry, or None where the layer has
    none}.  A span boundary is a multiple of span strictly inside the layer's entry range."""
    table = np.asarray(table, dtype=np.uint32)
    n = len(table)
    span = absmax_span(n)
    lo, hi = layer_entries(off, l)
    live = lo + np.flatnonzero((table[lo:hi] >> 24) != 0xFF)
    out = dict.fromkeys(CLASSES)
    if live.size == 0:
        return out
    out["first"], out["last"] = int(live[0]), int(live[-1])

    def at_or_after(b, end=hi):
        i = np.searchsorted(live, b)
        return int(live[i]) if i < live.size and live[i] < end else None

    def before(b):
        i = np.searchsorted(live, b)
        return int(live[i - 1]) if i > 0 else None

    bounds = [b for b in range((lo // span + 1) * span, hi, span)]
    if bounds:
        out["after_first_boundary"], out["before_first_boundary"] = at_or_after(bounds[0]), before(bounds[0])
        out["after_last_boundary"], out["before_last_boundary"] = at_or_after(bounds[-1]), before(bounds[-1])
    rem = [int(e) for e in live if in_remainder_loop(int(e), n)]
    out["remainder"] = rem[len(rem) // 2] if rem else None
    if lo % span:                                                       # the workgroup that holds `lo` began in the layer before
        out["straddle"] = at_or_after(lo, min((lo // span + 1) * span, hi))
    return out


# ---------------------------------------------------------------------------------------- inputs of the gradient-scale tests
GRAD_SIZES = {259: (7, 37), 21: (3, 7)}
EQUIVARIANCE_K = (-40, -14, 14, 40)
# The paper model's smallest per-point per-layer max |dZ| on the 259-point input is 2^-10.9 (fp64 oracle), so its fp16 chain clamps a
# point's scale below k = -36.1: k = -40 leaves the set for that chain (tests/test_split_stream_host.py) and -32 stands in for it.
# The second family keeps -40 on a THIN margin: its smallest maximum is 2^-6.3, unclamped down to k = -40.7, and that figure is the
# oracle's with true ReLUs where the device uses the masks its forward saved.  Inputs and seeds are fixed, so the case is
# deterministic; after a change of either, an equivariance failure of that family at k = -40 alone means a clamped point, not a
# bookkeeping bug -- run the host test first and move the family to a larger k if its range no longer holds -40.
F16_EQUIVARIANCE_K = {"nf_paper": (-32, -14, 14, 40), "nf_lcode": EQUIVARIANCE_K}


def equivariance_k(prefix, mode):
    return F16_EQUIVARIANCE_K[prefix] if mode == "f16" else EQUIVARIANCE_K


def grad_family_params(prefix):
    """-> (parameters, expression, latent, fp64 network) of the paper model or the second family as tests/test_gpu_dw_plans.py's
    `_family` serves them (restated: that function needs a device; tests/test_gpu_grad_scales.py checks the two agree)."""
    from oracle import cases as C
    from oracle import nerface_oracle as O
    c = C.build_case("train_rand_64_64")
    if prefix == "nf_paper":
        return c["p_fine"], c["expr"], c["latent"], O.paper_mlp
    return O.init_lcode_params(6), c["expr"], c["latent"], O.lcode_mlp


SPREAD_K = -24                                  # the per-point spread's smallest rows: 2^-24
CHAIN_UNCLAMPED = (2.0 ** -47, 2.0 ** 73)      # nfb_pow2_scale does not clamp a maximum inside [2^-47, 2^73)


@functools.lru_cache(maxsize=None)
def grad_inputs(n):
    """-> (ro, rd, z, B): the rays, depths and the dense N(0, 1) upstream gradient of the n-point case (CPU, float32)."""
    from oracle import cases as C
    n_rays, n_samples = GRAD_SIZES[n]
    ro, rd, _, _, _ = C.ray_subset(512, 512, 9, n_rays, 29)
    g = torch.Generator().manual_seed(1000 + n)
    z = torch.sort(torch.rand((n_rays, n_samples), generator=g) * 0.6 + 0.2, dim=-1)[0]
    b = torch.randn((n_rays, n_samples, 4), generator=g)
    return ro, rd, z, b


def spread_exponents(n):
    """e_i = -8 (i mod 4): four magnitudes down to 2^-24 inside every 32-point tile."""
    return -8 * (torch.arange(n) % 4)


def per_point_dz_maxima(mlp, params, x64, expr, latent, d_raw64):
    """The fp64 oracle backward: per layer the per-point largest |dZ| (pre-activation gradient), the rgb gradient's first."""
    pp = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    acts = []
    out = mlp(pp, x64, expr.double(), latent.double(), acts=acts)
    for a in acts:
        a.retain_grad()
    out.backward(d_raw64)
    maxima = [d_raw64[:, :3].abs().amax(dim=1)]
    for a in acts:
        dz = a.grad if bool((a.detach() < 0).any()) else a.grad * (a.detach() > 0)          # no ReLU behind a section with negative values
        maxima.append(dz.abs().amax(dim=1))
    return maxima
