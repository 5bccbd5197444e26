"""The specification tests/test_gpu_mlp_fwd_edges.py holds the fused NeRFace MLP forwards to, in plain torch: the five model classes
with the parameters their own GPU tests use, the point counts, the inputs, the network in fp64 with everything the training forward
saves (and every ReLU's pre-activation), the gates per arithmetic, and -- as data, with the source line behind each entry -- which
elements of `saved` each layout never writes.  No GPU and no library: tests/test_mlp_fwd_edges_host.py holds this module against
itself (the gates are ones float32 can meet, the seeds keep the ReLU band small), the GPU test holds the kernels against it.

The reference's inputs: the point ro + rd * z is formed in float32 with a separate multiply and add, as the kernels (nf_add / nf_mul)
and the reference's own input assembly do; everything behind the float32 point -- both encodings and the network -- is fp64."""
from __future__ import annotations

import functools

import torch

from oracle import cases as C
from oracle import nerface_oracle as O
from tests import blendshape_ref as B
from tests import smaller_ref as S
from tests.test_gpu_backward import RELU_ORDER, SAVED
from tests.test_gpu_lcode import LC_MASK_OFF, LC_RELU, LC_SAVED
from tests.test_gpu_smaller import SM_ACTS, SM_RELU, SM_SAVED
from tests.tiny_ref import pe_slot_to_col

KINDS = ("paper", "lcode", "bshape", "cbshape", "smaller")
PREFIX = {k: "nf_" + k for k in KINDS}
ALL = ("f32", "bf16x3", "f16x3", "f16x2")
ARITHMETICS = {"paper": ALL, "lcode": ALL, "bshape": ALL, "cbshape": ALL, "smaller": ("f32",)}
# (entry point after the family prefix, arithmetic, training forward)
ENTRIES = [("mlp_fwd", "f32", False), ("mlp_fwd_bf16", "bf16x3", False), ("mlp_fwd_f16", "f16x3", False), ("mlp_fwd_f16x2", "f16x2", False),
           ("mlp_fwd_train", "f32", True), ("mlp_fwd_train_bf16", "bf16x3", True), ("mlp_fwd_train_f16", "f16x3", True)]
INFERENCE_ENTRY = {a: e for e, a, t in ENTRIES if not t}
PAIRS = [(k, e, a, t) for k in KINDS for e, a, t in ENTRIES if a in ARITHMETICS[k]]

# (rays, samples): ray = p / S with S = 1, S not dividing 32 and S > 32; 16 points are a tile of the exact-f32 kernels, 32 a wave of
# both kernel kinds, 128 a workgroup
COUNTS = [(1, 1), (3, 5), (2, 8), (17, 1), (1, 31), (4, 8), (3, 11), (127, 1), (2, 64), (3, 43), (3, 100), (67, 11)]
SCALE_CASE = (67, 11)               # below 128 points a channel's largest magnitude is noisy: the 737-point case of the model lends its own
RD_VIEW_CASE = (3, 11)
BWD_COUNTS = [(1, 1), (17, 1), (1, 31), (3, 11), (3, 43), (3, 100)]
PREFIX_LAUNCH, PREFIX_KS = 300, (31, 33, 127, 129)      # the first k points of a 300 x 1 launch against a launch of k x 1

PE_GATE = 2e-6                      # test_posenc's
BAND_CAP = 0.005                    # share of a layer's ReLU decisions the comparison may leave out, per layer and case
# seed of a model's inputs (rays and depths).  Chosen so that the reference keeps every layer of every case inside BAND_CAP
# (tests/test_mlp_fwd_edges_host.py asserts it; a seed that breaks the cap is replaced, the cap stays)
SEED = {"paper": 41, "lcode": 42, "bshape": 43, "cbshape": 44, "smaller": 45}

# the f32-row form of `saved` (csrc/nf_mlp_layout.h, nf_mlp_lcode_layout.h, nf_mlp_smaller_layout.h: S_*), from the tests that own the tables:
# sections (offset, width) in floats per point, the order in which the fp64 networks collect `acts`, the sections behind a ReLU in
# the order of the mask words, where the mask words start
LAYOUT = {
    "paper": dict(sections=SAVED, acts=RELU_ORDER[:6] + ["feat"] + RELU_ORDER[6:], relu=RELU_ORDER, mask_off=2256),
    "lcode": dict(sections=LC_SAVED, acts=["l1"] + LC_RELU, relu=LC_RELU, mask_off=LC_MASK_OFF),
    "smaller": dict(sections=SM_SAVED, acts=SM_ACTS, relu=SM_RELU, mask_off=2000),
}
LAYOUT_OF = {"paper": "paper", "lcode": "lcode", "bshape": "lcode", "cbshape": "lcode", "smaller": "smaller"}


def layout(kind):
    return LAYOUT[LAYOUT_OF[kind]]


def pad32(n):
    return (n + 31) & ~31


def saved_floats(kind, n):
    """nf_*_saved_floats: one size for both layouts -- SAVED_PER_POINT pad32(n) + one 16-point tile of mask words per ReLU layer."""
    lay = layout(kind)
    return (lay["mask_off"] + 8 * len(lay["relu"])) * pad32(n) + 128 * len(lay["relu"])


# ---------------------------------------------------------------------------------------------------------------- never written
# What a training forward leaves untouched in its `saved` buffer of saved_floats(n) floats, as half-open float ranges.  With
# M = the mask section's offset per point, L = the ReLU layers, DIRF = the direction slots' offset per point, P = pad32(n):
#
# exact-f32 layout (sections [n][width] at X * n):
#   [M n + 128 L ceil(n / 16), end)   the mask words are kept per 16-point tile, [L][ceil(n / 16)][64 lanes][2 dwords] (nf_mlp_dev.h,
#                                     nf_mask_ptr) and a tile is stored whole when its first point exists (nf_mlp_net_common.h,
#                                     NF_NET_SAVE_PENDING: `if (p0 + 16 * t < n)`); the buffer is sized for the split layout
#                                     (nf_mlp_paper_net.h, nf_paper_net_saved_floats), which is longer.  Every row section is written
#                                     in full: rows >= n fall outside the section's buffer descriptor (nf_mlp_dev.h, nf_slab_copy), the
#                                     PE pad slot is stored as 0.0 (it is part of the PE fragment), the direction slots as (sin, cos, 0, 0).
# split layouts, bf16 and fp16 (sections at X * P):
#   [64 n, 64 P)                      PE rows of the padding points: the stores are predicated on `p_raw < n_points`
#                                     (nf_mlp_split_fwd.inc, pe_step: `if (SAVE && p_raw < n_points)`)
#   [DIRF P + 16 n, DIRF P + 16 P)    direction rows of the padding points: the same predicate (nf_mlp_split_fwd.inc, `float* d = saved + ...`)
#   [M P + 8 L n, end)                the mask words are [L][n][2 lane halves][4 dwords] with n, not P, rows per layer
#                                     (nf_mlp_bf16_machinery.inc, nfb_save_mask: `(layer * n_points + p) * 2 + h`), stored for live
#                                     points only (nf_mlp_split_fwd.inc, NFB_FINISH: `&& live`): 8 L (P - n) floats of padding and
#                                     the 128 L floats sized for the exact-f32 tiles stay.
#   The hidden sections are fragment streams over all P points, written in full: a partial tile's padding points hold copies of point
#   n - 1 (nf_mlp_split_fwd.inc: `p = p_raw < n_points ? p_raw : n_points - 1`), and the stream's descriptor covers P points
#   (nf_mlp_bf16_machinery.inc, nfb_stream_target).
def never_written(kind, arith, n):
    """-> [(lo, hi, what)]: the float ranges of `saved` that still hold the poison after a training forward over n points."""
    lay = layout(kind)
    m, nl, dirf, p = lay["mask_off"], len(lay["relu"]), lay["sections"]["dirf"][0], pad32(n)
    end = saved_floats(kind, n)
    if arith == "f32":
        return [(m * n + 128 * nl * ((n + 15) // 16), end, "mask tiles behind the last one, and the split layout's extra length")]
    out = [(64 * n, 64 * p, "PE rows of the padding points"), (dirf * p + 16 * n, dirf * p + 16 * p, "direction rows of the padding points"),
           (m * p + 8 * nl * n, end, "mask words behind point n - 1 of the last layer")]
    return [r for r in out if r[0] < r[1]]


# ---------------------------------------------------------------------------------------------------------------- models
MLP = {"paper": O.paper_mlp, "lcode": O.lcode_mlp, "bshape": B.bshape_mlp, "cbshape": B.cbshape_mlp, "smaller": S.smaller_mlp}


@functools.lru_cache(maxsize=None)
def model_params(kind):
    """The parameters tests/test_gpu_density.py's _model(kind) loads (CPU, float32); every bias is non-zero -- a zero bias would hide
    a bias the kernels drop or take from another layer."""
    if kind == "paper":
        p = C.build_case("eval_det_64_128")["p_coarse"]
    elif kind == "lcode":
        p = O.init_lcode_params(6)
    elif kind == "smaller":
        p = S.init_smaller_params(14)
    else:
        p = B.init_params(kind, 14, boost="survey")
    for k, v in p.items():
        if k.endswith(".bias"):
            assert float(v.abs().min()) > 0, (kind, k)
    return p


@functools.lru_cache(maxsize=None)
def conditioning():
    """(expression (76), latent code (32)) of that module's _model: frame 3's."""
    c = C.build_case("eval_det_64_128")
    return c["expr"], c["latent"]


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _ray_pool(kind, n):
    ro, rd, _, _, _ = C.ray_subset(512, 512, 3, n, SEED[kind])
    return ro, rd


def inputs(kind, n_rays, n_samples):
    """float32 CPU inputs of one case: rays of frame 3 (C.ray_subset), sorted random depths in [0.2, 0.8]; fixed seed per model and size."""
    ro, rd = _ray_pool(kind, max(1024, n_rays))
    g = torch.Generator().manual_seed(1000 * SEED[kind] + 7 * n_rays + n_samples)
    z = torch.sort(torch.rand((n_rays, n_samples), generator=g) * 0.6 + 0.2, dim=-1)[0]
    return ro[:n_rays].contiguous(), rd[:n_rays].contiguous(), z.contiguous()


def grid_counts(n_cu):
    """The persistent grid of the exact-f32 inference kernels (at most one 128-point workgroup per CU, nf_paper_net_launch_fwd): one point
    below, at and above a full lap, and a second lap whose last block is partial."""
    return [128 * n_cu - 1, 128 * n_cu, 128 * n_cu + 1, 2 * 128 * n_cu + 33]


def grid_inputs(kind, n):
    """n rays with one sample each: the first n of these serve every count of grid_counts."""
    ro, rd, _, _, _ = C.ray_subset(512, 512, 3, n, SEED[kind] + 100)
    g = torch.Generator().manual_seed(1000 * SEED[kind] + 999)
    return ro, rd, (torch.rand((n, 1), generator=g) * 0.6 + 0.2).contiguous()


def other_view(rd):
    """A `rd_view` whose z-component differs from rd's; x and y are NaN: the kernels read rd_view[3 ray + 2] alone (Quirk Q1)."""
    rv = torch.full_like(rd, float("nan"))
    rv[:, 2] = rd[:, 2] * 0.5 + 0.125
    return rv.contiguous()


def hot_rows(n):
    """Rows n - 1 and 0 and the last row of every 16-, 32- and 128-point unit."""
    rows = {0, n - 1}
    for u in (16, 32, 128):
        rows.update(range(u - 1, n, u))
    return sorted(rows)


# ---------------------------------------------------------------------------------------------------------------- the networks
def encode(ro, rd, z, rd_view=None, dtype=torch.float64):
    """-> (the float32 points (n, 3), x87 (n, 87) in `dtype` = [PE10 of the float32 point | PE4 of (rd_view_z, near, far)]): O.encode_points
    behind the float32 point."""
    assert ro.dtype == rd.dtype == z.dtype == torch.float32
    n_rays, n_samples = z.shape
    pts = (ro[:, None, :] + rd[:, None, :] * z[:, :, None]).reshape(-1, 3)
    vz = (rd if rd_view is None else rd_view)[:, 2].to(dtype)
    fake = torch.stack((vz, torch.full_like(vz, O.NEAR), torch.full_like(vz, O.FAR)), dim=-1)
    dirs = fake[:, None, :].expand(n_rays, n_samples, 3).reshape(-1, 3)
    return pts, torch.cat((O.posenc(pts.to(dtype), 10, True), O.posenc(dirs, 4, False)), dim=-1)


def _network(kind, p, x87, expr, latent):
    """-> (raw, acts, pre): the family's network with its `acts` hook and, through torch.relu, the input of every ReLU of the trunk."""
    acts, pre = [], []
    keep = torch.relu

    def relu(v):
        pre.append(v)
        return keep(v)
    torch.relu = relu
    try:
        raw = MLP[kind](p, x87, expr, latent, acts=acts)
    finally:
        torch.relu = keep
    if kind == "cbshape":
        pre = pre[3:]                                # the expression encoder's three ReLUs come first (tests/blendshape_ref.py: encoder)
    return raw, acts, pre


def forward64(kind, ro, rd, z, rd_view=None):
    """The reference on the inputs' device -> dict: pts32 (n, 3) float32; pe (n, 63) and dirs (n, 24) fp64 in reference column order;
    raw (n, 4); `act`: section name -> what the training forward saves there; `pre`: section name -> the ReLU's input, for the
    sections behind one; t_sigma: the f16x2 density gate's T = max over points of sqrt(sum_k (x_k fc_alpha.weight_k)^2), x = fc_alpha's
    input (tests/test_gpu_f16x2.py, tests/test_gpu_blendshape.py)."""
    dev = ro.device
    p = {k: v.to(dev).double() for k, v in model_params(kind).items()}
    expr, latent = (t.to(dev).double() for t in conditioning())
    pts, x87 = encode(ro, rd, z, rd_view)
    raw, acts, pre = _network(kind, p, x87, expr, latent)
    lay = layout(kind)
    assert len(acts) == len(lay["acts"]) and len(pre) == len(lay["relu"])
    act = dict(zip(lay["acts"], acts))
    pre = dict(zip(lay["relu"], pre))
    for k in lay["relu"]:
        assert torch.equal(act[k], torch.relu(pre[k])), (kind, k)
    x_alpha = act["x2"] if LAYOUT_OF[kind] == "lcode" else act["feat"]
    t_sigma = float(((x_alpha ** 2) @ (p["fc_alpha.weight"] ** 2).t()).sqrt().max())
    return dict(pts32=pts, pe=x87[:, :63], dirs=x87[:, 63:], raw=raw, act=act, pre=pre, t_sigma=t_sigma)


def forward32(kind, ro, rd, z):
    """The same network evaluated by torch in float32 throughout -> raw (n, 4): what the arithmetic costs without any kernel."""
    p = {k: v.to(ro.device) for k, v in model_params(kind).items()}
    expr, latent = (t.to(ro.device) for t in conditioning())
    _, x87 = encode(ro, rd, z, dtype=torch.float32)
    return MLP[kind](p, x87, expr, latent)


def scales(ref):
    """What the gates of one case are relative to, from a reference of at least 128 points: the largest magnitude per channel of raw,
    per unit of every saved section and per unit of every ReLU input; and T."""
    return dict(raw=ref["raw"].abs().amax(dim=0), act={k: v.abs().amax(dim=0) for k, v in ref["act"].items()},
                pre={k: v.abs().amax(dim=0) for k, v in ref["pre"].items()}, t_sigma=ref["t_sigma"])


# ---------------------------------------------------------------------------------------------------------------- gates
def gate(arith, scale):
    """The bound on |kernel - fp64| for a quantity whose largest magnitude is `scale`, in the arithmetics that have a relative gate:
    2e-5 * scale + 2e-5 for "f32" (test_paper_mlp_fwd, test_lcode_mlp_vs_fp64_oracle, test_smaller_mlp_three_routes_vs_fp64_restatement,
    test_blendshape_mlp_vs_fp64_restatement) and "f16x3" (test_f16x3_raw_outputs_meet_the_f32_gate, test_lcode_f16x3_mlp_meets_the_f32_gate),
    3e-4 * scale + 1e-5 for "bf16x3" (test_bf16x3_mlp_vs_oracle, test_lcode_bf16x3_mlp_vs_oracle)."""
    if arith in ("f32", "f16x3"):
        return 2e-5 * scale + 2e-5
    assert arith == "bf16x3", arith
    return 3e-4 * scale + 1e-5


def raw_gate(arith, sc):
    """Per channel of raw.  "f16x2": colours 1e-3, density 2e-3 T (test_f16x2_raw_outputs; tests/test_gpu_blendshape.py: mlp_bound)."""
    if arith == "f16x2":
        return torch.tensor([1e-3, 1e-3, 1e-3, 2e-3 * sc["t_sigma"]], dtype=torch.float64, device=sc["raw"].device)
    return gate(arith, sc["raw"])


def band_share(arith, ref, sc):
    """name -> share of the layer's ReLU inputs that lie inside the gate's band around 0, where a decision is not compared."""
    band = "f32" if arith == "f16x2" else arith
    return {k: float((z.abs() <= gate(band, sc["pre"][k])).double().mean()) for k, z in ref["pre"].items()}


def pe_in_slot_order(ref):
    """(n, 64): the reference's PE in the slot order of `saved` (nfl::pe_slot_to_col), 0 in the pad slot."""
    cols = [pe_slot_to_col(s) for s in range(64)]
    out = torch.zeros((ref["pe"].shape[0], 64), dtype=ref["pe"].dtype, device=ref["pe"].device)
    live = [s for s in range(64) if cols[s] >= 0]
    out[:, live] = ref["pe"][:, [cols[s] for s in live]]
    return out


def dir_slots(ref):
    """(n, 16): the direction slots of `saved`: (sin, cos, 0, 0)(rd_view_z 2^g), g = 0 .. 3 (reference columns 6 g and 6 g + 3 of PE4)."""
    out = torch.zeros((ref["dirs"].shape[0], 16), dtype=ref["dirs"].dtype, device=ref["dirs"].device)
    for g in range(4):
        out[:, 4 * g] = ref["dirs"][:, 6 * g]
        out[:, 4 * g + 1] = ref["dirs"][:, 6 * g + 3]
    return out
