"""The specification of the tiny path's two fused MLP families (csrc/nf_tiny.hip: VeryTinyNerfModel; csrc/nf_flex.hip:
FlexibleNeRFModel with 2 .. 5 layers) in plain torch: the PE slot order of the `saved` buffer, the slice plan of the backward's
weight-gradient kernel, the network in fp64 with everything the training forward saves, and fp64 autograd at given ReLU masks.  No
GPU and no library: tests/test_tiny_plan_host.py holds the plan and the slot map against the library, tests/test_gpu_tiny_edges.py
holds the kernels against the rest.

`params` is a state_dict-ordered mapping as oracle.nerface_oracle.tiny_init_params / flex_init_params return it; its key order is
the order of the backward's gradient vector."""
from __future__ import annotations

import torch

from oracle import nerface_oracle as O

N_FREQ = 10                    # PE(10, include input): 3 + 60 columns
PE_SLOTS, PE_COLS, HIDDEN = 64, 63, 128
MIN_PPS, TARGET_SLICES = 256, 256


# ---------------------------------------------------------------------------------------------------------------- PE slot order
def pe_slot_to_col(slot: int) -> int:
    """nfl::pe_slot_pair / nfl::pe_slot_to_col (csrc/nf_mlp_layout.h): slot = 16 j + 4 g + r (K chunk j, lane group g, MFMA step r) ->
    column of the reference's PE [x y z | sin f0 xyz | cos f0 xyz | sin f1 xyz | ...], -1 for the one zero pad (slot 63)."""
    j, g, r = slot >> 4, (slot >> 2) & 3, slot & 3
    if g < 3:
        pair = g * 8 + j * 2 + (r >> 1)
    else:
        pair = 24 + j * 2 + (r >> 1) if j < 3 else -1
    if pair >= 0:
        return 3 + 6 * (pair // 3) + 3 * (r & 1) + pair % 3
    return r if r < 3 else -1


# ---------------------------------------------------------------------------------------------------------------- slice plan
def bwd_plan(n_points: int):
    """nf_tiny_bwd_plan (nf_flex_bwd_plan is the same) -> (pts_per_slice, n_slices): one slice per CU wanted (256), slices start on
    a 16-point chunk and none is shorter than 256 points."""
    pps = -(-n_points // TARGET_SLICES)
    pps = -(-pps // 16) * 16
    pps = max(pps, MIN_PPS)
    return pps, -(-n_points // pps)


def slice_rows(n_points: int):
    """[(first row, last row)] of every slice of bwd_plan(n_points)."""
    pps, ns = bwd_plan(n_points)
    return [(k * pps, min((k + 1) * pps, n_points) - 1) for k in range(ns)]


def dz_per_point(kind: str, num_layers: int = 0) -> int:
    """Floats per point of the backward chain's dZ sections: nft::DZ_PER_POINT, NfFlex<L - 1>::DZ_PER_POINT."""
    return 256 if kind == "tiny" else 128 * num_layers


def hot_rows(n_points: int):
    """Rows at which a 16-point tile, a 32-point wave, a 128-point workgroup or a slice begins or ends, as far as they exist."""
    pps, ns = bwd_plan(n_points)
    rows = {0, 15, 16, 31, 32, 127, 128, n_points - 1}
    for k in range(1, ns):
        rows.update((k * pps - 1, k * pps))
    return sorted(r for r in rows if 0 <= r < n_points)


# (n_rays, n_samples) of the GPU tests, by the edge they sit on.  SIZES_ALL run for every model, SIZES_ENDS for the tiny model and the
# two ends of the flex kernels' NH recursion (2 and 5 layers).  The plan column is asserted in tests/test_tiny_plan_host.py.
SIZES_ALL = [
    # 16-point tile, 32-point wave ((3, 16) = 48: the second tile of the last wave is empty)
    (1, 1), (5, 3), (16, 1), (17, 1), (31, 1), (1, 32), (11, 3), (3, 16),
    # 128-point workgroup
    (127, 1), (4, 32), (43, 3),
    # one slice / two slices, the second of one row
    (85, 3), (8, 32), (257, 1),
    # more than two slabs in the reduction: 2, 3 (last of one row), 4, 5 (last of one row)
    (7, 73), (27, 19), (32, 32), (1025, 1),
]
SIZES_ENDS = [
    # 256 full slices; 256 slices, the last of one row; slices of 272 points (241 of them); 272-point slices, the last of one row
    (2048, 32), (673, 97), (65537, 1), (65553, 1),
]
PLAN_OF_SIZE = {
    (1, 1): (256, 1), (5, 3): (256, 1), (16, 1): (256, 1), (17, 1): (256, 1), (31, 1): (256, 1), (1, 32): (256, 1), (11, 3): (256, 1),
    (3, 16): (256, 1), (127, 1): (256, 1), (4, 32): (256, 1), (43, 3): (256, 1), (85, 3): (256, 1), (8, 32): (256, 1),
    (257, 1): (256, 2), (7, 73): (256, 2), (27, 19): (256, 3), (32, 32): (256, 4), (1025, 1): (256, 5),
    (2048, 32): (256, 256), (673, 97): (256, 256), (65537, 1): (272, 241), (65553, 1): (272, 242),
}
MODELS = ["tiny", "flex2", "flex3", "flex4", "flex5"]
MODELS_ENDS = ["tiny", "flex2", "flex5"]


def cases():
    """[(model, n_rays, n_samples)] of the GPU tests."""
    return [(m, r, s) for m in MODELS for r, s in SIZES_ALL] + [(m, r, s) for m in MODELS_ENDS for r, s in SIZES_ENDS]


def model_params(model: str):
    """-> (kind, num_layers, params): the fixtures of tests/test_gpu_tiny.py."""
    if model == "tiny":
        return "tiny", 0, O.tiny_init_params(9458)
    num_layers = int(model[4:])
    return "flex", num_layers, O.flex_init_params(4000 + num_layers, num_layers)


def inputs(n_rays: int, n_samples: int):
    """float32 CPU inputs of one size: ro non-zero, rd ~ 0.3 randn, depths sorted in [2, 6]; fixed seed per size."""
    g = torch.Generator().manual_seed(52000 + 97 * n_rays + n_samples)
    ro = torch.randn((n_rays, 3), generator=g) * 0.25 + torch.tensor([0.3, -0.2, 0.4])
    rd = torch.randn((n_rays, 3), generator=g) * 0.3
    depth = torch.sort(torch.rand((n_rays, n_samples), generator=g) * 4 + 2, dim=-1)[0]
    return ro.contiguous(), rd.contiguous(), depth.contiguous()


# ---------------------------------------------------------------------------------------------------------------- the networks
def layer_names(kind: str, params):
    """-> (first layer, hidden layers behind a ReLU, output layer).  tiny: layer1 itself is followed by a ReLU, so it counts as hidden."""
    if kind == "tiny":
        return None, ["layer1", "layer2"], "layer3"
    n_hidden = sum(1 for k in params if k.startswith("layers_xyz.") and k.endswith(".weight"))
    return "layer1", [f"layers_xyz.{i}" for i in range(n_hidden)], "fc_out"


def points32(ro, rd, depth):
    """ro + rd * depth in float32 with a separate multiply and add (the kernels' nf_mul / nf_add): (n_rays * n_samples, 3)."""
    assert ro.dtype == rd.dtype == depth.dtype == torch.float32
    prod = rd[:, None, :] * depth[:, :, None]
    return (ro[:, None, :] + prod).reshape(-1, 3)


def _net(kind, p, pe, masks=None):
    """-> (raw, pre-activations, saved activations).  masks: one boolean (n, 128) per ReLU, which then is a multiplication by it."""
    first, hidden, last = layer_names(kind, p)
    pre, act = [], []
    h = pe
    if first is not None:                       # FlexibleNeRFModel: layer1 WITHOUT activation; its output is saved as it is
        h = O._lin(h, p, first)
        pre.append(h)
        act.append(h)
    for i, name in enumerate(hidden):
        z = O._lin(h, p, name)
        h = torch.relu(z) if masks is None else z * masks[i].to(z.dtype)
        pre.append(z)
        act.append(h)
    return O._lin(h, p, last), pre, act


def forward64(kind, params, ro, rd, depth):
    """The points in float32, everything behind them in fp64.  -> dict: pts32 (n, 3) float32; pe (n, 63), raw (n, 4), `act`: the
    hidden sections of `saved` in order (tiny: h1, h2 post-ReLU; flex: layer1's output as it is, then every layers_xyz[k] post-ReLU),
    `pre`: their pre-activations (flex: pre[0] is act[0]), `relu`: which sections sit behind a ReLU."""
    pts = points32(ro, rd, depth)
    p = {k: v.to(pts.device).double() for k, v in params.items()}
    pe = O.posenc(pts.double(), N_FREQ, True)
    raw, pre, act = _net(kind, p, pe)
    first, hidden, _ = layer_names(kind, p)
    return dict(pts32=pts, pe=pe, raw=raw, pre=pre, act=act, relu=[False] * (first is not None) + [True] * len(hidden))


def forward32(kind, params, ro, rd, depth):
    """The same network evaluated by torch in float32 throughout -> raw (n, 4): what the arithmetic costs without any kernel."""
    pts = points32(ro, rd, depth)
    p = {k: v.to(pts.device).float() for k, v in params.items()}
    return _net(kind, p, O.posenc(pts, N_FREQ, True))[0]


def grads64_at_masks(kind, params, pe64, masks, d_raw64):
    """fp64 autograd of sum(raw * d_raw) with every ReLU replaced by a multiplication with the given mask -> {name: gradient}.  A
    unit whose pre-activation is a rounding error away from 0 then cannot move the gradient."""
    p = {k: v.to(pe64.device).double().clone().requires_grad_(True) for k, v in params.items()}
    raw, _, _ = _net(kind, p, pe64, masks=masks)
    raw.backward(d_raw64)
    return {k: v.grad for k, v in p.items()}


def gate(ref, dim=0):
    """The forward gate per channel: 2e-5 * (the channel's largest magnitude) + 2e-5 (test_paper_mlp_fwd's)."""
    return 2e-5 * ref.abs().amax(dim=dim) + 2e-5
