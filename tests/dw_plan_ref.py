"""Host model of the two slice plans of the fused MLP families' weight-gradient GEMMs: nf_dw_plan_groups (csrc/nf_mlp_dw.h, the
exact-f32 shared-panel kernel: a slice count and a slice length PER GROUP of four products) and nfb_dw_plan
(csrc/nf_mlp_bf16_dw.hip, the split kernels: one plan for all products).  No arithmetic and no torch: the model says which rows
each slice of each group covers, the GPU tests (tests/test_gpu_dw_plans.py) say that the gradients summed over them are right.

A family is named by its entry-point prefix ("nf_paper", "nf_smaller", "nf_lcode").  The share of a group is its relative cost in
half-units (NfDwGroup::share): 2 for four full 128 x 128 products, 1 for the products against the 64-wide positional encoding."""
from __future__ import annotations

import os

MIN_PPS_F32, MIN_PPS_SPLIT = 1024, 256
# groups in table order (nf_paper_net_build_dw_groups, nf_lcode_build_dw_groups): the 256 x 256 layers, then -- paper models -- the
# products against the positional encoding (share 1) and the two view-branch groups
SHARES = {"nf_paper": (2,) * 6 + (1, 2, 2), "nf_smaller": (2,) * 5 + (1, 2, 2), "nf_lcode": (2,) * 6}
# nfb_dw_plan: `model` 0 is the paper model (11 bundles x 23 slices = 253 workgroups); every other model index -- the second family,
# and the smaller paper model, which has no split kernels but whose workspace is sized through the same function -- gets 32
SPLIT_TARGET = {"nf_paper": 23, "nf_lcode": 32, "nf_smaller": 32}
SPLIT_FAMILIES = ("nf_paper", "nf_lcode")


def _slices(n_points: int, want: int, floor: int):
    pps = -(-n_points // want)
    pps = -(-pps // 16) * 16
    pps = max(pps, floor)
    return pps, -(-n_points // pps)


def unit(family: str, n_cu: int) -> int:
    """Slices a share-2 group is given when the points suffice: one workgroup per CU over all groups."""
    return max(1, (2 * n_cu) // sum(SHARES[family]))


def group_plan(family: str, n_points: int, n_cu: int):
    """-> ([(share, pts_per_slice, n_slices) per group], most): nf_dw_plan_groups.  `most` = the number of slabs the reduction sums."""
    u = unit(family, n_cu)
    plan = []
    for share in SHARES[family]:
        pps, ns = _slices(n_points, max(1, u * share // 2), MIN_PPS_F32)
        plan.append((share, pps, ns))
    return plan, max(ns for _, _, ns in plan)


def split_plan(family: str, n_points: int, target=None):
    """-> (pts_per_slice, n_slices): nfb_dw_plan.  target None: the family's own, or NERFACE_DW_SLICES where that is set to 1 .. 512
    (the library reads the variable on every call)."""
    if target is None:
        target = SPLIT_TARGET[family]
        try:
            v = int(os.environ.get("NERFACE_DW_SLICES", ""))
            if 1 <= v <= 512:
                target = v
        except ValueError:
            pass
    return _slices(n_points, target, MIN_PPS_SPLIT)


def regime(family: str, n_points: int, n_cu: int) -> int:
    """Exact-f32 plan: 0 while every group runs minimum-length slices, 1 while only the share-2 groups do (the share-1 group runs its
    full count of longer ones), 2 above.  A family without a share-1 group has no regime 1."""
    u = unit(family, n_cu)
    if n_points <= MIN_PPS_F32 * min(max(1, u * s // 2) for s in SHARES[family]):
        return 0
    return 1 if n_points <= MIN_PPS_F32 * u else 2


def switch_points(family: str, n_cu: int):
    """The largest point counts of regimes 0 and 1 (equal where the family has no share-1 group)."""
    u = unit(family, n_cu)
    return MIN_PPS_F32 * min(max(1, u * s // 2) for s in SHARES[family]), MIN_PPS_F32 * u


def edges(family: str, n_cu: int) -> dict:
    """Point counts at which a plan changes shape, per arithmetic: "f32" (group plan), "split" (split plan; absent for a family without
    split kernels), "exact_dw" (paper model: the group plan on the converted saves of a split forward).
    f32: a last slice of ONE row behind 1, 2, 3, 4 minimum-length slices (most = 2, 3, 4, 5: every tail residue of the reduction),
    then each switch point, the count behind it (a one-row last slice, or the first longer slices) and 17 behind it (a last slice of
    one whole 16-row chunk and a row).  split: the same around one minimum-length slice and around the target count of them."""
    a, b = switch_points(family, n_cu)
    out = {}
    if family == "nf_paper":
        f32 = [1025, 2049, 3073, 4097, a, a + 1, a + 17, b, b + 1, b + 17]
    elif family == "nf_smaller":
        f32 = [1025, a, a + 1, b, b + 1]
    else:
        f32 = [1025, 4097, b, b + 1]
    out["f32"] = sorted(set(f32))
    if family in SPLIT_FAMILIES:
        t = MIN_PPS_SPLIT * SPLIT_TARGET[family]
        out["split"] = sorted({MIN_PPS_SPLIT, MIN_PPS_SPLIT + 1, t, t + 1, t + 17})
    if family == "nf_paper":
        out["exact_dw"] = sorted({a + 1, b + 1})
    return out


def slice_rows(n_points: int, pps: int, n_slices: int):
    """[(first row, last row)] of every slice of a plan (the last slice ends at n_points - 1)."""
    return [(k * pps, min((k + 1) * pps, n_points) - 1) for k in range(n_slices)]
