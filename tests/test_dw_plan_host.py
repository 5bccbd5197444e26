"""The host model of the weight-gradient slice plans (tests/dw_plan_ref.py) against the library, and the plans' own invariants.
No device needed: the library sizes the backward workspace on the host, and without a device its CU count answers 256."""
import random

import pytest

from tests import dw_plan_ref as P

FAMILIES = ("nf_paper", "nf_lcode", "nf_smaller")


def _n_cu():
    """The CU count the library plans with: the current device's, 256 where there is none (nf_cu_count, csrc/nf_common.h)."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def sweep(family, n_cu):
    ns = set()
    for lst in P.edges(family, n_cu).values():
        for e in lst:
            ns.update((e - 16, e - 1, e, e + 1, e + 16))
    rng = random.Random(20260 + len(family))
    ns.update(rng.randint(1, 300000) for _ in range(200))
    return sorted(n for n in ns if n >= 1)


def test_edges_on_256_cus_are_the_documented_ones():
    assert P.edges("nf_paper", 256) == {"f32": [1025, 2049, 3073, 4097, 15360, 15361, 15377, 30720, 30721, 30737],
                                        "split": [256, 257, 5888, 5889, 5905], "exact_dw": [15361, 30721]}
    assert P.edges("nf_smaller", 256) == {"f32": [1025, 17408, 17409, 34816, 34817]}
    assert P.edges("nf_lcode", 256) == {"f32": [1025, 4097, 43008, 43009], "split": [256, 257, 8192, 8193, 8209]}
    # the mixed regime of the paper model, as (pts_per_slice, n_slices) of a share-2 and of the share-1 group
    plan, most = P.group_plan("nf_paper", 15361, 256)
    assert (plan[0][1:], plan[6][1:], most) == ((1024, 16), (1040, 15), 16) and 15361 - 15 * 1024 == 1      # the 16th slice holds one row
    plan, most = P.group_plan("nf_paper", 30721, 256)
    assert (plan[0][1:], plan[6][1:], most) == ((1040, 30), (2064, 15), 30)


@pytest.mark.parametrize("family", FAMILIES)
def test_workspace_size_follows_the_plan_model(hip_lib, family):
    """bwd_workspace_floats(N) == dz_per_point N + (max(most, split n_slices) + 1) slab_floats + 16 over the sweep, with dz_per_point
    and slab_floats recovered from N = 1 and N = 2 (one slice in either plan).  This pins `most` of the group plan wherever it exceeds
    the split plan's count (and the split plan's where that is larger); the SHORT group's slice count is not visible through this
    size -- it only reaches the reduction (NfReduceAlt), which tests/test_gpu_dw_plans.py exercises.  The smaller paper model has no
    split kernels, but its workspace goes through the same nf_bwd_workspace_floats with its own model index, for which nfb_dw_plan
    answers the 32-slice target: that is what the model takes for it."""
    n_cu = _n_cu()
    ws = getattr(hip_lib, f"{family}_bwd_workspace_floats")
    w1, w2 = ws(1), ws(2)
    dz = w2 - w1
    slab = (w1 - dz - 16) // 2
    assert dz > 0 and slab > 0 and w1 == dz + 2 * slab + 16 and slab % 4 == 0
    for n in sweep(family, n_cu):
        _, most = P.group_plan(family, n, n_cu)
        _, ns_split = P.split_plan(family, n)
        assert ws(n) == dz * n + (max(most, ns_split) + 1) * slab + 16, (family, n, most, ns_split)


@pytest.mark.parametrize("v", [1, 2, 3, 46])
def test_workspace_size_follows_the_slice_knob(hip_lib, monkeypatch, v):
    """NERFACE_DW_SLICES is read on every call: the size asked for after it is set is the model's with that target."""
    n_cu, n = _n_cu(), 4736
    base = hip_lib.nf_paper_bwd_workspace_floats(n)
    w1, w2 = hip_lib.nf_paper_bwd_workspace_floats(1), hip_lib.nf_paper_bwd_workspace_floats(2)
    dz = w2 - w1
    slab = (w1 - dz - 16) // 2
    monkeypatch.setenv("NERFACE_DW_SLICES", str(v))
    _, most = P.group_plan("nf_paper", n, n_cu)
    pps, ns = P.split_plan("nf_paper", n)
    assert (pps, ns) == P.split_plan("nf_paper", n, target=v) and ns <= v
    assert hip_lib.nf_paper_bwd_workspace_floats(n) == dz * n + (max(most, ns) + 1) * slab + 16
    monkeypatch.delenv("NERFACE_DW_SLICES")
    assert hip_lib.nf_paper_bwd_workspace_floats(n) == base


@pytest.mark.parametrize("n_cu", [256, 304, 64])
@pytest.mark.parametrize("family", FAMILIES)
def test_plan_invariants(family, n_cu):
    """Every slice of every group is non-empty and together they cover the points once; slices start on a 16-row chunk; at most ONE
    slice count below `most` (nf_dw_reduce_alt describes one short count, else the driver falls back to zero-filled slabs); one
    workgroup per CU at most."""
    for n in sweep(family, n_cu):
        plan, most = P.group_plan(family, n, n_cu)
        assert len(plan) == len(P.SHARES[family]) and most == max(ns for _, _, ns in plan)
        for share, pps, ns in plan:
            assert ns * pps >= n and (ns - 1) * pps < n and pps % 16 == 0 and pps >= P.MIN_PPS_F32, (family, n, share, pps, ns)
        assert len({ns for _, _, ns in plan if ns != most}) <= 1, (family, n, plan)
        assert sum(ns for _, _, ns in plan) <= n_cu, (family, n, plan)
        pps, ns = P.split_plan(family, n, target=P.SPLIT_TARGET[family])
        assert ns * pps >= n and (ns - 1) * pps < n and pps % 16 == 0 and pps >= P.MIN_PPS_SPLIT and ns <= P.SPLIT_TARGET[family]


@pytest.mark.parametrize("n_cu", [256, 304])
def test_edges_reach_every_regime(n_cu):
    """The point counts the GPU tests run contain every regime of every family's group plan, every residue of `most` modulo 4 (the
    tail of k_grad_reduce), a short group, a one-row last slice, and both sides of each switch of the split plan."""
    residues = set()
    for family in FAMILIES:
        e = P.edges(family, n_cu)
        want = {0, 1, 2} if 1 in P.SHARES[family] else {0, 2}
        assert {P.regime(family, n, n_cu) for n in e["f32"]} == want, family
        plans = [P.group_plan(family, n, n_cu) for n in e["f32"]]
        if family == "nf_paper":
            assert {most % 4 for _, most in plans} == {0, 1, 2, 3}
        residues |= {most % 4 for _, most in plans}
        if 1 in P.SHARES[family]:
            assert any(any(ns < most for _, _, ns in plan) and any(pps == 1024 for _, pps, _ in plan) for plan, most in plans)   # mixed
            assert any(any(ns < most for _, _, ns in plan) and all(pps > 1024 for _, pps, _ in plan) for plan, most in plans)
        assert any(n - (ns - 1) * pps == 1 for n, (plan, _) in zip(e["f32"], plans) for _, pps, ns in plan)
        if "split" in e:
            t = P.SPLIT_TARGET[family]
            got = {(pps > 256, ns) for pps, ns in (P.split_plan(family, n, target=t) for n in e["split"])}
            assert {(False, 1), (False, 2), (False, t)} <= got and any(longer for longer, _ in got), (family, got)
        for n in e.get("exact_dw", ()):
            assert P.regime(family, n, n_cu) in (1, 2)
    assert residues == {0, 1, 2, 3}
