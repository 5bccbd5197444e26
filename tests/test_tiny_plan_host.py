"""The host model of the tiny path (tests/tiny_ref.py) against the library and against itself: the backward's slice plan through the
workspace size (the library exposes no plan), the plan's invariants, the PE slot map, the size functions, and -- from the fp64
reference alone -- that the gates tests/test_gpu_tiny_edges.py applies are ones float32 arithmetic can meet at its seeds.  No device."""
import functools

import pytest
import torch

from oracle import nerface_oracle as O
from tests import tiny_ref as T

FLEX_LAYERS = (2, 3, 4, 5)


def _sizes():
    """Every point count the GPU tests use, 1 .. 600 exhaustively and both sides of the step to 272-point slices."""
    ns = {r * s for _, r, s in T.cases()} | set(range(1, 601)) | set(range(65000, 66001))
    return sorted(ns)


def test_plan_model_follows_the_workspace_size(hip_lib):
    """workspace = DZ_PER_POINT n + (n_slices + 1) SLAB: the dZ sections, one slab per slice and the reduced slab.  SLAB from n = 1
    (one slice); then the formula with tiny_ref.bwd_plan's slice count at every size."""
    fams = [("tiny", 0, hip_lib.nf_tiny_bwd_workspace_floats)]
    fams += [("flex", L, functools.partial(hip_lib.nf_flex_bwd_workspace_floats, L)) for L in FLEX_LAYERS]
    for kind, L, ws in fams:
        dz = T.dz_per_point(kind, L)
        assert T.bwd_plan(1) == (256, 1)
        slab, rest = divmod(ws(1) - dz, 2)
        assert rest == 0 and slab > 0 and slab % 4 == 0, (kind, L, ws(1))
        # the slab holds every weight and bias gradient once, layer1's 64 slots wide, the output layer's bias padded to 16
        n_hidden = 1 if kind == "tiny" else L - 1
        assert slab == 128 * 64 + 128 + n_hidden * (128 * 128 + 128) + 4 * 128 + 16, (kind, L, slab)
        for n in _sizes():
            _, n_slices = T.bwd_plan(n)
            assert ws(n) == dz * n + (n_slices + 1) * slab, (kind, L, n, n_slices)


def test_plan_invariants():
    for n in _sizes():
        pps, ns = T.bwd_plan(n)
        assert pps % 16 == 0 and pps >= 256 and 1 <= ns <= 256, (n, pps, ns)
        rows = T.slice_rows(n)
        assert len(rows) == ns and rows[0][0] == 0 and rows[-1][1] == n - 1
        assert all(a <= b for a, b in rows), (n, rows[-1])                           # no slice is empty, the last one included
        assert all(rows[k + 1][0] == rows[k][1] + 1 for k in range(ns - 1)), n       # no row twice, none left out
        assert all(a % 16 == 0 for a, _ in rows)


def test_size_table_sits_on_the_plan_edges():
    """The plan column of the size table, and what the table is there for: one and two slices, every tail of the reduction (slab count
    modulo 4), a last slice of one row at 2, 3, 5 and 256 slices, 256 full slices, both slice lengths."""
    sizes = T.SIZES_ALL + T.SIZES_ENDS
    assert len(set(sizes)) == len(sizes) and set(sizes) == set(T.PLAN_OF_SIZE)
    for r, s in sizes:
        assert T.bwd_plan(r * s) == T.PLAN_OF_SIZE[(r, s)], (r, s, T.bwd_plan(r * s))
    assert {T.bwd_plan(r * s)[1] % 4 for r, s in T.SIZES_ALL} == {0, 1, 2, 3}
    one_row = {T.bwd_plan(r * s) for r, s in sizes if T.slice_rows(r * s)[-1][0] == r * s - 1 and r * s > 1}
    assert one_row == {(256, 2), (256, 3), (256, 5), (256, 256), (272, 242)}
    assert T.bwd_plan(255)[1] == T.bwd_plan(256)[1] == 1 and T.bwd_plan(65536) == (256, 256) and T.bwd_plan(65537)[0] == 272
    # point counts either side of a 16-point tile, a 32-point wave and a 128-point workgroup
    counts = {r * s for r, s in sizes}
    assert {15, 16, 17, 31, 32, 33, 48, 127, 128, 129} <= counts
    # the boundary-hot gradient touches both rows of every slice boundary
    for r, s in sizes:
        hot = set(T.hot_rows(r * s))
        for a, b in T.slice_rows(r * s):
            assert a in hot and b in hot


def test_pe_slot_map_is_a_bijection():
    cols = [T.pe_slot_to_col(s) for s in range(T.PE_SLOTS)]
    assert [s for s, c in enumerate(cols) if c < 0] == [63]
    assert sorted(c for c in cols if c >= 0) == list(range(T.PE_COLS))
    # the raw point sits in chunk 3 of lane group 3, in front of the pad
    assert cols[60:64] == [0, 1, 2, -1]
    # a (sin, cos) pair of one frequency and component shares a register pair: columns 3 apart
    for s in range(0, 60, 2):
        assert cols[s + 1] == cols[s] + 3 and (cols[s] - 3) % 6 < 3


def test_size_functions(hip_lib):
    for n in (1, 15, 256, 65537):
        assert hip_lib.nf_tiny_saved_floats(n) == n * (64 + 2 * 128)
    assert hip_lib.nf_tiny_grad_floats() == 128 * 63 + 128 + 128 * 128 + 128 + 4 * 128 + 4
    for n in (0, -1, -(1 << 40)):
        assert hip_lib.nf_tiny_saved_floats(n) == 0 and hip_lib.nf_tiny_bwd_workspace_floats(n) == 0, n
        for L in FLEX_LAYERS:
            assert hip_lib.nf_flex_saved_floats(L, n) == 0 and hip_lib.nf_flex_bwd_workspace_floats(L, n) == 0, (L, n)


def test_fixtures_have_biases():
    """A zero bias would hide a bias the kernels drop or take from another layer."""
    for m in T.MODELS:
        _, _, p = T.model_params(m)
        for k, v in p.items():
            if k.endswith(".bias"):
                assert float(v.abs().min()) > 0 and float(v.abs().max()) > 1e-2, (m, k)


def test_reference_restates_the_oracle():
    ro, rd, depth = T.inputs(11, 3)
    pts = ro.double()[:, None, :] + (rd[:, None, :] * depth[:, :, None]).double()
    for m in T.MODELS:
        kind, _, p = T.model_params(m)
        f = T.forward64(kind, p, ro, rd, depth)
        assert (f["pts32"].double() - pts.reshape(-1, 3)).abs().max() < 1e-6           # the float32 point, rounded once more by the add
        p64 = {k: v.double() for k, v in p.items()}
        x = O.posenc(f["pts32"].double(), 10, True)
        assert x.shape == (33, 63) and torch.equal(f["pe"], x)
        if kind == "flex":
            want = O.flex_mlp(p64, x)
        else:                                                                        # as tests/test_gpu_tiny.py spells the tiny model out
            want = O._lin(torch.relu(O._lin(torch.relu(O._lin(x, p64, "layer1")), p64, "layer2")), p64, "layer3")
        assert torch.equal(f["raw"], want)
        assert len(f["act"]) == len(f["pre"]) == len(f["relu"]) == (2 if kind == "tiny" else int(m[4:]))
        for a, z, relu in zip(f["act"], f["pre"], f["relu"]):
            assert torch.equal(a, torch.relu(z) if relu else z)
        # at the reference's own ReLU decisions the masked autograd is ordinary autograd
        masks = [z > 0 for z, relu in zip(f["pre"], f["relu"]) if relu]
        d_raw = torch.randn(f["raw"].shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
        got = T.grads64_at_masks(kind, p, f["pe"], masks, d_raw)
        pp = {k: v.double().clone().requires_grad_(True) for k, v in p.items()}
        T._net(kind, pp, f["pe"])[0].backward(d_raw)
        assert list(got) == list(p)
        for k in p:
            assert torch.allclose(got[k], pp[k].grad, rtol=1e-12, atol=1e-14), (m, k)


@pytest.mark.parametrize("model", T.MODELS)
def test_gates_are_ones_float32_can_meet(model):
    """From the fp64 reference alone, at the seeds the GPU tests use (every size below 2000 points; the three-model sizes above are
    checked where they run): torch's own float32 evaluation of the network stays under HALF the forward gate, and fewer than 1 % of a
    post-ReLU section's units have a pre-activation inside the gate's band around 0, where the mask comparison leaves them out."""
    kind, _, p = T.model_params(model)
    worst, worst_share = 0.0, 0.0
    for r, s in T.SIZES_ALL:
        ro, rd, depth = T.inputs(r, s)
        f = T.forward64(kind, p, ro, rd, depth)
        ratio = float(((T.forward32(kind, p, ro, rd, depth).double() - f["raw"]).abs().amax(dim=0) / T.gate(f["raw"])).max())
        worst = max(worst, ratio)
        assert ratio < 0.5, (model, r, s, ratio)
        for z, relu in zip(f["pre"], f["relu"]):
            if relu:
                share = float((z.abs() <= T.gate(z)).double().mean())
                worst_share = max(worst_share, share)
                assert share < 0.01, (model, r, s, share)
    print(f"tiny-edges host {model}: float32 torch error / gate at most {worst:.3f}, share of units inside the band at most {worst_share:.2e}")
