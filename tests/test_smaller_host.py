"""CPU: the third model family (ConditionalBlendshapePaperSmallerNeRFModel) -- class and state_dict, gather table, dW job table,
cross-compiled kernel shapes, fixtures against the restatement, the precision refusal."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import smaller_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _model(**kw):
    import nerf
    return nerf.models.ConditionalBlendshapePaperSmallerNeRFModel(**dict(S.SMALLER_KW, **kw))


def test_smaller_class_matches_the_reference_layout():
    """state_dict keys, shapes and the 496,132 total equal SMALLER_SHAPES (the reference's own layout, tests/smaller_ref.py ref_model
    asserts it there); a reference-style dict round-trips; fused_supported() holds for the config geometry only."""
    import nerf
    from nerf import ops
    m = _model()
    sd = m.state_dict()
    assert list(sd.keys()) == S.SMALLER_KEYS == list(ops.SMALLER_KEYS) == list(ops.SMALLER.keys) and len(sd) == 22
    for k, shp in S.SMALLER_SHAPES.items():
        assert tuple(sd[k].shape) == shp and tuple(sd[k.replace("weight", "bias")].shape) == (shp[0],), k
    assert sum(p.numel() for p in m.parameters()) == S.SMALLER_NUMEL == 496132
    assert [tuple(p.shape) for p in m.hip_param_list()] == [tuple(sd[k].shape) for k in S.SMALLER_KEYS]
    p = S.init_smaller_params(3)
    m.load_state_dict(p)                                       # strict: no missing, no unexpected key
    assert all(torch.equal(v, p[k]) for k, v in m.state_dict().items())
    assert m.fused_supported() and m.FAMILY is ops.SMALLER and ops.SMALLER.none_grads == ()
    assert not _model(num_encoding_fn_xyz=6).fused_supported()
    assert not _model(include_input_dir=True).fused_supported()
    assert not _model(use_viewdirs=False).fused_supported()
    assert not _model(latent_code_dim=16).fused_supported()
    # num_layers / hidden_size / skip_connect_every are accepted and ignored, as in the reference
    assert list(_model(num_layers=8, hidden_size=128, skip_connect_every=2).state_dict().keys()) == S.SMALLER_KEYS
    assert getattr(nerf.models, "ConditionalBlendshapePaperSmallerNeRFModel") is type(m)
    # default initialisation: torch.nn.Linear's, in the reference's construction order
    torch.manual_seed(5)
    a = _model().state_dict()
    torch.manual_seed(5)
    lin = [torch.nn.Linear(171, 256)] + [torch.nn.Linear(427 if i == 3 else 256, 256) for i in range(1, 5)]
    lin += [torch.nn.Linear(256, 256), torch.nn.Linear(256, 1), torch.nn.Linear(356, 128), torch.nn.Linear(128, 128),
            torch.nn.Linear(128, 128), torch.nn.Linear(128, 3)]
    for k, l in zip(list(S.SMALLER_SHAPES), lin):
        assert torch.equal(a[k], l.weight) and torch.equal(a[k.replace("weight", "bias")], l.bias), k


def test_smaller_gather_table_covers_every_weight_once(hip_lib):
    """Every weight element appears exactly once among the MFMA fragment sections -- except the folded columns, which appear exactly
    once in the conditioning matrices and nowhere in the fragments: 63:171 of layers_xyz.0 and layers_xyz.3, and in layers_dir.0 the
    16 near / far direction columns plus columns 280:356.  Every bias appears once.  (test_gather_table_covers_every_live_weight_once
    for this family; the pre-encoded entry's copy of layers_dir.0 lies behind the bias table.)"""
    n = hip_lib.nf_smaller_packed_floats()
    tab = np.zeros(n, dtype=np.uint32)
    assert hip_lib.nf_smaller_gather_table(tab.ctypes.data_as(ctypes.c_void_p), n) == 0
    assert hip_lib.nf_smaller_gather_table(tab.ctypes.data_as(ctypes.c_void_p), n - 1) != 0
    ids, offs = tab >> 24, tab & 0xFFFFFF
    shapes = [S.SMALLER_SHAPES[k] if k.endswith("weight") else (S.SMALLER_SHAPES[k.replace("bias", "weight")][0],) for k in S.SMALLER_KEYS]
    frag_end = (4 * 16 + 3 * 256 + 20 * 16 + 256 + 17 * 9 + 2 * 64 + 8) * 256                   # nsm::FRAG_END
    cond_end = frag_end + 2 * 256 * 108 + 128 * 16 + 128 * 76                                  # nsm::OFF_BIAS
    bias_end = cond_end + 1952                                                                 # nsm::OFF_D0E
    assert n == bias_end + 18 * 9 * 256
    assert set(np.unique(ids)) == set(range(22)) | {0xFF}
    varying = [256 + 6 * f + 3 * sc for f in range(4) for sc in range(2)]                     # the rd_z columns of PE4(dir)
    nearfar = [c for c in range(256, 280) if c not in varying]
    assert len(nearfar) == 16
    for tid, shp in enumerate(shapes):
        numel = int(np.prod(shp))
        assert offs[ids == tid].max() < numel
        if len(shp) == 1:
            cnt = np.bincount(offs[cond_end:bias_end][ids[cond_end:bias_end] == tid], minlength=numel)
            assert np.all(cnt == 1), tid
            assert not np.any(ids[:cond_end] == tid) and not np.any(ids[bias_end:] == tid)
            continue
        frag = np.bincount(offs[:frag_end][ids[:frag_end] == tid], minlength=numel).reshape(shp)
        cond = np.bincount(offs[frag_end:cond_end][ids[frag_end:cond_end] == tid], minlength=numel).reshape(shp)
        folded = np.zeros(shp, dtype=bool)
        if tid in (0, 6):
            folded[:, 63:171] = True
        elif tid == 14:
            folded[:, nearfar] = True
            folded[:, 280:356] = True
        assert np.array_equal(frag, (~folded).astype(frag.dtype)), tid
        assert np.array_equal(cond, folded.astype(cond.dtype)), tid
    # the pre-encoded layers_dir.0 image: feat + all 24 direction columns once, the expression columns never; fc_alpha once
    e_ids, e_offs = ids[bias_end:], offs[bias_end:]
    assert set(np.unique(e_ids)) == {12, 14, 0xFF}
    cnt = np.bincount(e_offs[e_ids == 14], minlength=128 * 356).reshape(128, 356)
    assert np.all(cnt[:, :280] == 1) and np.all(cnt[:, 280:] == 0)
    assert np.all(np.bincount(e_offs[e_ids == 12], minlength=256) == 1)


def test_smaller_sizes_and_job_table(hip_lib):
    """The dW job table self-test (every slab entry the unpack kernel reads is written exactly once per slice) and the buffer sizes of
    csrc/nf_mlp_smaller_layout.h."""
    assert hip_lib.nf_selftest_dw_tables_smaller_f32() == 0
    assert hip_lib.nf_smaller_grad_floats() == 496132 + 32
    assert hip_lib.nf_smaller_cond_floats() >= 2076
    assert hip_lib.nf_smaller_saved_floats(100) == 2064 * 128 + 8 * 128
    assert hip_lib.nf_smaller_packed_bwd_floats() == (8 + 64 + 64 + 9 * 16 + 5 * 256) * 256
    assert hip_lib.nf_smaller_bwd_workspace_floats(4096) > 1920 * 4096
    # NULL pointers are refused before anything touches a device
    assert hip_lib.nf_smaller_pack(None, None, None) != 0 and hip_lib.nf_smaller_condition(None, None, None, 0.0, 1.0, None, None) != 0
    assert hip_lib.nf_smaller_mlp_fwd(None, None, None, None, None, None, 4, 4, None, None) != 0
    assert hip_lib.nf_smaller_mlp_fwd_train(None, None, None, None, None, None, 4, 4, None, None, None) != 0
    assert hip_lib.nf_smaller_mlp_bwd(None, None, None, None, None, 4, 4, None, 0, None, None) != 0
    assert hip_lib.nf_smaller_forward_encoded(None, None, None, None, 4, None, None, None) != 0


def test_smaller_kernels_keep_their_shape(tmp_path):
    """CPU (hipcc cross-compiles gfx950), as test_hot_kernels_keep_their_register_and_instruction_budget: the new forward, training
    forward and chain kernels have no spill, no scratch, 131,072 bytes of LDS (four wave-private 32 KiB slabs), no flat_load, no
    s_barrier, and stream their weights as buffer_load_dwordx4."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is needed to build the library at all"
    sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))
    import build
    src_dir = os.path.join(ROOT, "4d-facial-avatars_amd", "csrc")
    assert "nf_mlp_smaller.hip" in build.SOURCES and "nf_mlp_smaller_bwd.hip" in build.SOURCES

    def kernels(src):
        out = str(tmp_path / (src + ".s"))
        subprocess.run([hipcc, *build.FLAGS, "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", out, os.path.join(src_dir, src)],
                       check=True, capture_output=True)
        txt = open(out).read()
        found = {}
        for m in re.finditer(r"- \.agpr_count:\s+(\d+).*?\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?"
                             r"\.sgpr_spill_count:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", txt, re.S):
            agpr, lds, name, scratch, sspill, vgpr, spill = m.groups()
            body = re.search(r"^%s:[^\n]*\n(.*?)\n\s*s_endpgm" % re.escape(name), txt, re.S | re.M).group(1)
            found[name] = dict(lds=int(lds), scratch=int(scratch), vgpr=int(vgpr), spill=int(spill) + int(sspill), body=body)
        return found

    def one(ks, name):
        hit = [v for k, v in ks.items() if re.search(r"\d+%sILi2E" % re.escape(name), k)]
        assert len(hit) == 1, (name, sorted(ks))
        return hit[0]

    ks = kernels("nf_mlp_smaller.hip")
    n_mfma = {}
    for name in ("k_smaller_mlp_fwd", "k_smaller_mlp_fwd_save", "k_smaller_mlp_fwd_encoded"):
        k = one(ks, name)
        assert k["spill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 512, (name, k["spill"], k["scratch"], k["vgpr"])
        assert k["lds"] == 131072
        b = k["body"]
        assert "flat_load" not in b and "s_barrier" not in b
        assert len(re.findall(r"buffer_load_dwordx4", b)) >= 500          # the weight and bias stream
        if name != "k_smaller_mlp_fwd_encoded":                           # (its INPUT rows x87 may arrive as vector loads)
            assert len(re.findall(r"global_load_dwordx4", b)) == 0        # no weight fragment through a 64-bit vector address
        n_mfma[name] = len(re.findall(r"v_mfma_f32_16x16x4_f32", b))
    # the same network in both forwards: a dropped or duplicated K chunk shows as a different static count
    assert n_mfma["k_smaller_mlp_fwd"] == n_mfma["k_smaller_mlp_fwd_save"] > 3000, n_mfma
    k = one(kernels("nf_mlp_smaller_bwd.hip"), "k_smaller_mlp_bwd_chain")
    assert k["spill"] == 0 and k["scratch"] == 0 and k["lds"] == 131072
    assert "flat_load" not in k["body"] and "s_barrier" not in k["body"]
    assert len(re.findall(r"buffer_load_dwordx4", k["body"])) >= 200


@pytest.mark.parametrize("name", [n for n in S.SMALLER_CASES if n != S.GRAD_CASE])
def test_smaller_restatement_matches_fixture(name):
    """The restatement on the CPU against the committed reference outputs: fixture, seeds and restatement cannot drift apart.  Same
    torch build: bit-exact.  Another build may differ in BLAS blocking -- then every output within the gate the GPU test holds the
    product to against the same fixture (another fp32 evaluation is allowed exactly that)."""
    c = S.build_case(name)
    gold = np.load(os.path.join(GOLD, f"{name}.npz"))
    assert abs(float(gold["params_checksum"]) - S.checksum(c)) < 1e-6, "seeded weight generation drifted; regenerate with tests/smaller_ref.py"
    out = S.run_restatement(c)
    tol = S.case_tol(name)
    for n, t in zip(S.NAMES7, out):
        if t is None:
            assert n not in gold.files
            continue
        got = t.numpy()
        assert got.shape == gold[n].shape and got.dtype == gold[n].dtype == np.float32
        assert np.array_equal(got, gold[n]) or np.abs(got - gold[n]).max() <= tol[n], (n, np.abs(got - gold[n]).max())
    # the float64 restatement -- the exact result -- within a third of every gate of the reference's fp32 output (the generator's choice
    # of seeds): half a gate here leaves room for another build's BLAS
    for n, t in zip(S.NAMES7, S.run_restatement(c, torch.float64)):
        if t is not None:
            assert np.abs(t.numpy() - gold[n]).max() <= 0.5 * tol[n], (n, np.abs(t.numpy() - gold[n]).max())


def test_smaller_gradient_fixture():
    """The restatement's fp32 and float64 autograd against the reference's autograd (Q9 shim) on the gradient case: loss, latent
    gradient, and per-tensor norms and 257-element heads of all 2 x 22 tensors, rel 1e-4 (the generator asserted 1e-5 between the
    reference's fp32 and the float64 autograd in every FULL tensor)."""
    c = S.build_case(S.GRAD_CASE)
    g = np.load(os.path.join(GOLD, f"{S.GRAD_CASE}_grads.npz"))
    assert abs(float(g["params_checksum"]) - S.checksum(c)) < 1e-6
    # (+ 1e-30: the head of a tensor whose first output unit never fires on these few rays is all zero on both sides)
    rel = lambda a, b: float(np.linalg.norm(a.double().numpy() - b.astype(np.float64)) / (np.linalg.norm(b.astype(np.float64)) + 1e-30))
    for dt in (torch.float32, torch.float64):
        loss, pc, pf, lat_grad, _ = S.autograd(c, dt)
        assert abs(float(loss) - float(g["loss"])) < 1e-6
        assert rel(lat_grad, g["latent"]) < 1e-4
        n = 0
        for tag, p in (("coarse", pc), ("fine", pf)):
            for k, v in p.items():
                want = float(g[f"norm:{tag}.{k}"])
                assert abs(float(v.grad.double().norm()) - want) <= 1e-4 * want, (dt, tag, k)
                assert rel(v.grad.reshape(-1)[:257], g[f"head:{tag}.{k}"]) < 1e-4, (dt, tag, k)
                n += 1
        assert n == 44


def test_smaller_family_declares_its_precisions(hip_lib):
    """The family record says which arithmetics it serves; a model of this family under another one raises NotImplementedError that
    names the family and "f32" -- before anything is packed (no device is touched: this runs on the CPU).  The other families serve all."""
    import nerf
    from nerf import ops
    assert ops.SMALLER.precisions == ("f32",) and ops.SMALLER.prefix == "nf_smaller" and not ops.SMALLER.exact_dw
    assert set(ops.PAPER.precisions) == set(ops.LCODE.precisions) == {"f32", "bf16x3", "f16x3", "f16x2"}
    m = _model()
    z = torch.zeros((2, 3))
    args = (torch.zeros((2, 3)), torch.zeros((2, 3)), z, None, torch.zeros(76), torch.zeros(32), 0.2, 0.8)
    for prec in ("f16x3", "bf16x3", "f16x2"):
        nerf.set_mlp_precision(prec)
        for need_grad in (False, True):
            with pytest.raises(NotImplementedError, match=r'nf_smaller.*"f32"'):
                m.hip_forward(*args, need_grad)
        assert m.hip_weights()._cache == {}
        ops.PAPER.require_precision(prec)
        ops.LCODE.require_precision(prec)
    nerf.set_mlp_precision("f32")
    ops.SMALLER.require_precision("f32")
    with pytest.raises(RuntimeError, match="ROCm device"):               # in "f32" the call goes on -- to the device check: no CPU path
        m.hip_forward(*args, False)
    with pytest.raises(NotImplementedError):
        m(torch.zeros(2, 87), torch.zeros(76), torch.zeros(32))           # grad mode: no autograd through forward()
