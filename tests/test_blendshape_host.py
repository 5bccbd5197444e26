"""CPU: the two blendshape classes without a learnable code (ConditionalBlendshapeNeRFModel, ConditionalCompressedBlendshapeNeRFModel)
-- classes and state_dicts, family records, exported symbols, the second family's refactored gather tables, the restatements."""
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch

from oracle import nerface_oracle as O
from tests import blendshape_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(kind, **kw):
    import nerf
    return getattr(nerf.models, B.CLASS[kind])(**dict(B.MODEL_KW, **kw))


def _reference():
    try:
        from oracle import ref_import as RI
        return RI.import_reference()
    except Exception:
        return None


@pytest.mark.parametrize("kind", B.KINDS)
def test_state_dict_is_the_reference_layout(kind):
    """Constructed with the trainer's keyword set: the reference's state_dict keys, order and shapes (the live reference where it can
    be imported, else the shapes tests/blendshape_ref.py lists, which its generator holds to the reference)."""
    from nerf import ops
    from oracle import make_golden as MG
    assert B.MODEL_KW == MG.DROPIN_MODEL_KW                            # neither class takes latent_code_dim
    m = _model(kind)
    sd = m.state_dict()
    fam = {"bshape": ops.BSHAPE, "cbshape": ops.CBSHAPE}[kind]
    assert list(sd.keys()) == B.KEYS[kind] == list(fam.keys) and len(sd) == {"bshape": 16, "cbshape": 22}[kind]
    for k, shp in B.SHAPES[kind].items():
        assert tuple(sd[k].shape) == shp and tuple(sd[k.replace("weight", "bias")].shape) == (shp[0],)
    assert sum(p.numel() for p in m.parameters()) == B.NUMEL[kind]
    assert [tuple(p.shape) for p in m.hip_param_list()] == [tuple(sd[k].shape) for k in B.KEYS[kind]]
    assert (m.layers_expr is None) == (kind == "bshape") and m.FAMILY is fam
    with pytest.raises(TypeError):
        _model(kind, latent_code_dim=32)
    ref = _reference()
    if ref is not None:
        rsd = getattr(ref.models, B.CLASS[kind])(**B.MODEL_KW).state_dict()
        assert [(k, tuple(v.shape)) for k, v in rsd.items()] == [(k, tuple(v.shape)) for k, v in sd.items()]


@pytest.mark.parametrize("kind", B.KINDS)
def test_fused_supported_for_the_configs_geometry_only(kind):
    assert _model(kind).fused_supported()
    for kw in (dict(use_viewdirs=False), dict(hidden_size=128), dict(num_layers=5)):
        m = _model(kind, **kw)                                         # constructs (and would load a checkpoint) but has no kernel
        assert not m.fused_supported(), kw
    assert "fc_out.weight" in _model(kind, use_viewdirs=False).state_dict()


def test_family_records():
    from nerf import ops
    for fam, prefix in ((ops.BSHAPE, "nf_bshape"), (ops.CBSHAPE, "nf_cbshape")):
        assert fam.prefix == prefix and fam.hidden == ops.LCODE.hidden == (64, 1472) and fam.none_grads == () and not fam.exact_dw
        assert set(fam.precisions) == {"f32", "bf16x3", "f16x3", "f16x2"}
        for prec in fam.precisions:
            fam.require_precision(prec)


def test_library_exports_every_declared_blendshape_symbol(hip_lib):
    from nerf import _hip, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerface_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nf_c?bshape_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 2 * 30               # the 29 family entry points + the stage-timing hook
    for name in sorted(declared):
        assert hasattr(hip_lib, name) and name in _hip._PROTOTYPES, name
    lib = _hip.lib()
    for fam, enc in ((ops.BSHAPE, 0), (ops.CBSHAPE, 4126)):
        n_params = sum(s[0] * s[1] + s[0] for s in B.SHAPES["bshape" if enc == 0 else "cbshape"].values())
        assert fam.fn("grad_floats")() == n_params + 32
        assert fam.fn("packed_floats")() == lib.nf_lcode_packed_floats() + ((enc + 3) & ~3)
        for size in ("cond_floats", "packed_bwd_floats", "packed_bf16_bytes", "packed_bwd_bf16_bytes", "packed_f16_bytes",
                     "packed_bwd_f16_bytes", "f16_flag_offset"):
            assert fam.fn(size)() == getattr(lib, "nf_lcode_" + size)(), size
        assert fam.fn("saved_floats")(259) == lib.nf_lcode_saved_floats(259)


# CRC-32 of the second family's split-stream gather tables as exported by the commit before the builders took a geometry record
LCODE_STREAM_TABLES = {"nf_lcode_stream_table_bf16": (327680, 1139123363), "nf_lcode_stream_table_bwd_bf16": (307200, 3095828169)}


@pytest.mark.parametrize("name", sorted(LCODE_STREAM_TABLES))
def test_refactored_builders_reproduce_the_second_familys_tables(hip_lib, name):
    n_want, crc = LCODE_STREAM_TABLES[name]
    fn = getattr(hip_lib, name)
    fn.restype, fn.argtypes = ctypes.c_long, [ctypes.c_void_p, ctypes.c_size_t]
    assert fn(None, 0) == n_want
    tab = np.zeros(n_want, dtype=np.uint32)
    assert fn(tab.ctypes.data_as(ctypes.c_void_p), n_want) == n_want
    assert zlib.crc32(tab.tobytes()) == crc


@pytest.mark.parametrize("kind", B.KINDS)
def test_restatement_equals_live_reference(kind):
    """257 points: the restatement equals the unmodified reference's forward to fp32 rounding."""
    ref = _reference()
    if ref is None:
        pytest.skip("the reference tree is not on this machine")
    p = B.init_params(kind, 21, boost="survey")
    m = B.ref_model(ref, kind, p)
    g = torch.Generator().manual_seed(5)
    x87 = torch.rand((257, 87), generator=g) * 2 - 1
    expr, _ = O.frame_conditioning(4)
    with torch.no_grad():
        want = m(x87, expr)
        got = B.MLP[kind](p, x87, expr)
    scale = want.abs().amax(dim=0)
    assert torch.all((got - want).abs().amax(dim=0) <= 4e-6 * scale + 1e-6)
    if kind == "cbshape":                                             # the latent code is ignored (M:821)
        with torch.no_grad():
            assert torch.equal(m(x87, expr, torch.ones(32)), want)
