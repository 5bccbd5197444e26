"""Live-colour forward (nf_paper_mlp_fwd_live, ops.mlp_fwd_live, hip_forward(live_only=...)): what can be checked without a GPU -- the
ABI surface, the argument checks of the entry point, the scratch size, and when the Python layer takes the path."""
import ctypes

import pytest
import torch

from tests.test_density_host import EINVAL, KW, _declared

LIVE = ("int (*)(const float*, const float*, const float*, const float*, const float*, const float*, int64_t, int, float*, float*, size_t, "
        "int, nf_stream_t)")
WAVE_FLOATS = 64 * (1024 + 64 + 16) // 4           # a wave's ring: 64 rows of feat fragments, direction fragments and a point index


def test_symbols_are_declared_exported_and_prototyped(hip_lib):
    from nerf import _hip
    ok, log = _declared([("nf_paper_mlp_fwd_live", LIVE), ("nf_paper_mlp_fwd_live_scratch_floats", "size_t (*)(int)")])
    assert ok, log
    assert not _declared([("nf_lcode_mlp_fwd_live", LIVE)])[0]                # the paper family only
    for name in ("nf_paper_mlp_fwd_live", "nf_paper_mlp_fwd_live_scratch_floats"):
        assert hasattr(hip_lib, name) and name in _hip._PROTOTYPES and name not in _hip._OPTIONAL, name
    fwd = _hip._PROTOTYPES["nf_paper_mlp_fwd"][1]
    assert _hip._PROTOTYPES["nf_paper_mlp_fwd_live"][1] == fwd[:-1] + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int] + fwd[-1:]
    assert hip_lib.nf_abi_version() == 5 and _hip.ABI_VERSION == 5           # the ABI only grew


def test_scratch_size_and_argument_checks(hip_lib):
    """Four waves per workgroup, one ring each; a cap above the CU count (256 without a device) is the CU count.  NULL, short or
    misaligned scratch and a negative cap are NF_EINVAL before anything else; then the checks of the full forward."""
    size = hip_lib.nf_paper_mlp_fwd_live_scratch_floats
    assert size(1) == 4 * WAVE_FLOATS and size(2) == 8 * WAVE_FLOATS
    assert size(0) == size(1 << 20) and size(0) % (4 * WAVE_FLOATS) == 0 and size(0) >= size(2)
    fn = hip_lib.nf_paper_mlp_fwd_live
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    need = size(2)
    assert fn(one, one, one, one, None, one, 4, 64, one, None, need, 2, None) == EINVAL
    assert fn(one, one, one, one, None, one, 4, 64, one, one, need - 1, 2, None) == EINVAL
    assert fn(one, one, one, one, None, one, 4, 64, one, odd, need, 2, None) == EINVAL
    assert fn(one, one, one, one, None, one, 4, 64, one, one, need, -1, None) == EINVAL
    assert fn(None, None, None, None, None, None, 0, 64, None, one, need, 2, None) == 0          # empty work
    assert fn(None, one, one, one, None, one, 4, 64, one, one, need, 2, None) == EINVAL          # NULL weights
    assert fn(one, one, one, one, None, one, 4, 64, None, one, need, 2, None) == EINVAL          # NULL output
    assert fn(one, one, one, one, None, one, 4, 0, one, one, need, 2, None) == EINVAL


def test_when_the_python_layer_takes_the_path(hip_lib):
    """ops.live_colour_kernel: exact f32 and a family with the kernel; ops.live_colour_applies: also the switch, per pass.  hip_forward(live_only=True) refuses everything else
    before it packs a weight image."""
    import nerf
    from nerf import ops
    try:
        nerf.set_mlp_precision("f32")
        assert ops.live_colour_kernel(ops.PAPER) and not ops.live_colour_kernel(ops.SMALLER) and not ops.live_colour_kernel(ops.LCODE)
        ops.set_live_colour(None)
        assert [ops.live_colour_applies(ops.PAPER, w) for w in ("coarse", "fine")] == [w in ops.LIVE_PASSES_DEFAULT for w in ("coarse", "fine")]
        ops.set_live_colour(True)
        assert ops.live_colour_applies(ops.PAPER, "coarse") and ops.live_colour_applies(ops.PAPER, "fine")
        assert not ops.live_colour_applies(ops.SMALLER, "coarse")
        ops.set_live_colour(True, passes=("coarse",))
        assert ops.live_colour_applies(ops.PAPER, "coarse") and not ops.live_colour_applies(ops.PAPER, "fine")
        ops.set_live_colour(False)
        assert not ops.live_colour_applies(ops.PAPER, "coarse") and not ops.live_colour_applies(ops.PAPER, "fine")
        nerf.set_mlp_precision("f16x3")
        ops.set_live_colour(True)
        assert not ops.live_colour_kernel(ops.PAPER) and not ops.live_colour_applies(ops.PAPER, "coarse")
        m = nerf.models.ConditionalBlendshapePaperNeRFModel(**KW)
        t3, z = torch.zeros(2, 3), torch.zeros(2, 3)
        with pytest.raises(ValueError, match="live_only"):                     # not exact f32
            m.hip_forward(t3, t3, z, None, torch.zeros(76), torch.zeros(32), 0.2, 0.8, False, live_only=True)
        nerf.set_mlp_precision("f32")
        with pytest.raises(ValueError, match="live_only"):                     # a training forward
            m.hip_forward(t3, t3, z, None, torch.zeros(76), torch.zeros(32), 0.2, 0.8, True, live_only=True)
        s = nerf.models.ConditionalBlendshapePaperSmallerNeRFModel(**KW)
        with pytest.raises(ValueError, match="live_only"):                     # a family without the kernel
            s.hip_forward(t3, t3, z, None, torch.zeros(76), torch.zeros(32), 0.2, 0.8, False, live_only=True)
        assert m.hip_weights()._cache == {} and s.hip_weights()._cache == {}
        with pytest.raises(NotImplementedError, match="no live-colour kernel"):
            ops.mlp_fwd_live(ops.LCODE, None, None, None, None, z)
    finally:
        ops.set_live_colour(None)
        nerf.set_mlp_precision("f32")
