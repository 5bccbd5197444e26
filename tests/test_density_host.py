"""Density-only forward (nf_*_mlp_sigma*, nf_volume_weights_fwd, nerf.density, coarse_density_only): what can be checked without a GPU --
the ABI surface, the argument checks of the new entry points and the refusals of the Python layer, each before any launch."""
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
FULL = ("nf_paper", "nf_lcode", "nf_bshape", "nf_cbshape")
SPLIT = ("_bf16", "_f16", "_f16x2")
NEW = [f"{p}_mlp_sigma{s}" for p in FULL for s in ("",) + SPLIT] + ["nf_smaller_mlp_sigma", "nf_volume_weights_fwd"]


def _c_compiler():
    import shutil
    for cand in ("cc", "gcc", "clang", "/opt/rocm/lib/llvm/bin/clang"):
        path = shutil.which(cand)
        if path:
            return path
    raise AssertionError("no C compiler found to parse include/nerface_hip.h with")


def _declared(names_and_types):
    """A C compiler parses the header and a pointer of the expected type is initialised from every name: an undeclared name, or one
    declared with another signature, is a compile error (the header is plain C and declares the sigma family through a macro)."""
    import subprocess
    src = '#include "nerface_hip.h"\n' + "".join(f"{t.replace('(*)', f'(*p_{n})')} = {n};\n" for n, t in names_and_types)
    r = subprocess.run([_c_compiler(), "-fsyntax-only", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src.encode(),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return r.returncode == 0, r.stdout.decode()


FWD_F32 = "int (*)(const float*, const float*, const float*, const float*, const float*, const float*, int64_t, int, float*, nf_stream_t)"
FWD_SPLIT = FWD_F32.replace("int (*)(const float*", "int (*)(const void*", 1)
WEIGHTS = "int (*)(const float*, const float*, const float*, const float*, int64_t, int, float*, float*, float*, nf_stream_t)"


def test_new_symbols_are_declared_exported_and_prototyped(hip_lib):
    from nerf import _hip
    typed = [(n, WEIGHTS if n == "nf_volume_weights_fwd" else FWD_F32 if n.endswith("_mlp_sigma") else FWD_SPLIT) for n in NEW]
    ok, log = _declared(typed)
    assert ok, log
    assert not _declared([("nf_paper_mlp_sigma_f32", FWD_F32)])[0]               # the check can fail: a name the header lacks
    for name in NEW:
        assert hasattr(hip_lib, name), f"libnerface_hip.so does not export {name}"
        assert name in _hip._PROTOTYPES and name not in _hip._OPTIONAL, name
    sig = _hip._PROTOTYPES["nf_paper_mlp_fwd"]
    for name in NEW[:-1]:                                   # <prefix>_mlp_fwd*'s signature, sigma in place of raw
        assert _hip._PROTOTYPES[name] == sig, name
    assert len(_hip._PROTOTYPES["nf_volume_weights_fwd"][1]) == 10
    assert hip_lib.nf_abi_version() == 5 and _hip.ABI_VERSION == 5          # the ABI only grew


def test_smaller_family_has_the_exact_f32_form_only(hip_lib):
    from nerf import _hip
    assert hasattr(hip_lib, "nf_smaller_mlp_sigma")
    for s in SPLIT:
        name = f"nf_smaller_mlp_sigma{s}"
        assert not hasattr(hip_lib, name) and name not in _hip._PROTOTYPES and not _declared([(name, FWD_SPLIT)])[0], name


def test_argument_checks_of_the_new_entry_points(hip_lib):
    """As test_host.py holds nf_flex_mlp_fwd and the fused forwards: no rays = nothing to do (0), NULL pointers or impossible sizes
    = NF_EINVAL, all before a launch."""
    one = ctypes.c_void_p(16)                               # any non-NULL pointer: the checks come before a launch
    for name in NEW[:-1]:
        fn = getattr(hip_lib, name)
        assert fn(None, None, None, None, None, None, 0, 64, None, None) == 0, name                # empty work
        assert fn(None, None, None, None, None, None, 4, 64, None, None) == EINVAL, name
        assert fn(None, one, one, one, None, one, 4, 64, one, None) == EINVAL, name              # NULL weights
        assert fn(one, one, one, one, None, one, 4, 64, None, None) == EINVAL, name              # NULL output
        assert fn(one, None, one, one, None, one, 4, 64, one, None) == EINVAL, name              # NULL bias table
        assert fn(one, one, one, one, None, one, -1, 64, one, None) == EINVAL, name
        assert fn(one, one, one, one, None, one, 4, 0, one, None) == EINVAL, name
    w = hip_lib.nf_volume_weights_fwd                       # (sigma, z, rd, noise, n_rays, n_samples, disp, acc, weights, stream)
    assert w(None, None, None, None, 0, 64, None, None, None, None) == 0
    assert w(None, one, one, None, 4, 64, one, one, one, None) == EINVAL
    assert w(one, one, one, None, 4, 64, one, one, None, None) == EINVAL
    assert w(one, one, one, None, 4, 64, None, one, one, None) == EINVAL
    assert w(one, one, one, None, -1, 64, one, one, one, None) == EINVAL
    assert w(one, one, one, None, 4, 0, one, one, one, None) == EINVAL


KW = dict(num_encoding_fn_xyz=10, num_encoding_fn_dir=4, include_input_xyz=True, include_input_dir=False, use_viewdirs=True,
          num_layers=4, hidden_size=256, include_expression=True)


def test_density_needs_a_rocm_device(hip_lib):
    import nerf
    m = nerf.models.ConditionalBlendshapePaperNeRFModel(**KW)
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm device"):
        nerf.density(m, torch.zeros(4, 3), torch.zeros(76), torch.zeros(32))
    with torch.no_grad(), pytest.raises(NotImplementedError):                 # a class with a latent code needs it
        nerf.density(m, torch.zeros(4, 3), torch.zeros(76))
    assert m.hip_weights()._cache == {}


def _options(nerf, **extra):
    mode = dict(num_coarse=5, num_fine=7, chunksize=48, perturb=True, lindisp=False, radiance_field_noise_std=1.0,
                white_background=False, num_random_rays=64, **extra)
    return nerf.CfgNode(dict(nerf=dict(use_viewdirs=True, train=dict(mode), validation=dict(mode)),
                             dataset=dict(no_ndc=True, near=0.2, far=0.8)))


def test_coarse_density_only_is_refused_before_any_draw_or_launch(hip_lib):
    """Without a fine network the coarse colour is the image; with a gradient wanted there is no backward: ValueError in both cases,
    with the generator untouched and no weight image packed."""
    import nerf
    from nerf import train_utils as T
    mc, mf = nerf.models.ConditionalBlendshapePaperNeRFModel(**KW), nerf.models.ConditionalBlendshapePaperNeRFModel(**KW)
    ro, rd = torch.zeros(6, 3), torch.ones(6, 3)
    expr, latent = torch.zeros(76), torch.zeros(32)
    opt = _options(nerf, coarse_density_only=True)
    rng = torch.get_rng_state()
    with torch.no_grad(), pytest.raises(ValueError, match="fine network"):
        T._render_rays(ro, rd, None, mc, None, opt, "validation", expr, None, latent)
    with torch.enable_grad(), pytest.raises(ValueError, match="inference"):     # the parameters require grad
        T._render_rays(ro, rd, None, mc, mf, opt, "validation", expr, None, latent)
    assert torch.equal(torch.get_rng_state(), rng)
    assert mc.hip_weights()._cache == {} and mf.hip_weights()._cache == {}
    assert getattr(_options(nerf).nerf.validation, "coarse_density_only", False) is False        # the default: the key is absent


def test_smaller_hip_sigma_refuses_split_precisions(hip_lib):
    import nerf
    m = nerf.models.ConditionalBlendshapePaperSmallerNeRFModel(**KW)
    z = torch.zeros(2, 3)
    nerf.set_mlp_precision("f16x3")
    with pytest.raises(NotImplementedError, match='nf_smaller model family has no "f16x3" kernels'):
        m.hip_sigma(torch.zeros(2, 3), torch.zeros(2, 3), z, torch.zeros(76), torch.zeros(32), 0.2, 0.8)
    assert m.hip_weights()._cache == {}
