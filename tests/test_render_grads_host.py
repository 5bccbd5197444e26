"""CPU: the host side of the integrator's full backward -- the two new C entries are declared, exported and prototyped and keep the
argument checks of the rgb-only entries; nerf.ops refuses a cotangent of the wrong shape or dtype by name before anything is launched;
the launcher's --supervised-background needs --train-background."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"nf_volume_render_bwd_full": 16, "nf_render_volume_density_bwd_full": 9}


def test_new_entries_are_declared_exported_and_prototyped(hip_lib):
    from nerf import _hip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerface_hip.h")).read(), flags=re.S)
    for name, n_args in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, f"{name} is not declared in include/nerface_hip.h"
        assert len(m.group(1).split(",")) == n_args
        assert hasattr(hip_lib, name)
        proto = [v for k, v in vars(_hip).items() if isinstance(v, dict) and name in v]
        assert len(proto) == 1 and len(proto[0][name][1]) == n_args
    assert _hip.ABI_VERSION == 5 == hip_lib.nf_abi_version()                      # added only: the revision stays


def test_new_entries_keep_the_argument_checks(hip_lib):
    """NF_EINVAL (-22) beyond 64 * NF_MAX_CHUNKS samples, for no cotangent at all and for a d_bg without a prior; no rays is a no-op.
    Nothing is launched by any of these calls (the checks come first), so they run without a device."""
    from nerf import ops
    one = 1                                                                       # any non-NULL pointer: never dereferenced on the host
    full, tiny = hip_lib.nf_volume_render_bwd_full, hip_lib.nf_render_volume_density_bwd_full
    assert full(one, one, one, None, None, one, None, None, None, None, 4, ops.MAX_BWD_SAMPLES + 1, 0, one, None, None) == -22
    assert tiny(one, one, one, None, None, 4, ops.MAX_BWD_SAMPLES + 1, one, None) == -22
    assert full(one, one, one, None, None, None, None, None, None, None, 4, 64, 0, one, None, None) == -22
    assert tiny(one, one, None, None, None, 4, 64, one, None) == -22
    assert full(one, one, one, None, None, one, None, None, None, None, 4, 64, 0, one, one, None) == -22       # d_bg, no bg
    assert full(None, None, None, None, None, None, None, None, None, None, 0, 64, 0, None, None, None) == 0
    assert tiny(None, None, None, None, None, 0, 64, None, None) == 0


@pytest.mark.parametrize("name,shape", [("d_rgb", (5, 4)), ("d_disp", (5, 1)), ("d_acc", (4,)), ("d_weights", (5, 7)), ("d_w_last", (5, 8))])
def test_wrong_shape_cotangent_is_refused_by_name(name, shape):
    from nerf import ops
    raw, z, rd = torch.zeros(5, 8, 4), torch.zeros(5, 8), torch.zeros(5, 3)
    with pytest.raises(ValueError, match=rf"volume_render_bwd_full: {name} must have shape"):
        ops.volume_render_bwd_full(raw, z, rd, None, None, **{name: torch.zeros(shape)})
    good = dict(d_rgb=(5, 3), d_disp=(5,), d_acc=(5,), d_weights=(5, 8), d_w_last=(5,))[name]
    with pytest.raises(ValueError, match=rf"volume_render_bwd_full: {name} must be float32"):
        ops.volume_render_bwd_full(raw, z, rd, None, None, **{name: torch.zeros(good, dtype=torch.float64)})
    if name in ("d_rgb", "d_acc"):
        with pytest.raises(ValueError, match=rf"render_volume_density_bwd_full: {name} must have shape"):
            ops.render_volume_density_bwd_full(raw, z, **{name: torch.zeros(shape)})


def test_tiny_depth_cotangent_and_empty_calls_are_refused_by_name():
    from nerf import ops
    raw, z, rd = torch.zeros(5, 8, 4), torch.zeros(5, 8), torch.zeros(5, 3)
    with pytest.raises(ValueError, match="render_volume_density_bwd_full: d_depth must have shape"):
        ops.render_volume_density_bwd_full(raw, z, d_depth=torch.zeros(5, 8))
    with pytest.raises(ValueError, match="no cotangent given"):
        ops.render_volume_density_bwd_full(raw, z)
    with pytest.raises(ValueError, match="no cotangent given"):
        ops.volume_render_bwd_full(raw, z, rd, None, None)
    with pytest.raises(ValueError, match="need_d_bg without a background prior"):
        ops.volume_render_bwd_full(raw, z, rd, None, None, d_rgb=torch.zeros(5, 3), need_d_bg=True)


def test_supervised_background_needs_train_background(capsys):
    sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))
    from launch import train_sharded
    with pytest.raises(SystemExit) as e:
        train_sharded.main(["--config", "unused.yml", "--supervised-background"])
    assert e.value.code == 2 and "--supervised-background requires --train-background" in capsys.readouterr().err
