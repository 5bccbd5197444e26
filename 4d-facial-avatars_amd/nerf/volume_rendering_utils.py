"""MI355X-native volume_render_radiance_field (reference nerf/volume_rendering_utils.py:7-75)."""
from __future__ import annotations

import torch

from . import ops


class _VolumeRender(torch.autograd.Function):
    """K5 forward/backward.  Differentiable w.r.t. `radiance_field` and `background_prior` through all four outputs (rgb_map,
    disp_map, acc_map, weights).  A backward that carries only d_rgb and needs no background gradient -- the trainer's loss,
    train_transformed_rays.py:355-375 -- is the rgb-only kernel (ops.volume_render_bwd); anything else the full one."""

    @staticmethod
    def forward(ctx, raw, z, rd, noise, bg, white_background):
        rgb, disp, acc, w = ops.volume_render_fwd(raw, z, rd, noise, bg, white_background)
        ctx.save_for_backward(raw, z, rd, noise, bg)
        ctx.white_background = white_background
        ctx.set_materialize_grads(False)       # an output the loss does not read arrives as None, not as a zero-filled tensor
        return rgb, disp, acc, w

    @staticmethod
    def backward(ctx, d_rgb, d_disp, d_acc, d_w):
        raw, z, rd, noise, bg = ctx.saved_tensors
        need_d_bg = bg is not None and ctx.needs_input_grad[4]
        if d_rgb is None and d_disp is None and d_acc is None and d_w is None:
            return None, None, None, None, None, None
        if d_disp is None and d_acc is None and d_w is None and not need_d_bg:
            return ops.volume_render_bwd(raw, z, rd, noise, bg, d_rgb.contiguous(), ctx.white_background), None, None, None, None, None
        d_raw, d_bg = ops.volume_render_bwd_full(raw, z, rd, noise, bg, ops._c(d_rgb), ops._c(d_disp), ops._c(d_acc), ops._c(d_w), None,
                                                 ctx.white_background, need_d_bg)
        return d_raw, None, None, None, d_bg, None


def volume_render_radiance_field(radiance_field, depth_values, ray_directions, radiance_field_noise_std=0.0,
                                 white_background=False, background_prior=None):
    """Same signature and return tuple as the reference: (rgb_map, disp_map, acc_map, weights, None).

    Like the reference, the caller is expected to have overwritten radiance_field[:, -1, :3] with the
    background when `background_prior` is given (train_utils.py:95-96); the kernel reads the colour of the
    last sample from `background_prior` directly, which is the same value."""
    raw = ops._c(radiance_field)
    z = ops._c(depth_values)
    rd = ops._c(ray_directions)
    bg = ops._c(background_prior) if background_prior is not None else None
    noise = None
    if radiance_field_noise_std > 0.0:
        noise = torch.randn(raw[..., 3].shape, dtype=raw.dtype, device=raw.device) * radiance_field_noise_std
    lead = z.shape[:-1]
    S = z.shape[-1]
    rgb, disp, acc, w = _VolumeRender.apply(raw.reshape(-1, S, 4), z.reshape(-1, S), rd.reshape(-1, 3),
                                            None if noise is None else noise.reshape(-1, S),
                                            None if bg is None else bg.reshape(-1, 3), bool(white_background))
    return rgb.reshape(*lead, 3), disp.reshape(lead), acc.reshape(lead), w.reshape(*lead, S), None
