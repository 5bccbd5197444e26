"""Tensor-level wrappers over the C ABI (one function per entry point of include/nerface_hip.h).

These allocate outputs with torch, pass raw device pointers + the current HIP stream, and translate
non-zero return codes into RuntimeError; sizes beyond a render kernel's compile-time limit are refused by name (ValueError) before
anything is allocated.  No numerical work happens in Python.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _hip as H

PAPER_KEYS = (
    [f"layers_xyz.{i}.{p}" for i in range(6) for p in ("weight", "bias")]
    + [f"{n}.{p}" for n in ("fc_feat", "fc_alpha") for p in ("weight", "bias")]
    + [f"layers_dir.{i}.{p}" for i in range(4) for p in ("weight", "bias")]
    + [f"fc_rgb.{p}" for p in ("weight", "bias")]
)
LCODE_KEYS = [f"{n}.{p}" for n in ("layer1", "layers_xyz.0", "layers_xyz.1", "layers_xyz.2", "layers_dir.0", "fc_alpha", "fc_rgb", "fc_feat")
              for p in ("weight", "bias")]
SMALLER_KEYS = [f"{n}.{p}" for n in ([f"layers_xyz.{i}" for i in range(5)] + ["fc_feat", "fc_alpha"] + [f"layers_dir.{i}" for i in range(3)]
                                     + ["fc_rgb"]) for p in ("weight", "bias")]
BSHAPE_KEYS = list(LCODE_KEYS)                                                   # ConditionalBlendshapeNeRFModel: layer1.weight (256, 139)
CBSHAPE_KEYS = [f"layers_expr.{i}.{p}" for i in range(3) for p in ("weight", "bias")] + LCODE_KEYS    # the compressed class: (256, 83)


# Arithmetic of the MLP GEMMs: "f32" = exact-f32 MFMA (the library default and the arithmetic of the reference);
# "bf16x3" = split-bf16, three bf16 MFMAs per product with f32 accumulation (~2^-16 relative per product, 3x faster).
# The switch applies to inference AND to a training step: under "bf16x3" the training forward, the dX chain and the
# weight-gradient GEMMs all run on the split-bf16 kernels (paper_mlp_bwd(..., exact_dw=True) keeps the dW GEMMs exact).
# "f16x3" = split-fp16: the same three-MFMA scheme on fp16 pairs (22 operand bits, per-layer power-of-two weight scales,
# per-point block-floating-point gradient scales): fp32-class accuracy at the bf16x3 speed, for inference and for all three training GEMM kernels
# of both model families.
# "f16x2" (round 5): INFERENCE only -- the split-fp16 kernel with two products per weight (W_hi x_hi + W_lo x_hi: activations enter with
# fp16's 11 bits, weights keep 22), a third fewer MFMAs than "f16x3"; whole frames stay within 1e-4 dB PSNR of the reference (measured
# 2e-6 .. 5.6e-5 dB, median 9e-6, over 21 frames), per-point outputs carry 2^-12 relative rounding.  A training step under "f16x2" raises (train with "f16x3").
_VALID_PRECISIONS = ("f32", "bf16x3", "f16x3", "f16x2")
F16_MODES = ("f16x3", "f16x2")           # arithmetics that run on the scaled fp16 weight stream (range probe + range flag apply)
INFERENCE_ONLY_PRECISIONS = ("f16x2",)
_mlp_precision = os.environ.get("NERFACE_MLP_PRECISION", "f32")


def set_mlp_precision(mode: str) -> None:
    global _mlp_precision
    if mode not in _VALID_PRECISIONS:
        raise ValueError(f"precision must be one of {_VALID_PRECISIONS}")
    _mlp_precision = mode


def get_mlp_precision() -> str:
    return _mlp_precision


def _c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    return t if t.is_contiguous() else t.contiguous()


# ---------------------------------------------------------------------------------------- tables
_LINSPACE_CACHE = {}


def linspace01(n: int, device) -> torch.Tensor:
    """torch.linspace(0, 1, n) as the reference calls it (T:50-55, H:357-360).  The table is produced by
    torch's own CPU kernel once per (n, device) and cached on the device, so that the deterministic
    depths / CDF abscissae carry exactly torch's rounding."""
    key = (int(n), str(device))
    t = _LINSPACE_CACHE.get(key)
    if t is None:
        t = torch.linspace(0.0, 1.0, int(n), dtype=torch.float32).to(device)
        _LINSPACE_CACHE[key] = t
    return t


# ---------------------------------------------------------------------------------------- K1
def ray_bundle(height: int, width: int, fx: float, fy: float, cx: float, cy: float, c2w: torch.Tensor):
    c2w = c2w if (c2w.dtype == torch.float32 and c2w.stride(-1) == 1) else c2w.to(torch.float32).contiguous()
    if not c2w.is_cuda:
        raise RuntimeError("get_ray_bundle (MI355X build): tform_cam2world must be on a ROCm device")
    if c2w.dim() != 2 or c2w.shape[0] < 3 or c2w.shape[1] < 4:
        raise ValueError("tform_cam2world must be (3|4, 4)")
    dev = c2w.device
    ro = torch.empty((height, width, 3), dtype=torch.float32, device=dev)
    rd = torch.empty((height, width, 3), dtype=torch.float32, device=dev)
    # W*cx and H*cy are formed in double and rounded once, as python-scalar operands are in the reference
    cx_w = float(np.float32(np.float64(width) * np.float64(cx)))
    cy_h = float(np.float32(np.float64(height) * np.float64(cy)))
    with torch.cuda.device(dev):
        H.check(H.lib().nf_ray_bundle(height, width, float(np.float32(fx)), float(np.float32(fy)), cx_w, cy_h,
                                      H.ptr(c2w), int(c2w.stride(0)), H.ptr(ro), H.ptr(rd), H.stream_ptr(dev)),
                "nf_ray_bundle")
    return ro, rd


# ---------------------------------------------------------------------------------------- K0
def weighted_choice(weights: torch.Tensor, n: int, u: Optional[torch.Tensor] = None, check: bool = False) -> torch.Tensor:
    """np.random.choice(len(weights), size=n, replace=False, p=weights / weights.sum()) on the device (TR:320-322): n distinct int64
    indices in ascending order (a seed reproduces the batch element for element).  u: the uniform numbers to use (len(weights), in [0, 1)); default torch.rand on the device, i.e.
    torch's generator and seeds.  check=True reads the "fewer than n positive weights" flag back (host sync) and raises ValueError
    like numpy does."""
    w = _c(weights.reshape(-1))
    dev = H.require_device(w)
    n_items = int(w.numel())
    if not 0 <= n <= n_items:
        raise ValueError("Cannot take a larger sample than population when replace is False")
    if u is None:
        u = torch.rand(n_items, dtype=torch.float32, device=dev)
    u = _c(u.reshape(-1))
    H.require_device(u)
    if u.numel() != n_items:
        raise ValueError("u must hold one uniform number per weight")
    lib = H.lib()
    ws_bytes = int(lib.nf_weighted_choice_workspace_bytes())
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    idx = torch.empty(n, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        H.check(lib.nf_weighted_choice(H.ptr(w), H.ptr(u), n_items, int(n), H.ptr(idx), H.ptr(ws), ws_bytes, H.stream_ptr(dev)),
                "nf_weighted_choice")
    if check and n > 0 and int(ws[5].item()):
        raise ValueError("Fewer non-zero entries in p than size")
    return idx


class _SelectedBackground(torch.autograd.Function):
    """bg (n, 3) = background (H, W, 3) at the selected pixels, as nf_ray_batch gathered it; the backward scatters the cotangent
    back into a zero image (a pixel selected twice accumulates).  What makes a learned background (`train_background`, TR:143-157)
    reachable through get_ray_batch; a pixel outside the image (ray_batch's out-of-range flag) receives nothing."""

    @staticmethod
    def forward(ctx, background, sel, bg):
        ctx.save_for_backward(sel)
        ctx.hw = tuple(background.shape[:2])
        return bg.view_as(bg)

    @staticmethod
    def backward(ctx, g):
        (sel,) = ctx.saved_tensors
        h, w = ctx.hw
        row, col = (torch.div(sel, w, rounding_mode="floor"), sel % w) if sel.dim() == 1 else (sel[:, 0], sel[:, 1])
        ok = (row >= 0) & (row < h) & (col >= 0) & (col < w) if sel.dim() == 2 else (sel >= 0) & (sel < h * w)
        d = torch.zeros((h, w, 3), dtype=g.dtype, device=g.device)
        d.index_put_((row.clamp(0, h - 1), col.clamp(0, w - 1)), g * ok[:, None].to(g.dtype), accumulate=True)
        return d, None, None


def ray_batch(height: int, width: int, fx: float, fy: float, cx: float, cy: float, c2w: torch.Tensor, sel: torch.Tensor,
              image: Optional[torch.Tensor] = None, background: Optional[torch.Tensor] = None, check: bool = False):
    """Rays of the selected pixels only (sel (n, 2) int64 {row, col}, or (n,) flat pixel indices row * W + col) -- bit-identical to
    get_ray_bundle(...)[sel[:, 0], sel[:, 1]]
    -- plus the target pixels of `image` (H, W, C) and the background prior (H, W, 3) at the same pixels, in one launch
    (TR:302, 325-330).  Returns (ro, rd, target | None, bg | None).  check=True reads the out-of-range flag back (host sync)."""
    c2w = c2w if (c2w.dtype == torch.float32 and c2w.stride(-1) == 1) else c2w.to(torch.float32).contiguous()
    if sel.dtype != torch.int64 or not (sel.dim() == 1 or (sel.dim() == 2 and sel.shape[1] == 2)):
        raise ValueError("sel must be an (n, 2) int64 tensor of {row, col} or an (n,) int64 tensor of flat pixel indices")
    sel, image, background = sel.contiguous(), _c(image), _c(background)
    dev = H.require_device(c2w, image, background)
    if sel.device != dev:
        raise RuntimeError("ray_batch: select_inds must live on the device of the pose")
    n = int(sel.shape[0])
    if image is not None and (image.dim() != 3 or tuple(image.shape[:2]) != (height, width) or image.dtype != torch.float32):
        raise ValueError("image must be a float32 (H, W, C) tensor")
    if background is not None and (tuple(background.shape) != (height, width, 3) or background.dtype != torch.float32):
        raise ValueError("background must be a float32 (H, W, 3) tensor")
    ch = int(image.shape[2]) if image is not None else 0
    ro = torch.empty((n, 3), dtype=torch.float32, device=dev)
    rd = torch.empty((n, 3), dtype=torch.float32, device=dev)
    target = torch.empty((n, ch), dtype=torch.float32, device=dev) if image is not None else None
    bg = torch.empty((n, 3), dtype=torch.float32, device=dev) if background is not None else None
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    cx_w = float(np.float32(np.float64(width) * np.float64(cx)))
    cy_h = float(np.float32(np.float64(height) * np.float64(cy)))
    with torch.cuda.device(dev):
        H.check(H.lib().nf_ray_batch(height, width, float(np.float32(fx)), float(np.float32(fy)), cx_w, cy_h, H.ptr(c2w),
                                     int(c2w.stride(0)), H.ptr(sel), 1 if sel.dim() == 1 else 0, n, H.ptr(image), ch, H.ptr(background),
                                     H.ptr(ro), H.ptr(rd),
                                     H.ptr(target), H.ptr(bg), H.ptr(flag), H.stream_ptr(dev)), "nf_ray_batch")
    if check and int(flag.item()):
        raise IndexError("ray_batch: a selected pixel lies outside the image")
    if background is not None and background.requires_grad and torch.is_grad_enabled():
        bg = _SelectedBackground.apply(background, sel, bg)
    return ro, rd, target, bg


# ---------------------------------------------------------------------------------------- K2
def sample_coarse(n_rays: int, n_coarse: int, near: float, far: float, device, t_rand: Optional[torch.Tensor] = None,
                  lindisp: bool = False):
    """T:56-76: stratified depths (n_rays, n_coarse); lindisp = the reference's linear-in-disparity spacing (T:65-66)."""
    t_rand = _c(t_rand)
    tv = linspace01(n_coarse, device)
    z = torch.empty((n_rays, n_coarse), dtype=torch.float32, device=device)
    if t_rand is not None:
        H.require_device(t_rand)
        assert tuple(t_rand.shape) == (n_rays, n_coarse)
    with torch.cuda.device(device):
        H.check(H.lib().nf_sample_coarse_ex(n_rays, n_coarse, float(np.float32(near)), float(np.float32(far)), H.ptr(tv),
                                            H.ptr(t_rand), 1 if lindisp else 0, H.ptr(z), H.stream_ptr(device)), "nf_sample_coarse_ex")
    return z


# ---------------------------------------------------------------------------------------- K3
def posenc(x: torch.Tensor, n_freq: int, include_input: bool) -> torch.Tensor:
    x = _c(x)
    dev = H.require_device(x)
    dim = x.shape[-1]
    rows = x.numel() // dim if dim else 0
    width = dim * ((1 if include_input else 0) + 2 * n_freq)
    out = torch.empty(tuple(x.shape[:-1]) + (width,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        H.check(H.lib().nf_posenc(H.ptr(x), rows, dim, n_freq, 1 if include_input else 0, H.ptr(out), H.stream_ptr(dev)),
                "nf_posenc")
    return out


# ---------------------------------------------------------------------------------------- K4
class MLPFamily(NamedTuple):
    """What tells the fused NeRFace MLP families apart.  Every entry point of a family is `<prefix>_<name>`, with one C
    signature per name for all families (include/nerface_hip.h)."""
    prefix: str                 # "nf_paper" / "nf_lcode" / "nf_smaller" / "nf_bshape" / "nf_cbshape"
    keys: tuple                 # parameter names, in the order of the ABI's parameter-pointer arrays and gradient images
    hidden: tuple               # [lo, hi) of the hidden-activation sections of the exact-f32 `saved` buffer, in floats per point
    none_grads: tuple           # gradient slots autograd leaves None
    exact_dw: bool              # the split-bf16 backward takes (exact_dw, saved_f32)
    precisions: tuple = _VALID_PRECISIONS   # the arithmetics of nerf.set_mlp_precision the family has kernels for

    def require_precision(self, precision: str) -> None:
        """A family without kernels for `precision` refuses it by name -- before anything is packed or launched."""
        if precision not in self.precisions:
            raise NotImplementedError(f'the {self.prefix} model family has no "{precision}" kernels (it serves '
                                      f'{", ".join(repr(p) for p in self.precisions)}): use nerf.set_mlp_precision("f32")')

    def fn(self, name: str):
        return getattr(H.lib(), f"{self.prefix}_{name}")

    def call(self, name: str, *args) -> None:
        """Launch `<prefix>_<name>(*args)`; a non-zero return code raises RuntimeError."""
        H.check(self.fn(name)(*args), f"{self.prefix}_{name}")


PAPER = MLPFamily("nf_paper", tuple(PAPER_KEYS),
                  (64, 2240),           # S_H0 .. S_DIRF (csrc/nf_mlp_layout.h): h0 .. h5, fc_feat, layers_dir.0 .. 2
                  (22, 23),             # layers_dir.3 exists in every checkpoint but is never used (Quirk Q3)
                  True)
LCODE = MLPFamily("nf_lcode", tuple(LCODE_KEYS),
                  (64, 1472),           # S_L1 .. S_DIRF (csrc/nf_mlp_lcode_layout.h): layer1, layers_xyz.0 .. 2, fc_feat, layers_dir.0
                  (), False)
SMALLER = MLPFamily("nf_smaller", tuple(SMALLER_KEYS),
                    (64, 1984),         # S_H0 .. S_DIRF (csrc/nf_mlp_smaller_layout.h): h0 .. h4, fc_feat, layers_dir.0 .. 2
                    (), False,
                    ("f32",))           # exact f32 only: the split arithmetics are not built for this family

# the two blendshape classes without a learnable code: the second family's per-point kernels and buffer layouts (so its `hidden`
# range), their own pack tables, bias table and gradient scatter (csrc/nf_mlp_bshape.hip, csrc/nf_mlp_cbshape.hip)
BSHAPE = MLPFamily("nf_bshape", tuple(BSHAPE_KEYS), LCODE.hidden, (), False)
CBSHAPE = MLPFamily("nf_cbshape", tuple(CBSHAPE_KEYS), LCODE.hidden, (), False)

# Packed weight images are cached per (parameter storage, version counter, PACK EPOCH).  The version counter follows ordinary
# in-place updates (optimizer.step() of the default / foreach optimizers, load_state_dict, copy_ under no_grad) -- but NOT every
# writer bumps it: torch's FUSED optimizers (Adam(fused=True)), writes through `p.data` and c10d collectives leave it untouched.
# So every run_one_iter_of_nerf / run_one_iter_of_tinynerf call advances the pack epoch: the images are rebuilt once per
# rendered frame or training step (a few 10-microsecond kernels), and a stale image can never outlive one call.
_PACK_EPOCH = [0]


def bump_pack_epoch() -> None:
    _PACK_EPOCH[0] += 1


def pack_epoch() -> int:
    return _PACK_EPOCH[0]


class MLPWeights:
    """Kernel-ready images of one fused model of `family` on one device, one per kind, each re-packed whenever a parameter's
    version counter or the pack epoch moves (i.e. after optimizer.step() / load_state_dict() / a new frame or step):
      f32 / f32_t      fragment-ordered f32 image for the forward / transposed image for the backward chain
      bf16 / bf16_t    (hi, lo) bf16 streams of the split-bf16 forward / chain
      f16 / f16_t      (hi, lo) fp16 streams + per-layer scales of the split-fp16 forward / chain."""

    # kind -> (size entry point, pack entry point, element dtype); names after the family prefix
    _KINDS = {
        "f32": ("packed_floats", "pack", torch.float32),
        "f32_t": ("packed_bwd_floats", "pack_bwd", torch.float32),
        "bf16": ("packed_bf16_bytes", "pack_bf16", torch.uint8),
        "bf16_t": ("packed_bwd_bf16_bytes", "pack_bwd_bf16", torch.uint8),
        "f16": ("packed_f16_bytes", "pack_f16", torch.uint8),
        "f16_t": ("packed_bwd_f16_bytes", "pack_bwd_f16", torch.uint8),
    }

    def __init__(self, family: MLPFamily, params: Sequence[torch.Tensor]):
        assert len(params) == len(family.keys)
        self.family = family
        self._params = list(params)
        self._cache = {}                # kind -> (signature, buffer)
        self._f16_sticky = None         # range-guard flag of the split-fp16 forward carried across re-packs (0-d int32 on the device)

    def invalidate(self) -> None:
        """Drop every cached image.  The caches follow in-place updates through the parameters' version counters
        (optimizer.step(), load_state_dict(), copy_ under no_grad); writes that bypass the counter -- through `p.data`, or by
        a collective -- are NOT seen: call this (or model.hip_weights().invalidate()) after such a write."""
        for kind, (_, buf) in list(self._cache.items()):
            self._cache[kind] = (None, buf)

    def _signature(self):
        return (_PACK_EPOCH[0],) + tuple((int(p.data_ptr()), int(p._version)) for p in self._params)

    def _get(self, kind: str) -> torch.Tensor:
        sig = self._signature()
        hit = self._cache.get(kind)
        if hit is None or hit[0] != sig:
            size_fn, pack_fn, dtype = self._KINDS[kind]
            dev = H.require_device(*[p.detach() for p in self._params])
            buf = hit[1] if hit is not None and hit[1].device == dev else torch.empty(self.family.fn(size_fn)(), dtype=dtype, device=dev)
            if kind == "f16" and hit is not None and hit[1] is buf:
                # packing clears the stream's range-guard flag: carry it over first (one tiny device op, no host sync), so that a
                # training run polled every print_every iterations still sees an overflow of any iteration in between
                if self._f16_sticky is None or self._f16_sticky.device != dev:
                    self._f16_sticky = torch.zeros((), dtype=torch.int32, device=dev)
                off = self.family.fn("f16_flag_offset")()
                self._f16_sticky.bitwise_or_(buf[off:off + 4].view(torch.int32)[0])
            arr = (C.c_void_p * len(self._params))(*[int(p.data_ptr()) for p in self._params])
            with torch.cuda.device(dev):
                self.family.call(pack_fn, arr, H.ptr(buf), H.stream_ptr(dev))
            self._cache[kind] = (sig, buf)
        return self._cache[kind][1]

    def get(self) -> torch.Tensor:
        return self._get("f32")

    def get_bound(self) -> torch.Tensor:
        """The sigma-bound image of get() (csrc/nf_mlp_gated.hip): built from the f32 image by one small kernel, cached under that
        image's signature and so rebuilt exactly when the image is."""
        packed = self._get("f32")
        sig = self._cache["f32"][0]
        hit = self._cache.get("bound")
        if hit is None or hit[0] != sig or hit[1].device != packed.device:
            self._cache["bound"] = hit = (sig, sigma_bound(self.family, packed))
        return hit[1]

    def get_t(self) -> torch.Tensor:
        return self._get("f32_t")

    def get_bf16(self) -> torch.Tensor:
        return self._get("bf16")

    def get_bf16_t(self) -> torch.Tensor:
        return self._get("bf16_t")

    def get_f16(self) -> torch.Tensor:
        return self._get("f16")

    def get_f16_t(self) -> torch.Tensor:
        return self._get("f16_t")

    def f16_range_flag(self) -> Optional[torch.Tensor]:
        """0-d int32 device tensor: non-zero once a split-fp16 forward of this model produced a non-finite output (an activation
        left fp16's range) -- with the current stream or, carried over the re-packs of a training run, with any earlier one.
        None if the split-fp16 stream was never built."""
        hit = self._cache.get("f16")
        if hit is None:
            return None
        off = self.family.fn("f16_flag_offset")()
        flag = hit[1][off:off + 4].view(torch.int32)[0]
        return flag if self._f16_sticky is None else torch.bitwise_or(flag, self._f16_sticky)


def check_conditioning(expr: torch.Tensor, latent: torch.Tensor) -> None:
    """The conditioning kernels read expr[0..75] and latent[0..31] unconditionally: refuse other sizes before any launch."""
    if expr.numel() != 76 or latent.numel() != 32:
        raise ValueError("expected a 76-d expression and a 32-d latent code")


def mlp_condition(fam: MLPFamily, packed, expr, latent, near: float, far: float) -> torch.Tensor:
    """The per-call bias table of `fam` for one expression, latent code and near / far."""
    expr, latent = _c(expr.detach()), _c(latent.detach())
    dev = H.require_device(packed, expr, latent)
    check_conditioning(expr, latent)
    cond = torch.empty(fam.fn("cond_floats")(), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        fam.call("condition", H.ptr(packed), H.ptr(expr), H.ptr(latent), float(np.float32(near)), float(np.float32(far)), H.ptr(cond),
                 H.stream_ptr(dev))
    return cond


_FWD_ENTRY = {"f32": "mlp_fwd", "bf16x3": "mlp_fwd_bf16", "f16x3": "mlp_fwd_f16", "f16x2": "mlp_fwd_f16x2"}


def mlp_fwd(fam: MLPFamily, precision: str, packed, cond, ro, rd, z, rd_view=None) -> torch.Tensor:
    """Inference forward of `fam` in arithmetic `precision` -> raw (n_rays, n_samples, 4).  `packed` is the image of that arithmetic:
    MLPWeights.get() for "f32", get_bf16() for "bf16x3", get_f16() for "f16x3" and "f16x2" (one image serves both)."""
    dev = H.require_device(packed if precision == "f32" else None, cond, ro, rd, z, rd_view)
    n_rays, n_samples = z.shape
    raw = torch.empty((n_rays, n_samples, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        fam.call(_FWD_ENTRY[precision], H.ptr(packed), H.ptr(cond), H.ptr(ro), H.ptr(rd), H.ptr(rd_view), H.ptr(z), n_rays, n_samples,
                 H.ptr(raw), H.stream_ptr(dev))
    return raw


# Colour layers on live samples only (csrc/nf_mlp_live.hip): the exact-f32 inference forward of the families in LIVE_FAMILIES with
# layers_dir.0 .. fc_rgb run only where the integrator can see the colour.  raw[..., 3] is mlp_fwd's everywhere, raw[..., :3] is
# mlp_fwd's on live points (!(sigma <= 0), or the last sample of a ray) and 0.0 on the others -- so volume_render_fwd WITHOUT noise
# gives the same outputs bit for bit, and that is the only caller it serves (_RenderChunk.forward).  Which passes of a render take the
# kernel is a module switch: LIVE_PASSES_DEFAULT is what measured faster than the full kernel per launch and on whole frames
# (profiles/live_colour_fill.md; before the holes were filled in place the fine pass did not gain: profiles/live_colour.md);
# set_live_colour(True) turns it on for both passes, set_live_colour(False) off (A/B tests, tools/time_live_colour.py).
# live_colour_launches() counts the launches of the kernel.
LIVE_FAMILIES = ("nf_paper",)
LIVE_PASSES_DEFAULT = ("coarse", "fine")   # fine pass (live fraction 0.74 .. 0.88): -1.2 ms of 85.4 ms per launch
_live_passes = set(LIVE_PASSES_DEFAULT)
_live_launches = [0]
_LIVE_SCRATCH = {}                      # (device, stream, max_workgroups) -> the waves' rings of gathered rows
# The kernel's schedule constants (csrc/nf_mlp_live.hip), stated once for the host model of the schedule (tests/live_schedule_ref.py):
# a wave's ring in `scratch` has LIVE_RING_ROWS rows of LIVE_ROW_BYTES (feat 1 KiB + direction fragments 64 B + index and sigma 16 B),
# four waves per workgroup -- mlp_fwd_live_scratch_floats(w) == w * 4 * LIVE_RING_ROWS * LIVE_ROW_BYTES // 4; at most 31 rows are in
# use.  LIVE_PREFETCH_ROWS oldest rows are requested while fc_alpha's row runs; holes beyond that are loaded behind the ballot.
LIVE_RING_ROWS = 64
LIVE_ROW_BYTES = 1024 + 64 + 16
LIVE_PREFETCH_ROWS = 8


# The FORMER static order of the kernel, kept for the host model of that order (tests/live_schedule_ref.py): the kernel now hands out
# 32-point units from a counter, in the order the waves come for them (tools/live_schedule_sim.py replays both).
def live_rotation_step(workgroups: int) -> int:
    """Pass k of workgroup b of G took block k G + (b + k step) mod G."""
    step = (workgroups * 5 // 13) | 1
    return step if step < workgroups else 0


def set_live_colour(on, passes=("coarse", "fine")) -> None:
    """on=True: the passes named take the kernel; on=False: none does; on=None: back to LIVE_PASSES_DEFAULT.  An explicit choice
    (True / False) is a choice of THIS kernel or of the full one: no pass takes the gated kernel (set_sigma_gate) until it is
    switched on again; None restores that kernel's default passes too."""
    global _live_passes, _gated_passes
    _live_passes = set(LIVE_PASSES_DEFAULT) if on is None else (set(passes) if on else set())
    _gated_passes = set(GATED_PASSES_DEFAULT) if on is None else set()


def live_colour_kernel(fam: MLPFamily) -> bool:
    """The arithmetic is exact f32 and `fam` has the kernel."""
    return _mlp_precision == "f32" and fam.prefix in LIVE_FAMILIES


def live_colour_applies(fam: MLPFamily, which: str) -> bool:
    """Pass `which` ("coarse" / "fine") of a render without noise takes the kernel: switched on for it, and live_colour_kernel."""
    return which in _live_passes and live_colour_kernel(fam)


def live_colour_launches() -> int:
    return _live_launches[0]


def mlp_fwd_live(fam: MLPFamily, packed, cond, ro, rd, z, rd_view=None, max_workgroups: int = 0) -> torch.Tensor:
    """mlp_fwd(fam, "f32", ...) with zero colour on the dead points (see above) -> raw (n_rays, n_samples, 4).  max_workgroups > 0
    caps the persistent grid (tests: a wave then walks many blocks and its ring wraps)."""
    if fam.prefix not in LIVE_FAMILIES:
        raise NotImplementedError(f"the {fam.prefix} model family has no live-colour kernel")
    dev = H.require_device(packed, cond, ro, rd, z, rd_view)
    n_rays, n_samples = z.shape
    raw = torch.empty((n_rays, n_samples, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        key = (dev, H.stream_ptr(dev), int(max_workgroups))
        scratch = _LIVE_SCRATCH.get(key)
        if scratch is None:
            scratch = _LIVE_SCRATCH[key] = torch.empty(fam.fn("mlp_fwd_live_scratch_floats")(int(max_workgroups)), dtype=torch.float32, device=dev)
        fam.call("mlp_fwd_live", H.ptr(packed), H.ptr(cond), H.ptr(ro), H.ptr(rd), H.ptr(rd_view), H.ptr(z), n_rays, n_samples, H.ptr(raw),
                 H.ptr(scratch), scratch.numel(), int(max_workgroups), H.stream_ptr(dev))
    _live_launches[0] += 1
    return raw


# what a wave did, then where its passes spent their shader clocks (sums over the wave's passes; csrc/nf_mlp_live_kernel.h, nf_live_mark)
LIVE_PHASE_COLUMNS = ("clk_trunk", "clk_lone_tile", "clk_append", "clk_run_entry", "clk_run", "clk_dead_stores")
LIVE_STAT_COLUMNS = ("units", "colour_runs", "flush_rows", "exit_clock") + LIVE_PHASE_COLUMNS


def mlp_fwd_live_stats(fam: MLPFamily, packed, cond, ro, rd, z, rd_view=None, max_workgroups: int = 0):
    """mlp_fwd_live through the kernel's statistics instantiation (csrc/nf_mlp_live_stats.hip) -> (raw, stats): stats is int64
    (waves, 10) in the order of LIVE_STAT_COLUMNS, one row per wave of the capped grid (workgroup * 4 + wave; rows of workgroups the
    launch did not start stay zero); exit_clock is the device's wall_clock64() when the wave left, the clk_ columns are shader clocks.  An instrument for tests and
    profiles (tools/live_schedule_sim.py); no render path calls it."""
    if fam.prefix not in LIVE_FAMILIES:
        raise NotImplementedError(f"the {fam.prefix} model family has no live-colour kernel")
    dev = H.require_device(packed, cond, ro, rd, z, rd_view)
    n_rays, n_samples = z.shape
    raw = torch.empty((n_rays, n_samples, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        scratch = torch.empty(fam.fn("mlp_fwd_live_scratch_floats")(int(max_workgroups)), dtype=torch.float32, device=dev)
        waves = scratch.numel() * 4 // (LIVE_RING_ROWS * LIVE_ROW_BYTES)
        stats = torch.empty((waves, len(LIVE_STAT_COLUMNS)), dtype=torch.int64, device=dev)
        fam.call("mlp_fwd_live_phases", H.ptr(packed), H.ptr(cond), H.ptr(ro), H.ptr(rd), H.ptr(rd_view), H.ptr(z), n_rays, n_samples,
                 H.ptr(raw), H.ptr(scratch), scratch.numel(), int(max_workgroups), stats.data_ptr(), waves, H.stream_ptr(dev))
    return raw, stats


# fc_feat, too, only where it is needed (csrc/nf_mlp_gated.hip): the live-colour kernel with the trunk ended behind layers_xyz.5.  A
# bound on the density, a 256-term dot product on relu(layers_xyz.5) (DESIGN.md "Sigma gate"), proves most samples without density
# dead; fc_feat, fc_alpha and the colour layers run on the others.  Against mlp_fwd: all four channels bit for bit where
# !(sigma <= 0) or on a ray's last sample; elsewhere rgb 0.0 and sigma either mlp_fwd's or SOME NEGATIVE NUMBER -- so, again,
# volume_render_fwd without noise gives the same outputs bit for bit.  A pass in GATED_PASSES_DEFAULT takes this kernel in front of
# the live-colour one; the default is what measured faster than the live kernel on every frame, by more than that kernel's own spread.
# (profiles/sigma_gate_fine.md) coarse (kept 0.27 .. 0.58): -1.2 .. -2.4 ms of 26 ms; fine (kept 0.75 .. 0.89): -0.26 .. -1.77 ms of 83 ms
GATED_PASSES_DEFAULT = ("coarse", "fine")
# NERFACE_SIGMA_GATE="coarse,fine" (or one of them, or "") sets the passes for a process whose code one does not edit (bench.py)
_gated_passes = (set(GATED_PASSES_DEFAULT) if os.environ.get("NERFACE_SIGMA_GATE") is None
                 else {p for p in os.environ["NERFACE_SIGMA_GATE"].split(",") if p in ("coarse", "fine")})
_gated_launches = [0]
GATED_STAT_COLUMNS = LIVE_STAT_COLUMNS[:4] + ("proven_rows",) + LIVE_PHASE_COLUMNS


def set_sigma_gate(on, passes=("coarse", "fine")) -> None:
    """on=True: the passes named take the gated kernel; on=False: none does; on=None: back to GATED_PASSES_DEFAULT."""
    global _gated_passes
    _gated_passes = set(GATED_PASSES_DEFAULT) if on is None else (set(passes) if on else set())


def sigma_gate_applies(fam: MLPFamily, which: str) -> bool:
    """Pass `which` of a render without noise takes the gated kernel: switched on for it, under live_colour_kernel's conditions."""
    return which in _gated_passes and live_colour_kernel(fam)


def live_mode(fam: MLPFamily, which: str):
    """What a pass `which` without noise and without gradient passes to hip_forward(live_only=...): "gated", True (live) or False."""
    if sigma_gate_applies(fam, which):
        return "gated"
    return live_colour_applies(fam, which)


def sigma_gate_launches() -> int:
    return _gated_launches[0]


def sigma_bound(fam: MLPFamily, packed) -> torch.Tensor:
    """The sigma-bound image of the packed f32 image `packed` (MLPWeights.get_bound() caches it beside the image)."""
    if fam.prefix not in LIVE_FAMILIES:
        raise NotImplementedError(f"the {fam.prefix} model family has no gated kernel")
    dev = H.require_device(packed)
    bound = torch.empty(fam.fn("sigma_bound_floats")(), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        fam.call("sigma_bound", H.ptr(packed), H.ptr(bound), H.stream_ptr(dev))
    return bound


def _gated_call(entry, fam, packed, bound, cond, ro, rd, z, rd_view, max_workgroups, scratch, raw, *tail):
    n_rays, n_samples = z.shape
    fam.call(entry, H.ptr(packed), H.ptr(bound), H.ptr(cond), H.ptr(ro), H.ptr(rd), H.ptr(rd_view), H.ptr(z), n_rays, n_samples, H.ptr(raw),
             H.ptr(scratch), scratch.numel(), int(max_workgroups), *tail)


def mlp_fwd_gated(fam: MLPFamily, packed, bound, cond, ro, rd, z, rd_view=None, max_workgroups: int = 0) -> torch.Tensor:
    """mlp_fwd_live with fc_feat, too, only on the samples `bound` (sigma_bound(fam, packed)) cannot prove dead (see above) ->
    raw (n_rays, n_samples, 4)."""
    if fam.prefix not in LIVE_FAMILIES:
        raise NotImplementedError(f"the {fam.prefix} model family has no gated kernel")
    dev = H.require_device(packed, bound, cond, ro, rd, z, rd_view)
    n_rays, n_samples = z.shape
    raw = torch.empty((n_rays, n_samples, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        key = (dev, H.stream_ptr(dev), int(max_workgroups))
        scratch = _LIVE_SCRATCH.get(key)
        if scratch is None:
            scratch = _LIVE_SCRATCH[key] = torch.empty(fam.fn("mlp_fwd_live_scratch_floats")(int(max_workgroups)), dtype=torch.float32, device=dev)
        _gated_call("mlp_fwd_gated", fam, packed, bound, cond, ro, rd, z, rd_view, max_workgroups, scratch, raw, H.stream_ptr(dev))
    _gated_launches[0] += 1
    return raw


def mlp_fwd_gated_stats(fam: MLPFamily, packed, bound, cond, ro, rd, z, rd_view=None, max_workgroups: int = 0):
    """mlp_fwd_gated through the kernel's statistics instantiation -> (raw, stats): stats is int64 (waves, 11) in the order of
    GATED_STAT_COLUMNS (mlp_fwd_live_stats' columns, a gathered run counting as a colour run, with the rows the wave proved dead in
    front of the clocks)."""
    if fam.prefix not in LIVE_FAMILIES:
        raise NotImplementedError(f"the {fam.prefix} model family has no gated kernel")
    dev = H.require_device(packed, bound, cond, ro, rd, z, rd_view)
    n_rays, n_samples = z.shape
    raw = torch.empty((n_rays, n_samples, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        scratch = torch.empty(fam.fn("mlp_fwd_live_scratch_floats")(int(max_workgroups)), dtype=torch.float32, device=dev)
        waves = scratch.numel() * 4 // (LIVE_RING_ROWS * LIVE_ROW_BYTES)
        stats = torch.empty((waves, len(GATED_STAT_COLUMNS)), dtype=torch.int64, device=dev)
        _gated_call("mlp_fwd_gated_phases", fam, packed, bound, cond, ro, rd, z, rd_view, max_workgroups, scratch, raw, stats.data_ptr(), waves,
                    H.stream_ptr(dev))
    return raw, stats


_SIGMA_ENTRY = {"f32": "mlp_sigma", "bf16x3": "mlp_sigma_bf16", "f16x3": "mlp_sigma_f16", "f16x2": "mlp_sigma_f16x2"}


def mlp_sigma(fam: MLPFamily, precision: str, image, cond, ro, rd, z) -> torch.Tensor:
    """Density-only inference forward of `fam` in arithmetic `precision` -> raw sigma (n_rays, n_samples), bit for bit
    mlp_fwd(...)[..., 3]: the same kernel up to and including the layer that yields the density, nothing after it.  `image` as for
    mlp_fwd.  The direction does not reach the density, so there is no rd_view."""
    dev = H.require_device(image if precision == "f32" else None, cond, ro, rd, z)
    n_rays, n_samples = z.shape
    sigma = torch.empty((n_rays, n_samples), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        fam.call(_SIGMA_ENTRY[precision], H.ptr(image), H.ptr(cond), H.ptr(ro), H.ptr(rd), 0, H.ptr(z), n_rays, n_samples, H.ptr(sigma),
                 H.stream_ptr(dev))
    return sigma


def mlp_fwd_train(fam: MLPFamily, packed, cond, ro, rd, z, rd_view=None, packed_b=None, packed_h=None):
    """Training forward of `fam`: returns (raw, (saved,)) where `saved` holds every layer output for the backward.
    packed_b (split-bf16 stream) or packed_h (split-fp16 stream) given -> the forward runs on that split kernel and `saved`
    additionally carries its ReLU bit masks; the matching backward is mlp_bwd(..., split=True / "f16")."""
    dev = H.require_device(packed, cond, ro, rd, z, rd_view)
    n_rays, n_samples = z.shape
    raw = torch.empty((n_rays, n_samples, 4), dtype=torch.float32, device=dev)
    saved = torch.empty(fam.fn("saved_floats")(n_rays * n_samples), dtype=torch.float32, device=dev)
    entry, image = (("mlp_fwd_train_f16", packed_h) if packed_h is not None else
                    ("mlp_fwd_train_bf16", packed_b) if packed_b is not None else ("mlp_fwd_train", packed))
    with torch.cuda.device(dev):
        fam.call(entry, H.ptr(image), H.ptr(cond), H.ptr(ro), H.ptr(rd), H.ptr(rd_view), H.ptr(z), n_rays, n_samples, H.ptr(raw),
                 H.ptr(saved), H.stream_ptr(dev))
    return raw, (saved,)


def mlp_bwd(fam: MLPFamily, weights: MLPWeights, packed, cond, z, d_raw, saved_t, split=False, exact_dw=False):
    """d_raw (n_rays, n_samples, 4) -> ([parameter gradients in fam.keys order, None in fam.none_grads], d_latent (32)).
    saved_t: the `saved` buffer of the matching training forward.
    split=True runs the dX chain on the split-bf16 kernel (requires `saved` from the split-bf16 training forward) and, unless
    exact_dw (paper family only), the dW GEMMs too; split="f16" runs both on the split-fp16 kernels."""
    if exact_dw and not fam.exact_dw:
        raise ValueError(f"exact_dw: the split-bf16 backward of {fam.prefix} has no exact-f32 weight-gradient form")
    d_raw = _c(d_raw)
    dev = H.require_device(packed, cond, saved_t, d_raw)
    n_rays, n_samples = z.shape
    with torch.cuda.device(dev):             # the slice plan behind the size depends on the CURRENT device's CU count (nf_mlp_dw.h): ask on `dev`
        ws_floats = fam.fn("bwd_workspace_floats")(n_rays * n_samples)
    ws = torch.empty(ws_floats, dtype=torch.float32, device=dev)
    flat = torch.empty(fam.fn("grad_floats")(), dtype=torch.float32, device=dev)
    args = (H.ptr(cond), H.ptr(saved_t), H.ptr(d_raw), n_rays, n_samples, H.ptr(ws), ws_floats, H.ptr(flat))
    with torch.cuda.device(dev):
        if split == "f16":
            fam.call("mlp_bwd_f16", H.ptr(packed), H.ptr(weights.get_f16_t()), *args, H.stream_ptr(dev))
        elif split:
            packed_bt, exact = weights.get_bf16_t(), ()
            if fam.exact_dw:
                saved_f32 = split_saved_to_f32(saved_t, n_rays * n_samples, False) if exact_dw else None   # the exact GEMMs read f32 rows
                exact = (int(bool(exact_dw)), H.ptr(saved_f32))
            fam.call("mlp_bwd_bf16", H.ptr(packed), H.ptr(packed_bt), *args, *exact, H.stream_ptr(dev))
        else:
            fam.call("mlp_bwd", H.ptr(packed), H.ptr(weights.get_t()), *args, H.stream_ptr(dev))
    grads, off = [], 0
    for i, p in enumerate(weights._params):
        n = p.numel()
        grads.append(None if i in fam.none_grads else flat[off:off + n].view(p.shape))
        off += n
    return grads, flat[off:off + 32]


def mlp_forward_encoded(weights: MLPWeights, x, expr, latent) -> torch.Tensor:
    """The model's forward on pre-encoded inputs x (N, 87) = [PE10(xyz) | PE4(dirs)] -> (N, 4) (inference)."""
    x = _c(x.detach())
    if x.dim() != 2 or x.shape[1] != 87:
        raise ValueError("expected pre-encoded inputs of shape (N, 87)")
    expr, latent = _c(expr.detach()).reshape(-1), _c(latent.detach()).reshape(-1)
    check_conditioning(expr, latent)
    packed = weights.get()
    dev = H.require_device(packed, x, expr, latent)
    fam = weights.family
    cond = torch.empty(fam.fn("cond_floats")(), dtype=torch.float32, device=dev)
    out = torch.empty((x.shape[0], 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        fam.call("forward_encoded", H.ptr(packed), H.ptr(x), H.ptr(expr), H.ptr(latent), x.shape[0], H.ptr(cond), H.ptr(out),
                 H.stream_ptr(dev))
    return out


# the paper model's entry points under their historical names (bench.py, tools/ and the tests call them)
def paper_condition(packed: torch.Tensor, expr: torch.Tensor, latent: torch.Tensor, near: float, far: float) -> torch.Tensor:
    return mlp_condition(PAPER, packed, expr, latent, near, far)


def paper_mlp_fwd(packed, cond, ro, rd, z, rd_view=None) -> torch.Tensor:
    return mlp_fwd(PAPER, "f32", packed, cond, ro, rd, z, rd_view)


def paper_mlp_fwd_bf16(packed_b, cond, ro, rd, z, rd_view=None) -> torch.Tensor:
    """Split-bf16 (3 x bf16 MFMA, f32 accumulate) forward; same outputs as paper_mlp_fwd to ~1e-5 relative."""
    return mlp_fwd(PAPER, "bf16x3", packed_b, cond, ro, rd, z, rd_view)


def paper_mlp_fwd_f16(packed_h, cond, ro, rd, z, rd_view=None) -> torch.Tensor:
    """Split-fp16 (3 x fp16 MFMA on scaled weights, f32 accumulate) forward; fp32-class accuracy (see csrc/nf_mlp_f16.hip)."""
    return mlp_fwd(PAPER, "f16x3", packed_h, cond, ro, rd, z, rd_view)


def paper_mlp_fwd_f16x2(packed_h, cond, ro, rd, z, rd_view=None) -> torch.Tensor:
    """"f16x2" forward: the split-fp16 kernel with two products per weight (csrc/nf_mlp_f16x2.hip) on the SAME packed image as f16x3."""
    return mlp_fwd(PAPER, "f16x2", packed_h, cond, ro, rd, z, rd_view)


def paper_mlp_fwd_train(packed, cond, ro, rd, z, rd_view=None, packed_b=None, packed_h=None):
    return mlp_fwd_train(PAPER, packed, cond, ro, rd, z, rd_view, packed_b=packed_b, packed_h=packed_h)


def paper_mlp_bwd(model, packed, cond, z, d_raw, saved, split=False, exact_dw=False):
    (saved_t,) = saved
    return mlp_bwd(PAPER, model.hip_weights(), packed, cond, z, d_raw, saved_t, split=split, exact_dw=exact_dw)


def split_saved_to_f32(saved_t: torch.Tensor, n_points: int, f16: bool, family: str = "paper") -> torch.Tensor:
    """The activations a SPLIT training forward saved (fragment streams of (hi, lo) pairs, sections padded to 32 points) converted to
    the exact-f32 training layout (sections [n_points][width] f32 rows at nfl::S_* x n_points): for tests and for the exact-f32
    weight-gradient GEMMs on a split forward (paper_mlp_bwd(..., exact_dw=True))."""
    fam = LCODE if family == "lcode" else PAPER
    dev = H.require_device(saved_t)
    out = torch.empty(fam.fn("saved_floats")(n_points), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        H.check(H.lib().nf_split_saved_to_f32(int(fam is LCODE), H.ptr(saved_t), n_points, int(bool(f16)), H.ptr(out), H.stream_ptr(dev)),
                "nf_split_saved_to_f32")
    return out


def require_trainable_precision() -> None:
    """A training step (need_grad) under an inference-only arithmetic is refused, not silently run on another one."""
    if _mlp_precision in INFERENCE_ONLY_PRECISIONS:
        raise RuntimeError(f'nerf.set_mlp_precision("{_mlp_precision}") is an inference arithmetic: train with "f32", "f16x3" or "bf16x3"')


_f16_train_probe_every = [128]           # training: the f32 range probe runs on a model's first forward and every n-th after it


def set_f16_train_probe_every(n: int) -> None:
    """Cadence of the split-fp16 range probe in training (calls per model; the launcher sets it to its print_every)."""
    _f16_train_probe_every[0] = max(1, int(n))


def f16_train_probe_every() -> int:
    return _f16_train_probe_every[0]


F16_ACT_LIMIT = 65504.0 / 16.0          # largest |activation| the split-fp16 kernel represents (fp16 max / its 2^4 pre-scale)
F16_PREFLIGHT_MARGIN = 4.0               # the probe refuses a model whose sampled activations come within 4x of that limit


def f16_preflight(model, ro, rd, z, rd_view, expr, latent, near, far, max_rays: int = 256, max_samples: int = 8) -> float:
    """Range probe for the split-fp16 kernel: evaluate the model family's EXACT-f32 training forward (which writes every layer's
    activations) on a strided sample of the chunk's points and return the largest hidden |activation|.  ~2k points: microseconds
    of GPU time and one host read-back."""
    n_rays, n_s = z.shape
    rs = max(1, n_rays // max_rays)
    ss = max(1, n_s // max_samples)
    ro_s, rd_s = ro[::rs].contiguous(), rd[::rs].contiguous()
    z_s = z[::rs, ::ss].contiguous()
    rv_s = None if rd_view is None else rd_view[::rs].contiguous()
    hw = model.hip_weights()
    packed = hw.get()
    cond = mlp_condition(hw.family, packed, expr, latent, near, far)
    _, (saved,) = mlp_fwd_train(hw.family, packed, cond, ro_s, rd_s, z_s, rv_s)
    lo, hi = hw.family.hidden
    n = z_s.numel()
    return float(saved[lo * n:hi * n].abs().max().item())


def f16_guard(model, ro, rd, z, rd_view, expr, latent, near, far, training: bool) -> None:
    """Refuse `model` before a split-fp16 launch when f16_preflight finds hidden activations within F16_PREFLIGHT_MARGIN of the fp16
    range.  Inference probes once per (weights, conditioning), i.e. once per frame and model; in training the weights move every
    step, so a model's first call and every f16_train_probe_every()-th after it are probed."""
    state = model.__dict__
    if training and torch.cuda.is_current_stream_capturing():
        return                           # a probe reads the device: nerf.GraphedTrainer probes before it captures and polls the flag outside
    if training:
        n_calls = state["_f16_train_calls"] = state.get("_f16_train_calls", 0) + 1
        if not (_f16_train_probe_every[0] == 1 or n_calls % _f16_train_probe_every[0] == 1):
            return
    else:
        key = (model.hip_weights()._signature()[1:], expr.data_ptr(), latent.data_ptr(), expr._version, latent._version)
        if state.get("_f16_probe_key") == key:
            return
    amax = f16_preflight(model, ro, rd, z, rd_view, expr, latent, near, far)
    if not amax * F16_PREFLIGHT_MARGIN < F16_ACT_LIMIT:
        where, use = (", ", "train") if training else (" on a sample of this frame, ", "render")
        raise RuntimeError(f'nerf.set_mlp_precision("{_mlp_precision}"): hidden activations of {type(model).__name__} reach {amax:.3g}{where}'
                           f'within {F16_PREFLIGHT_MARGIN:g}x of the fp16 range limit ({F16_ACT_LIMIT:g}) -- {use} this model with "f32" or "bf16x3"')
    if not training:
        state["_f16_probe_key"] = key


def check_f16_range(*models, sync_ranks: bool = False) -> None:
    """Raise if the split-fp16 kernels of any of `models` flagged a non-finite output since their weights were last packed
    (one 4-byte read-back per model; called once per rendered frame, never inside a ray chunk).
    sync_ranks (data-parallel training): the flag is MAX-reduced over the process group first, so that every rank raises on the
    same iteration -- a rank that raised alone would leave the others waiting in the next gradient all-reduce."""
    flags = [m.hip_weights().f16_range_flag() for m in models if m is not None and hasattr(m, "hip_weights")]
    flags = [f for f in flags if f is not None]
    if not flags:
        return
    total = torch.stack(flags).sum().to(torch.int32).reshape(1)
    if sync_ranks:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(total, op=dist.ReduceOp.MAX)
    if int(total.item()) != 0:
        raise RuntimeError(f'nerf.set_mlp_precision("{_mlp_precision}"): an activation left the fp16 range (|x| >= 4094) and a density output is '
                           'not finite -- render this model with "f32" or "bf16x3"')


# ---------------------------------------------------------------------------------------- size limits of the render kernels
# csrc/nf_render.hip sizes its wave-private LDS tables and its per-chunk register arrays at compile time (tests/test_host.py holds
# these three numbers to the #defines there).  The C entry points answer a larger size with NF_EINVAL; the wrappers below refuse it
# first, by name, before anything is allocated or launched.
MAX_BINS = 512                       # NF_MAX_BINS: entries of the inverse-CDF table (K6, and the coarse mid-points of resample_merge)
MAX_SORT = 1024                      # NF_MAX_SORT: columns of one sorted row (K7, and coarse + fine depths of resample_merge)
MAX_BWD_SAMPLES = 1024               # 64 * NF_MAX_CHUNKS: samples per ray of the integrator's BACKWARD (the forward has no limit)


def _refuse(what: str, got: str, limit: str) -> None:
    raise ValueError(f"{what}: {got} exceeds {limit} (csrc/nf_render.hip); there is no kernel for this size")


def check_resample_sizes(n_coarse: int, n_fine: int, what: str = "resample_merge") -> None:
    if n_coarse - 1 > MAX_BINS:
        _refuse(what, f"{n_coarse} coarse samples ({n_coarse - 1} bins)", f"the sampler's table limit NF_MAX_BINS = {MAX_BINS}")
    if n_coarse + n_fine > MAX_SORT:
        _refuse(what, f"{n_coarse} + {n_fine} = {n_coarse + n_fine} samples per ray", f"the row-sort limit NF_MAX_SORT = {MAX_SORT}")


def check_bwd_samples(n_samples: int, what: str = "volume_render_bwd") -> None:
    if n_samples > MAX_BWD_SAMPLES:
        _refuse(what, f"{n_samples} samples per ray",
                f"the integrator backward's limit of NF_MAX_CHUNKS = {MAX_BWD_SAMPLES // 64} chunks of 64 = {MAX_BWD_SAMPLES}")


def check_sample_counts(n_coarse: int, n_fine: int, need_grad: bool) -> None:
    """What run_one_iter_of_nerf checks before its first launch: a fine pass needs the resample + merge kernel's sizes, a training
    step the integrator backward's (the forward integrator loops over chunks at run time and takes any count)."""
    if n_fine > 0:
        check_resample_sizes(n_coarse, n_fine, "run_one_iter_of_nerf (num_coarse + num_fine)")
    if need_grad:
        check_bwd_samples(n_coarse + max(n_fine, 0), "run_one_iter_of_nerf (training step)")


# ---------------------------------------------------------------------------------------- K5
def volume_render_fwd(raw, z, rd, noise=None, bg=None, white_background=False):
    dev = H.require_device(raw, z, rd, noise, bg)
    n_rays, n_samples = z.shape
    rgb = torch.empty((n_rays, 3), dtype=torch.float32, device=dev)
    disp = torch.empty((n_rays,), dtype=torch.float32, device=dev)
    acc = torch.empty((n_rays,), dtype=torch.float32, device=dev)
    w = torch.empty((n_rays, n_samples), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        H.check(H.lib().nf_volume_render_fwd(H.ptr(raw), H.ptr(z), H.ptr(rd), H.ptr(noise), H.ptr(bg), n_rays, n_samples,
                                             1 if white_background else 0, H.ptr(rgb), H.ptr(disp), H.ptr(acc), H.ptr(w),
                                             H.stream_ptr(dev)), "nf_volume_render_fwd")
    return rgb, disp, acc, w


def volume_weights_fwd(sigma, z, rd, noise=None):
    """(disp, acc, weights) of volume_render_fwd from sigma (n_rays, n_samples) = raw[..., 3] alone, bit for bit: they depend on the
    density, z, |rd| and the noise only."""
    dev = H.require_device(sigma, z, rd, noise)
    n_rays, n_samples = z.shape
    disp = torch.empty((n_rays,), dtype=torch.float32, device=dev)
    acc = torch.empty((n_rays,), dtype=torch.float32, device=dev)
    w = torch.empty((n_rays, n_samples), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        H.check(H.lib().nf_volume_weights_fwd(H.ptr(sigma), H.ptr(z), H.ptr(rd), H.ptr(noise), n_rays, n_samples, H.ptr(disp), H.ptr(acc),
                                              H.ptr(w), H.stream_ptr(dev)), "nf_volume_weights_fwd")
    return disp, acc, w


def volume_render_bwd(raw, z, rd, noise, bg, d_rgb, white_background=False):
    d_rgb = _c(d_rgb)
    dev = H.require_device(raw, z, rd, noise, bg, d_rgb)
    n_rays, n_samples = z.shape
    check_bwd_samples(n_samples)
    d_raw = torch.empty((n_rays, n_samples, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        H.check(H.lib().nf_volume_render_bwd(H.ptr(raw), H.ptr(z), H.ptr(rd), H.ptr(noise), H.ptr(bg), H.ptr(d_rgb), n_rays,
                                             n_samples, 1 if white_background else 0, H.ptr(d_raw), H.stream_ptr(dev)),
                "nf_volume_render_bwd")
    return d_raw


def _cotangent(name: str, t, shape, what: str):
    """A cotangent of the full integrator backward: None (zero), or float32 of exactly `shape`; anything else is refused by name,
    before anything is allocated or launched."""
    if t is None:
        return None
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what}: {name} must have shape {tuple(shape)}, got {got}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def volume_render_bwd_full(raw, z, rd, noise, bg, d_rgb=None, d_disp=None, d_acc=None, d_weights=None, d_w_last=None,
                           white_background=False, need_d_bg=False):
    """The integrator's backward through every output: cotangents of rgb (R, 3), disp (R), acc (R), weights (R, S) and of
    weights[:, -1] alone (R), each optional -> (d_raw (R, S, 4), d_bg (R, 3) or None).  d_bg, the gradient of the background prior
    (the last sample's colour), is computed when need_d_bg.  volume_render_bwd stays the path of a backward that carries d_rgb only."""
    what = "volume_render_bwd_full"
    n_rays, n_samples = z.shape
    d_rgb = _cotangent("d_rgb", d_rgb, (n_rays, 3), what)
    d_disp = _cotangent("d_disp", d_disp, (n_rays,), what)
    d_acc = _cotangent("d_acc", d_acc, (n_rays,), what)
    d_weights = _cotangent("d_weights", d_weights, (n_rays, n_samples), what)
    d_w_last = _cotangent("d_w_last", d_w_last, (n_rays,), what)
    if d_rgb is None and d_disp is None and d_acc is None and d_weights is None and d_w_last is None:
        raise ValueError(f"{what}: no cotangent given (d_rgb, d_disp, d_acc, d_weights and d_w_last are all None)")
    if need_d_bg and bg is None:
        raise ValueError(f"{what}: need_d_bg without a background prior (bg is None)")
    check_bwd_samples(n_samples, what)
    dev = H.require_device(raw, z, rd, noise, bg, d_rgb, d_disp, d_acc, d_weights, d_w_last)
    d_raw = torch.empty((n_rays, n_samples, 4), dtype=torch.float32, device=dev)
    d_bg = torch.empty((n_rays, 3), dtype=torch.float32, device=dev) if need_d_bg else None
    with torch.cuda.device(dev):
        H.check(H.lib().nf_volume_render_bwd_full(H.ptr(raw), H.ptr(z), H.ptr(rd), H.ptr(noise), H.ptr(bg), H.ptr(d_rgb), H.ptr(d_disp),
                                                  H.ptr(d_acc), H.ptr(d_weights), H.ptr(d_w_last), n_rays, n_samples,
                                                  1 if white_background else 0, H.ptr(d_raw), H.ptr(d_bg), H.stream_ptr(dev)),
                "nf_volume_render_bwd_full")
    return d_raw, d_bg


def render_volume_density(raw, depth):
    """tiny_nerf's compositing (TN:68-107: no background sample, no +1e-6, spacing not scaled by |rd|): raw (n_rays, S, 4),
    depth (n_rays, S) -> (rgb_map (n_rays, 3), depth_map (n_rays), acc_map (n_rays))."""
    dev = H.require_device(raw, depth)
    n_rays, n_samples = depth.shape
    rgb = torch.empty((n_rays, 3), dtype=torch.float32, device=dev)
    dmap = torch.empty((n_rays,), dtype=torch.float32, device=dev)
    acc = torch.empty((n_rays,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        H.check(H.lib().nf_render_volume_density(H.ptr(raw), H.ptr(depth), n_rays, n_samples, H.ptr(rgb), H.ptr(dmap), H.ptr(acc),
                                                 H.stream_ptr(dev)), "nf_render_volume_density")
    return rgb, dmap, acc


def render_volume_density_bwd(raw, depth, d_rgb):
    """Backward of render_volume_density for its rgb output: d_rgb (n_rays, 3) -> d_raw (n_rays, S, 4)."""
    d_rgb = _c(d_rgb)
    dev = H.require_device(raw, depth, d_rgb)
    n_rays, n_samples = depth.shape
    check_bwd_samples(n_samples, "render_volume_density_bwd")
    d_raw = torch.empty((n_rays, n_samples, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        H.check(H.lib().nf_render_volume_density_bwd(H.ptr(raw), H.ptr(depth), H.ptr(d_rgb), n_rays, n_samples, H.ptr(d_raw),
                                                     H.stream_ptr(dev)), "nf_render_volume_density_bwd")
    return d_raw


def render_volume_density_bwd_full(raw, depth, d_rgb=None, d_depth=None, d_acc=None):
    """Backward of render_volume_density through all three outputs: cotangents of rgb_map (R, 3), depth_map (R) and acc_map (R),
    each optional -> d_raw (R, S, 4)."""
    what = "render_volume_density_bwd_full"
    n_rays, n_samples = depth.shape
    d_rgb = _cotangent("d_rgb", d_rgb, (n_rays, 3), what)
    d_depth = _cotangent("d_depth", d_depth, (n_rays,), what)
    d_acc = _cotangent("d_acc", d_acc, (n_rays,), what)
    if d_rgb is None and d_depth is None and d_acc is None:
        raise ValueError(f"{what}: no cotangent given (d_rgb, d_depth and d_acc are all None)")
    check_bwd_samples(n_samples, what)
    dev = H.require_device(raw, depth, d_rgb, d_depth, d_acc)
    d_raw = torch.empty((n_rays, n_samples, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        H.check(H.lib().nf_render_volume_density_bwd_full(H.ptr(raw), H.ptr(depth), H.ptr(d_rgb), H.ptr(d_depth), H.ptr(d_acc), n_rays,
                                                          n_samples, H.ptr(d_raw), H.stream_ptr(dev)),
                "nf_render_volume_density_bwd_full")
    return d_raw


# ---------------------------------------------------------------------------------------- the trainer's loss (TR:355-387)
class _TrainingLoss(torch.autograd.Function):
    """loss = mse(rgb_coarse, target) + mse(rgb_fine, target) + code_scale * code_weight * ||latent||, forward and backward one launch
    each (nf_train_loss_fwd / nf_train_loss_bwd) instead of the ~20 torch launches of TR:355-387 and their backward nodes."""

    @staticmethod
    def forward(ctx, rgb_c, rgb_f, target, latent, code_weight, code_scale):
        dev = H.require_device(rgb_c, rgb_f, target, latent)
        out = torch.empty((7,), dtype=torch.float32, device=dev)
        n = rgb_c.numel()
        with torch.cuda.device(dev):
            H.check(H.lib().nf_train_loss_fwd(H.ptr(rgb_c), H.ptr(rgb_f), H.ptr(target), n, H.ptr(latent), 0 if latent is None else latent.numel(),
                                              float(code_weight), float(code_scale), H.ptr(out), H.stream_ptr(dev)), "nf_train_loss_fwd")
        ctx.save_for_backward(rgb_c, rgb_f, target, latent, out)
        ctx.consts = (float(code_weight), float(code_scale))
        parts = out.detach()
        ctx.mark_non_differentiable(parts)
        return out[0], parts

    @staticmethod
    def backward(ctx, go, _go_parts):
        rgb_c, rgb_f, target, latent, out = ctx.saved_tensors
        dev = rgb_c.device
        go = go.to(torch.float32).contiguous()
        d_c = torch.empty_like(rgb_c)
        d_f = torch.empty_like(rgb_f) if rgb_f is not None else None
        d_l = torch.empty_like(latent) if latent is not None else None
        with torch.cuda.device(dev):
            H.check(H.lib().nf_train_loss_bwd(H.ptr(rgb_c), H.ptr(rgb_f), H.ptr(target), rgb_c.numel(), H.ptr(latent),
                                              0 if latent is None else latent.numel(), ctx.consts[0], ctx.consts[1], H.ptr(out), H.ptr(go),
                                              H.ptr(d_c), H.ptr(d_f), H.ptr(d_l), H.stream_ptr(dev)), "nf_train_loss_bwd")
        return d_c, d_f, None, d_l, None, None


class _TrainingLossBg(torch.autograd.Function):
    """_TrainingLoss plus the background-supervision term of TR:376-381 (nf_train_loss_bg_fwd / nf_train_loss_bg_bwd): the same two
    launches, and the gradients of the selected background pixels and of the last sample's weight besides."""

    @staticmethod
    def forward(ctx, rgb_c, rgb_f, target, latent, bg, w_last, code_weight, code_scale, bg_weight):
        dev = H.require_device(rgb_c, rgb_f, target, latent, bg, w_last)
        out = torch.empty((8,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            H.check(H.lib().nf_train_loss_bg_fwd(H.ptr(rgb_c), H.ptr(rgb_f), H.ptr(target), rgb_c.numel(), H.ptr(latent),
                                                 0 if latent is None else latent.numel(), float(code_weight), float(code_scale), H.ptr(bg),
                                                 H.ptr(w_last), float(bg_weight), H.ptr(out), H.stream_ptr(dev)), "nf_train_loss_bg_fwd")
        ctx.save_for_backward(rgb_c, rgb_f, target, latent, bg, w_last, out)
        ctx.consts = (float(code_weight), float(code_scale), float(bg_weight))
        parts = out.detach()
        ctx.mark_non_differentiable(parts)
        return out[0], parts

    @staticmethod
    def backward(ctx, go, _go_parts):
        rgb_c, rgb_f, target, latent, bg, w_last, out = ctx.saved_tensors
        dev = rgb_c.device
        go = go.to(torch.float32).contiguous()
        d_c = torch.empty_like(rgb_c)
        d_f = torch.empty_like(rgb_f) if rgb_f is not None else None
        d_l = torch.empty_like(latent) if latent is not None else None
        d_bg, d_w = torch.empty_like(bg), torch.empty_like(w_last)
        with torch.cuda.device(dev):
            H.check(H.lib().nf_train_loss_bg_bwd(H.ptr(rgb_c), H.ptr(rgb_f), H.ptr(target), rgb_c.numel(), H.ptr(latent),
                                                 0 if latent is None else latent.numel(), ctx.consts[0], ctx.consts[1], H.ptr(bg),
                                                 H.ptr(w_last), ctx.consts[2], H.ptr(out), H.ptr(go), H.ptr(d_c), H.ptr(d_f), H.ptr(d_l),
                                                 H.ptr(d_bg), H.ptr(d_w), H.stream_ptr(dev)), "nf_train_loss_bg_bwd")
        return d_c, d_f, None, d_l, d_bg, d_w, None, None, None


def training_loss(rgb_coarse, rgb_fine, target, latent=None, code_weight: float = 0.0005, code_scale: float = 10.0,
                  background=None, last_weight=None, background_weight: float = 0.001):
    """The trainer's loss (TR:355-387) fused: returns (loss, parts) with parts = [loss, coarse mse, fine mse, code loss, coarse + fine,
    psnr of coarse + fine, ||latent||] (detached, for logging); `loss` is differentiable w.r.t. rgb_coarse, rgb_fine and latent.
    rgb_fine / latent may be None.  Colour maps and target: the same shape, float32 (made contiguous if they are not).
    background (n_rays, 3) + last_weight (n_rays): add the background-supervision term of TR:376-381, mean(sum((background -
    target)^2, 1) * last_weight) * background_weight, in the same two launches; `loss` is then differentiable w.r.t. both as well
    and `parts` ends with the term (8 entries).  With both None the entry points and launches are the ones above."""
    for t in (rgb_coarse, rgb_fine, target, latent, background, last_weight):   # before _c(): a float64 map must not be down-cast silently
        if t is not None and t.dtype != torch.float32:
            raise TypeError("training_loss: float32 tensors only")
    if (background is None) != (last_weight is None):
        raise ValueError("training_loss: the background term needs both `background` (n_rays, 3) and `last_weight` (n_rays)")
    rgb_c, tgt = _c(rgb_coarse), _c(target)
    rgb_f = _c(rgb_fine) if rgb_fine is not None else None
    lat = _c(latent) if latent is not None else None
    if tgt.shape != rgb_c.shape or (rgb_f is not None and rgb_f.shape != rgb_c.shape):
        raise ValueError(f"training_loss: colour maps {tuple(rgb_c.shape)} / {None if rgb_f is None else tuple(rgb_f.shape)} and target "
                         f"{tuple(tgt.shape)} must have one shape")
    if background is None:
        return _TrainingLoss.apply(rgb_c, rgb_f, tgt, lat, code_weight, code_scale)
    bg, w_last = _c(background), _c(last_weight)
    if rgb_c.dim() != 2 or rgb_c.shape[1] != 3 or bg.shape != rgb_c.shape or tuple(w_last.shape) != (rgb_c.shape[0],):
        raise ValueError(f"training_loss: the background term needs (n_rays, 3) colour maps and background and an (n_rays,) last_weight; "
                         f"got {tuple(rgb_c.shape)}, {tuple(bg.shape)}, {tuple(w_last.shape)}")
    return _TrainingLossBg.apply(rgb_c, rgb_f, tgt, lat, bg, w_last, code_weight, code_scale, background_weight)


# ---------------------------------------------------------------------------------------- K6 / K7
def _u_arg(u: Optional[torch.Tensor], n_rays: int, n_out: int, device):
    if u is None:                                     # det mode (H:357-362): linspace(0,1,n) broadcast over rays
        return linspace01(n_out, device), 0
    u = _c(u)
    H.require_device(u)
    assert tuple(u.shape) == (n_rays, n_out), (tuple(u.shape), (n_rays, n_out))
    return u, n_out


def sample_pdf(bins, weights, n_out: int, u: Optional[torch.Tensor] = None, want_table: bool = False):
    """sample_pdf_2 (H:344-387).  want_table: also return (inds int32 (R,n_out) = searchsorted(cdf, u, right=True), cdf (R,n_bins))."""
    bins, weights = _c(bins), _c(weights)
    dev = H.require_device(bins, weights)
    n_rays, n_bins = bins.shape
    assert weights.shape == (n_rays, n_bins - 1)
    if n_bins > MAX_BINS:
        _refuse("sample_pdf", f"{n_bins} bins", f"the sampler's table limit NF_MAX_BINS = {MAX_BINS}")
    u_t, stride = _u_arg(u, n_rays, n_out, dev)
    out = torch.empty((n_rays, n_out), dtype=torch.float32, device=dev)
    inds = torch.empty((n_rays, n_out), dtype=torch.int32, device=dev) if want_table else None
    cdf = torch.empty((n_rays, n_bins), dtype=torch.float32, device=dev) if want_table else None
    with torch.cuda.device(dev):
        H.check(H.lib().nf_sample_pdf_ex(H.ptr(bins), H.ptr(weights), H.ptr(u_t), stride, n_rays, n_bins, n_out, H.ptr(out),
                                         H.ptr(inds), H.ptr(cdf), H.stream_ptr(dev)), "nf_sample_pdf_ex")
    return (out, inds, cdf) if want_table else out


def resample_merge(z_coarse, w_coarse, n_fine: int, u: Optional[torch.Tensor] = None, want_samples: bool = False):
    dev = H.require_device(z_coarse, w_coarse)
    n_rays, n_coarse = z_coarse.shape
    check_resample_sizes(n_coarse, n_fine)
    u_t, stride = _u_arg(u, n_rays, n_fine, dev)
    z_fine = torch.empty((n_rays, n_coarse + n_fine), dtype=torch.float32, device=dev)
    z_s = torch.empty((n_rays, n_fine), dtype=torch.float32, device=dev) if want_samples else None
    with torch.cuda.device(dev):
        H.check(H.lib().nf_resample_merge(H.ptr(z_coarse), H.ptr(w_coarse), H.ptr(u_t), stride, n_rays, n_coarse, n_fine,
                                          H.ptr(z_s), H.ptr(z_fine), H.stream_ptr(dev)), "nf_resample_merge")
    return (z_fine, z_s) if want_samples else z_fine


def sort_rows(x: torch.Tensor) -> torch.Tensor:
    x = _c(x)
    dev = H.require_device(x)
    n_cols = x.shape[-1]
    if n_cols > MAX_SORT:
        _refuse("sort_rows", f"{n_cols} columns", f"the row-sort limit NF_MAX_SORT = {MAX_SORT}")
    rows = x.numel() // n_cols
    out = torch.empty_like(x)
    with torch.cuda.device(dev):
        H.check(H.lib().nf_sort_rows(H.ptr(x), rows, n_cols, H.ptr(out), H.stream_ptr(dev)), "nf_sort_rows")
    return out


# ---------------------------------------------------------------------------------------- eval post-processing
def eval_postprocess(rgb, depthmap=None, weights=None, intrinsics=None, want_normals=True):
    """(H,W,3) float image -> uint8 image (clamp, x255, truncate: EV:184-190) and, from the disparity/"depth" map the eval
    script feeds torch_normal_map (EV:84-119), the cleaned uint8 normal map (H-1, W-1, 3).  Device tensors in and out."""
    rgb = _c(rgb)
    depthmap = _c(depthmap) if depthmap is not None else None
    weights = _c(weights) if weights is not None else None
    dev = H.require_device(rgb, depthmap, weights)
    h, w = rgb.shape[0], rgb.shape[1]
    rgb_u8 = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    normals = None
    fx = fy = 1.0
    cx = cy = 0.0
    if want_normals and depthmap is not None:
        import numpy as _np
        a = _np.asarray(intrinsics, dtype=_np.float64).reshape(-1)
        fx, fy = float(_np.float32(a[0])), float(_np.float32(a[1]))
        cx, cy = float(_np.float32(a[2] * w)), float(_np.float32(a[3] * h))
        normals = torch.empty((h - 1, w - 1, 3), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        H.check(H.lib().nf_eval_postprocess(H.ptr(rgb), H.ptr(depthmap), H.ptr(weights), h, w, fx, fy, cx, cy, H.ptr(rgb_u8),
                                            H.ptr(normals), H.stream_ptr(dev)), "nf_eval_postprocess")
    return rgb_u8, normals


# ---------------------------------------------------------------------------------------- image metrics
def quantize_image(x: torch.Tensor) -> torch.Tensor:
    """Float image in [0, 1] -> uint8 by clamp and ROUND TO NEAREST: recovers k from float32(k / 255) for all 256 bytes (a test
    image as the loaders hold it).  The rendered frame is quantised by truncation instead (eval_postprocess, EV:184-190): those
    are the bytes written to disk."""
    return (x.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8)


METRIC_NAMES = ("l1", "mse", "psnr", "ssim")


def image_metrics(pred_u8: torch.Tensor, target_u8: torch.Tensor, ssim_data_range: float = 2.0) -> dict:
    """L1, MSE, PSNR and SSIM of uint8 images (H, W, 3) or (N, H, W, 3) against their targets, one launch for the batch and no host
    synchronisation: {"l1", "mse", "psnr", "ssim"} float64 and {"abs_sum", "sq_sum"} int64 device tensors, shape (N,) (0-d for a
    single image).  The values are the reference's nerf/metrics.py on the float images byte / 255: np.mean(np.abs(.)), compare_psnr
    (data range 1) and compare_ssim(multichannel=True), whose data range for float input is 2 (the dtype's range (-1, 1)): pass
    ssim_data_range=1.0 for the textbook constants."""
    for name, t in (("pred_u8", pred_u8), ("target_u8", target_u8)):
        if not torch.is_tensor(t) or t.dtype != torch.uint8:
            raise TypeError(f"image_metrics: {name} must be a uint8 tensor, got {getattr(t, 'dtype', type(t))} "
                            "(nerf.quantize_image turns a float image in [0, 1] into one)")
    if pred_u8.shape != target_u8.shape:
        raise ValueError(f"image_metrics: shapes differ: {tuple(pred_u8.shape)} and {tuple(target_u8.shape)}")
    if pred_u8.dim() not in (3, 4) or pred_u8.shape[-1] != 3:
        raise ValueError(f"image_metrics: expected (H, W, 3) or (N, H, W, 3), got {tuple(pred_u8.shape)}")
    h, w = int(pred_u8.shape[-3]), int(pred_u8.shape[-2])
    if h < 7 or w < 7:
        raise ValueError(f"image_metrics: the 7 x 7 SSIM window needs H >= 7 and W >= 7, got {h} x {w}")
    if not (pred_u8.is_cuda and target_u8.is_cuda):
        raise RuntimeError("nerf (MI355X build): tensors must live on a ROCm device (`device='cuda'`); "
                           "there is no CPU path in this package")
    if pred_u8.device != target_u8.device:
        raise RuntimeError("nerf (MI355X build): tensors are on different devices")
    single = pred_u8.dim() == 3
    a, b, dev = pred_u8.contiguous(), target_u8.contiguous(), pred_u8.device
    n = 1 if single else int(a.shape[0])
    out_f = torch.empty((n, 4), dtype=torch.float64, device=dev)
    out_i = torch.empty((n, 2), dtype=torch.int64, device=dev)
    if n:
        lib = H.lib()
        ws_bytes = int(lib.nf_image_metrics_workspace_bytes(n, h, w))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            H.check(lib.nf_image_metrics(H.ptr(a), H.ptr(b), n, h, w, float(ssim_data_range), H.ptr(ws), ws_bytes, H.ptr(out_f),
                                         H.ptr(out_i), H.stream_ptr(dev)), "nf_image_metrics")
    pick = (lambda t, k: t[0, k]) if single else (lambda t, k: t[:, k])
    res = {name: pick(out_f, k) for k, name in enumerate(METRIC_NAMES)}
    res["abs_sum"], res["sq_sum"] = pick(out_i, 0), pick(out_i, 1)
    return res


class ImageMetricsTable:
    """The metrics of a sequence, one frame per call, into buffers allocated once: an (n_frames, 4) float64 table (METRIC_NAMES), an
    (n_frames, 2) int64 table (sum |d|, sum d^2) and one workspace.  add() is nothing but the launch -- no allocation, no new tensor,
    no host synchronisation -- which is what a render loop that the host paces wants (launch/eval_sharded.py --metrics)."""

    def __init__(self, n_frames: int, height: int, width: int, device, ssim_data_range: float = 2.0):
        if height < 7 or width < 7:
            raise ValueError(f"ImageMetricsTable: the 7 x 7 SSIM window needs H >= 7 and W >= 7, got {height} x {width}")
        self.shape, self.device, self.data_range, self.count = (int(height), int(width), 3), torch.device(device), float(ssim_data_range), 0
        self.values = torch.zeros((n_frames, 4), dtype=torch.float64, device=self.device)
        self.sums = torch.zeros((n_frames, 2), dtype=torch.int64, device=self.device)
        self._lib = H.lib()
        self._ws_bytes = int(self._lib.nf_image_metrics_workspace_bytes(1, height, width))
        self._ws = torch.empty(self._ws_bytes, dtype=torch.uint8, device=self.device)

    def add(self, pred_u8: torch.Tensor, target_u8: torch.Tensor) -> int:
        """Launch the metrics of one (H, W, 3) uint8 pair into the next row; returns the row."""
        for t in (pred_u8, target_u8):
            if t.dtype != torch.uint8 or tuple(t.shape) != self.shape or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"ImageMetricsTable.add: expected contiguous uint8 {self.shape} on {self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        row = self.count
        if row >= self.values.shape[0]:
            raise IndexError("ImageMetricsTable.add: the table is full")
        h, w, _ = self.shape
        H.check(self._lib.nf_image_metrics(H.ptr(pred_u8), H.ptr(target_u8), 1, h, w, self.data_range, H.ptr(self._ws), self._ws_bytes,
                                           self.values.data_ptr() + 32 * row, self.sums.data_ptr() + 16 * row, H.stream_ptr(self.device)),
                "nf_image_metrics")
        self.count = row + 1
        return row


# ---------------------------------------------------------------------------------------- isosurface of a dense grid
def _box(lo, hi, what: str):
    lo, hi = [float(x) for x in lo], [float(x) for x in hi]
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError(f"{what}: lo and hi are three numbers each")
    lo32, hi32 = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    if not bool(np.all(lo32 < hi32)):
        raise ValueError(f"{what}: the box needs lo < hi on every axis (in float32), got lo={lo}, hi={hi}")
    return lo32, hi32


def _workspace(lib, fn_name, args, dev, message: str):
    """(workspace on dev, its bytes) by the unit's size query; ValueError(message) for a size past its plan.  dev = None: no workspace, the check alone."""
    ws_bytes = int(getattr(lib, fn_name)(*args))
    if ws_bytes == 0:
        raise ValueError(message)
    return None if dev is None else torch.empty(ws_bytes, dtype=torch.uint8, device=dev), ws_bytes


def isosurface(grid: torch.Tensor, level: float, lo, hi, normals: bool = False):
    """Triangle mesh of the surface grid == level inside the box [lo, hi]: grid (nz, ny, nx) float32 on a ROCm device, x fastest,
    grid point (i, j, k) at lo + (i, j, k) * (hi - lo) / (n - 1); a point is inside iff grid > level.  Marching tetrahedra on the
    Kuhn triangulation (DESIGN.md "Isosurface"): welded vertices, consistent orientation (normals from inside to outside),
    watertight wherever the box does not cut the surface, and the same bits from run to run.  Returns device tensors
    (vertices (V, 3) float32, faces (F, 3) int32, normals (V, 3) float32 or None); an all-inside or all-outside grid gives (0, 3)
    tensors.  Exactly one host read: the two counts, which size the outputs."""
    if not torch.is_tensor(grid) or grid.dim() != 3:
        raise ValueError("isosurface: expected a grid of shape (nz, ny, nx)")
    grid = grid.detach().contiguous()
    dev = H.require_device(grid)
    nz, ny, nx = (int(s) for s in grid.shape)
    if min(nx, ny, nz) < 2:
        raise ValueError(f"isosurface: every axis needs at least 2 grid points, got (nz, ny, nx) = {(nz, ny, nx)}")
    lo32, hi32 = _box(lo, hi, "isosurface")
    lib = H.lib()
    ws, ws_bytes = _workspace(lib, "nf_isosurface_workspace_bytes", (nx, ny, nz), dev, f"isosurface: a grid of {nx} x {ny} x {nz} points is past the plan "
                              "of csrc/nf_isosurface.hip (7 * points and 12 * cells stay below 2^31: vertex and face ids are int32)")
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    c_lo, c_hi = (C.c_float * 3)(*lo32.tolist()), (C.c_float * 3)(*hi32.tolist())
    with torch.cuda.device(dev):
        H.check(lib.nf_isosurface_count(H.ptr(grid), nx, ny, nz, float(level), H.ptr(ws), ws_bytes, H.ptr(counts), H.stream_ptr(dev)),
                "nf_isosurface_count")
        n_verts, n_faces = counts.tolist()                              # the one host read
        verts = torch.empty((n_verts, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
        norm = torch.empty((n_verts, 3), dtype=torch.float32, device=dev) if normals else None
        if n_verts and n_faces:
            H.check(lib.nf_isosurface_emit(H.ptr(grid), nx, ny, nz, float(level), C.addressof(c_lo), C.addressof(c_hi), H.ptr(ws), ws_bytes,
                                           H.ptr(verts), n_verts, H.ptr(faces), n_faces, H.ptr(norm), H.stream_ptr(dev)), "nf_isosurface_emit")
    return verts, faces, norm


# ---------------------------------------------------------------------------------------- connected components of a mesh
class MeshComponents(NamedTuple):
    vertex_label: torch.Tensor                   # (V,) int32: the component of every vertex, 0 .. C-1 by ascending smallest vertex id
    face_label: torch.Tensor                     # (F,) int32: the label of the face's first vertex, -1 for a face with an index outside [0, V)
    face_counts: torch.Tensor                    # (C,) int32: valid faces per component
    vertex_counts: torch.Tensor                  # (C,) int32: vertices per component


class MeshFilterStats(NamedTuple):
    components: int                              # components of the mesh (an unused vertex is one of its own)
    kept_components: int
    vertices: int
    kept_vertices: int
    faces: int
    kept_faces: int


def _check_faces(faces, n_vertices, what: str):
    if not torch.is_tensor(faces) or faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: faces must be an int32 tensor of shape (F, 3)")
    n_vertices = int(n_vertices)
    if not 0 <= n_vertices < 2 ** 31 or faces.shape[0] >= 2 ** 31:
        raise ValueError(f"{what}: the numbers of vertices and faces lie in [0, 2^31), got {n_vertices} and {faces.shape[0]}")
    return n_vertices, int(faces.shape[0])


def _check_vertices(vertices, what: str):
    if not torch.is_tensor(vertices) or vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{what}: vertices must be a float32 tensor of shape (V, 3)")


def _check_normals(normals, vertices, what: str):
    if normals is not None and (not torch.is_tensor(normals) or normals.dtype != torch.float32 or normals.shape != vertices.shape):
        raise ValueError(f"{what}: normals must be None or a float32 tensor of the vertices' shape {tuple(vertices.shape)}")


def _check_filter_args(vertices, faces, normals, largest, min_faces, what: str):
    """Everything filter_mesh can refuse without a device; returns (V, F, largest, min_faces) with min_faces = 0 under `largest`."""
    _check_vertices(vertices, what)
    n_vertices, n_faces = _check_faces(faces, vertices.shape[0], what)
    _check_normals(normals, vertices, what)
    largest = bool(largest)
    if largest == (min_faces is not None):
        raise ValueError(f"{what}: exactly one rule applies, largest=True or min_faces=N")
    if min_faces is not None:
        if isinstance(min_faces, bool) or int(min_faces) != min_faces or not 1 <= int(min_faces) < 2 ** 63:
            raise ValueError(f"{what}: min_faces is a whole number of at least 1, got {min_faces!r}")
        min_faces = int(min_faces)
    return n_vertices, n_faces, largest, min_faces or 0


def _require_same_device(what, first, *others):
    if not first.is_cuda:
        raise RuntimeError("nerf (MI355X build): tensors must live on a ROCm device (`device='cuda'`); there is no CPU path in this package")
    for t in others:
        if t is not None and t.device != first.device:
            raise RuntimeError(f"{what}: tensors are on different devices")
    return first.device


def _label_mesh(lib, faces, n_vertices, n_faces, counts, dev, what):
    """The workspace (returned first, with its bytes) and the launches of nf_mesh_components_label into fresh buffers (the counts hold V entries, C written)."""
    ws, ws_bytes = _workspace(lib, "nf_mesh_components_workspace_bytes", (n_vertices, n_faces), dev,
                              f"{what}: {n_vertices} vertices and {n_faces} faces are past the plan of csrc/nf_mesh_components.hip (both below 2^31)")
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    vertex_label, face_label, face_counts, vertex_counts = i32(n_vertices), i32(n_faces), i32(n_vertices), i32(n_vertices)
    H.check(lib.nf_mesh_components_label(H.ptr(faces), n_vertices, n_faces, H.ptr(ws), ws_bytes, H.ptr(vertex_label), H.ptr(face_label),
                                         H.ptr(face_counts), H.ptr(vertex_counts), H.ptr(counts), H.stream_ptr(dev)), "nf_mesh_components_label")
    return (ws, ws_bytes), vertex_label, face_label, face_counts, vertex_counts


def mesh_components(faces: torch.Tensor, n_vertices: int) -> MeshComponents:
    """Connected components of the mesh `faces` (F, 3) int32 over n_vertices vertices, on a ROCm device (DESIGN.md "Mesh components"):
    two vertices are connected iff a chain of faces links them, a shared vertex being enough; a face with an index outside
    [0, n_vertices) takes no part and is labelled -1; a vertex no face uses is a component of its own.  Components are numbered by
    ascending smallest vertex id.  Union-find on the device (csrc/nf_mesh_components.hip), the same bits from run to run.  Exactly
    one host read: the number of components, which sizes the counts."""
    n_vertices, n_faces = _check_faces(faces, n_vertices, "mesh_components")
    dev = _require_same_device("mesh_components", faces)
    faces = faces.detach().contiguous()
    lib = H.lib()
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _, vertex_label, face_label, face_counts, vertex_counts = _label_mesh(lib, faces, n_vertices, n_faces, counts, dev, "mesh_components")
        n_components = int(counts[0].item())                            # the one host read
    return MeshComponents(vertex_label, face_label, face_counts[:n_components].clone(), vertex_counts[:n_components].clone())


def filter_mesh(vertices: torch.Tensor, faces: torch.Tensor, normals: Optional[torch.Tensor] = None, *, largest: bool = False, min_faces=None):
    """The mesh of the components one rule keeps: largest=True, the component with the most faces (ties: the one with the smallest
    vertex id; nothing if no component has a face), or min_faces=N >= 1, every component with at least N faces.  Kept vertices and
    the faces of kept components stay in their order, the indices are renumbered, vertex and normal rows are copied bit for bit; a
    face with an index outside [0, V) is never kept.  Returns (vertices, faces, normals or None, MeshFilterStats); an empty result
    is made of (0, 3) tensors.  Labelling, selection and compaction run on the device with exactly one host read (the counts that
    size the outputs)."""
    n_vertices, n_faces, largest, min_faces = _check_filter_args(vertices, faces, normals, largest, min_faces, "filter_mesh")
    dev = _require_same_device("filter_mesh", vertices, faces, normals)
    vertices, faces = vertices.detach().contiguous(), faces.detach().contiguous()
    normals = None if normals is None else normals.detach().contiguous()
    lib = H.lib()
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        stream = H.stream_ptr(dev)
        (ws, ws_bytes), vertex_label, face_label, face_counts, _ = _label_mesh(lib, faces, n_vertices, n_faces, counts, dev, "filter_mesh")
        H.check(lib.nf_mesh_components_select(H.ptr(vertex_label), H.ptr(face_label), H.ptr(face_counts), n_vertices, n_faces, int(largest), min_faces,
                                              H.ptr(ws), ws_bytes, H.ptr(counts), stream), "nf_mesh_components_select")
        n_components, kept_v, kept_f, kept_c = counts.tolist()          # the one host read
        out_v = torch.empty((kept_v, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((kept_f, 3), dtype=torch.int32, device=dev)
        out_n = None if normals is None else torch.empty((kept_v, 3), dtype=torch.float32, device=dev)
        if kept_v:
            H.check(lib.nf_mesh_components_emit(H.ptr(vertices), H.ptr(faces), H.ptr(normals), H.ptr(vertex_label), H.ptr(face_label),
                                                H.ptr(face_counts), n_vertices, n_faces, H.ptr(ws), ws_bytes, H.ptr(out_v), kept_v, H.ptr(out_f),
                                                kept_f, H.ptr(out_n), stream), "nf_mesh_components_emit")
    return out_v, out_f, out_n, MeshFilterStats(n_components, kept_c, n_vertices, kept_v, n_faces, kept_f)


# ---------------------------------------------------------------------------------------- Taubin smoothing of a mesh
MESH_SMOOTH_SHORT_ROW = 32                       # nfs::SHORT_ROW of csrc/nf_mesh_smooth.hip: a row of the vertex -> neighbours (or vertex -> faces)
                                                 # table of at most this many entries, repeats included, is sorted by one thread, a longer one by a wave


class MeshAdjacency(NamedTuple):
    row_start: torch.Tensor                      # (V + 1,) int32: row v of the two arrays below is [row_start[v], row_start[v + 1])
    neighbours: torch.Tensor                     # (E,) int32: the distinct w != v that a side of a valid face joins to v, ascending
    multiplicity: torch.Tensor                   # (E,) int32: the number of sides joining v and w (2 inside a closed surface)
    boundary: torch.Tensor                       # (V,) uint8: 1 iff v is an end of an edge of multiplicity 1


class MeshSmoothStats(NamedTuple):
    edges: int                                   # E: directed pairs, twice the number of edges
    boundary_vertices: int
    pinned_vertices: int                         # the boundary vertices under fix_boundary, else 0
    passes: int                                  # launches of the pass kernel: iterations, twice that with mu != 0


def _check_smooth_sizes(n_vertices, n_faces, what: str):
    if not 0 <= n_vertices < 2 ** 31 or not 6 * n_faces < 2 ** 31:
        raise ValueError(f"{what}: V and 6 F lie in [0, 2^31) (ids and table positions are int32), got V = {n_vertices} and F = {n_faces}")


def _check_smooth_mesh(vertices, faces, what: str):
    _check_vertices(vertices, what)
    n_vertices, n_faces = _check_faces(faces, vertices.shape[0], what)
    _check_smooth_sizes(n_vertices, n_faces, what)
    return n_vertices, n_faces


def _check_smooth_args(vertices, faces, normals, iterations, lam, mu, what: str):
    """Everything smooth_mesh can refuse without a device; returns (V, F, iterations, lam, mu), the factors rounded to float32."""
    n_vertices, n_faces = _check_smooth_mesh(vertices, faces, what)
    _check_normals(normals, vertices, what)
    try:
        whole = not isinstance(iterations, bool) and int(iterations) == iterations and 0 <= int(iterations) < 2 ** 30
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole:
        raise ValueError(f"{what}: iterations is a whole number of at least 0 (and below 2^30), got {iterations!r}")
    try:
        lam32, mu32 = float(np.float32(lam)), float(np.float32(mu))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: lam and mu are numbers, got {lam!r} and {mu!r}")
    if not (0.0 < lam32 <= 1.0) or not (-1.0 <= mu32 <= 0.0):                 # not finite fails both
        raise ValueError(f"{what}: 0 < lam <= 1 and -1 <= mu <= 0 (in float32), got lam = {lam!r} and mu = {mu!r}")
    return n_vertices, n_faces, int(iterations), lam32, mu32


def _mesh_smooth_workspace(lib, n_vertices, n_faces, dev, what):
    return _workspace(lib, "nf_mesh_smooth_workspace_bytes", (n_vertices, n_faces), dev,
                      f"{what}: {n_vertices} vertices and {n_faces} faces are past the plan of csrc/nf_mesh_smooth.hip (V and 6 F below 2^31)")


def _adjacency(lib, faces, n_vertices, n_faces, dev):
    """The launches of nf_mesh_smooth_adjacency into fresh buffers: row_start, the two arrays of 6 F entries (the first E written),
    boundary and the device counts {E, boundary vertices}."""
    ws, ws_bytes = _mesh_smooth_workspace(lib, n_vertices, n_faces, dev, "mesh_adjacency")
    row_start = torch.empty(n_vertices + 1, dtype=torch.int32, device=dev)
    neighbours = torch.empty(max(6 * n_faces, 1), dtype=torch.int32, device=dev)       # never NULL: the pass takes the table of a mesh without faces
    multiplicity = torch.empty(max(6 * n_faces, 1), dtype=torch.int32, device=dev)
    boundary = torch.empty(n_vertices, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    H.check(lib.nf_mesh_smooth_adjacency(H.ptr(faces), n_vertices, n_faces, H.ptr(ws), ws_bytes, H.ptr(row_start), H.ptr(neighbours), H.ptr(multiplicity),
                                         H.ptr(boundary), H.ptr(counts), H.stream_ptr(dev)), "nf_mesh_smooth_adjacency")
    return row_start, neighbours, multiplicity, boundary, counts


def mesh_adjacency(faces: torch.Tensor, n_vertices: int) -> MeshAdjacency:
    """The neighbours of every vertex of the mesh `faces` (F, 3) int32 over n_vertices vertices, on a ROCm device, as CSR (DESIGN.md
    "Mesh smoothing"): a face with an index outside [0, n_vertices) takes no part; a valid face (a, b, c) has the sides ab, bc, ca,
    of which those with equal ends are dropped; row v holds the distinct w != v joined to v by a side, ascending, and how many sides
    join them (a face listed twice counts twice); a vertex is on the boundary iff it ends an edge of multiplicity 1.  Built by
    csrc/nf_mesh_smooth.hip with integer arithmetic only, the same bits from run to run.  Exactly one host read: E, which sizes
    the two arrays."""
    n_vertices, n_faces = _check_faces(faces, n_vertices, "mesh_adjacency")
    _check_smooth_sizes(n_vertices, n_faces, "mesh_adjacency")
    dev = _require_same_device("mesh_adjacency", faces)
    faces = faces.detach().contiguous()
    lib = H.lib()
    with torch.cuda.device(dev):
        row_start, neighbours, multiplicity, boundary, counts = _adjacency(lib, faces, n_vertices, n_faces, dev)
        n_edges = int(counts[0].item())                                 # the one host read
    return MeshAdjacency(row_start, neighbours[:n_edges].clone(), multiplicity[:n_edges].clone(), boundary)


def _vertex_normals(lib, vertices, faces, n_vertices, n_faces, dev):
    ws, ws_bytes = _mesh_smooth_workspace(lib, n_vertices, n_faces, dev, "vertex_normals")
    out = torch.empty((n_vertices, 3), dtype=torch.float32, device=dev)
    H.check(lib.nf_mesh_smooth_normals(H.ptr(vertices), H.ptr(faces), n_vertices, n_faces, H.ptr(ws), ws_bytes, H.ptr(out), H.stream_ptr(dev)),
            "nf_mesh_smooth_normals")
    return out


def vertex_normals(vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """(V, 3) float32 unit normals of the mesh's vertices from its faces: per valid face (p[b] - p[a]) x (p[c] - p[a]), per vertex the
    sum of those vectors over the faces that hold it (each face once, in ascending face order -- the same bits from run to run),
    divided by its length; the zero vector where the sum is zero or not finite (ops.isosurface's convention), as for a vertex no
    face uses.  The faces of ops.isosurface are counter-clockwise seen from lower density, so these point the way its normals do.
    No host read."""
    n_vertices, n_faces = _check_smooth_mesh(vertices, faces, "vertex_normals")
    dev = _require_same_device("vertex_normals", vertices, faces)
    vertices, faces = vertices.detach().contiguous(), faces.detach().contiguous()
    lib = H.lib()
    with torch.cuda.device(dev):
        return _vertex_normals(lib, vertices, faces, n_vertices, n_faces, dev)


def smooth_mesh(vertices: torch.Tensor, faces: torch.Tensor, normals: Optional[torch.Tensor] = None, *, iterations: int = 10, lam: float = 0.5,
                mu: float = -0.53, fix_boundary: bool = True):
    """Taubin's lambda | mu smoothing of a mesh on a ROCm device (DESIGN.md "Mesh smoothing").  Every iteration is a pass with `lam`
    and then, unless mu == 0, a pass with `mu`; a pass moves every vertex by its factor times (the mean of its neighbours - itself),
    all vertices at once from the positions before the pass.  0 < lam <= 1 shrinks, -1 <= mu <= 0 inflates again: mu < -lam is what
    keeps the volume (the defaults are Taubin's 0.5 and -0.53), and mu = 0 is plain Laplacian smoothing, which shrinks.  With
    fix_boundary (the default) the vertices of the mesh's open border -- the ends of edges that only one face side uses -- stay
    where they are, so a surface cut by the extraction box keeps its cut.  Vertices without neighbours stay too.  Returns
    (vertices, faces, normals or None, MeshSmoothStats): faces as given; normals, if given, are replaced by vertex_normals of the
    smoothed positions (the given ones belong to positions that no longer exist).  iterations = 0 returns the inputs as they are
    and launches nothing (the stats then hold zeros).  Sums run in ascending neighbour order without float atomics: the same bits
    from run to run.  Exactly one host read (the counts of the stats)."""
    n_vertices, n_faces, iterations, lam, mu = _check_smooth_args(vertices, faces, normals, iterations, lam, mu, "smooth_mesh")
    dev = _require_same_device("smooth_mesh", vertices, faces, normals)
    if iterations == 0:
        return vertices, faces, normals, MeshSmoothStats(0, 0, 0, 0)
    vertices_in, faces_in = vertices.detach().contiguous(), faces.detach().contiguous()
    lib = H.lib()
    with torch.cuda.device(dev):
        row_start, neighbours, _, boundary, counts = _adjacency(lib, faces_in, n_vertices, n_faces, dev)
        out, tmp = torch.empty_like(vertices_in), torch.empty_like(vertices_in)
        H.check(lib.nf_mesh_smooth_run(H.ptr(vertices_in), n_vertices, H.ptr(row_start), H.ptr(neighbours), H.ptr(boundary) if fix_boundary else 0, iterations,
                                       lam, mu, H.ptr(tmp), H.ptr(out), H.stream_ptr(dev)), "nf_mesh_smooth_run")
        out_n = None if normals is None else _vertex_normals(lib, out, faces_in, n_vertices, n_faces, dev)
        n_edges, n_boundary = counts.tolist()                           # the one host read
    return out, faces, out_n, MeshSmoothStats(n_edges, n_boundary, n_boundary if fix_boundary else 0, iterations * (2 if mu != 0.0 else 1))


# ---------------------------------------------------------------------------------------- decimation of a mesh by vertex clustering
MESH_DECIMATE_MAX = 2 ** 30                      # nfd::MAX_ELEMENTS of csrc/nf_mesh_decimate.hip: V and F, so that ids and table slots fit 31 bits


class MeshDecimateStats(NamedTuple):
    vertices: int
    kept_vertices: int
    faces: int
    kept_faces: int
    degenerate_faces: int                        # valid faces with two corners in one cluster
    coincident_faces: int                        # non-degenerate valid faces not kept: the others of a vertex set, both sides of a collapsed sheet
    invalid_faces: int                           # faces with an index outside [0, V)
    unclustered_vertices: int                    # NaN, infinite or past the 2^21 cells per axis: each a cluster of its own
    largest_cluster: int                         # members of the largest cluster


def _check_decimate_args(vertices, faces, normals, cell, origin, what: str):
    """Everything decimate_mesh can refuse without a device; returns (V, F, cell, origin), the last two as three float32 each."""
    _check_vertices(vertices, what)
    n_vertices, n_faces = _check_faces(faces, vertices.shape[0], what)
    _check_normals(normals, vertices, what)
    if n_vertices > MESH_DECIMATE_MAX or n_faces > MESH_DECIMATE_MAX:
        raise ValueError(f"{what}: V and F lie in [0, 2^30] (ids and table slots fit 31 bits), got V = {n_vertices} and F = {n_faces}")
    try:
        if isinstance(cell, (bool, str)) or isinstance(origin, (bool, str)):
            raise TypeError
        cell32, origin32 = np.asarray(cell, dtype=np.float32).reshape(-1), np.asarray(origin, dtype=np.float32).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: cell is one number or three and origin three numbers, got {cell!r} and {origin!r}")
    if cell32.size == 1:
        cell32 = np.repeat(cell32, 3)
    if cell32.size != 3 or origin32.size != 3:
        raise ValueError(f"{what}: cell is one number or three and origin three numbers, got {cell!r} and {origin!r}")
    if not bool(np.all(np.isfinite(cell32) & (cell32 > 0))) or not bool(np.all(np.isfinite(origin32))):
        raise ValueError(f"{what}: every cell size is finite and > 0 and the origin finite (in float32), got cell = {cell!r} and origin = {origin!r}")
    return n_vertices, n_faces, cell32, origin32


def decimate_mesh(vertices: torch.Tensor, faces: torch.Tensor, normals: Optional[torch.Tensor] = None, *, cell, origin=(0.0, 0.0, 0.0)):
    """A lighter mesh by vertex clustering on a ROCm device (DESIGN.md "Mesh decimation"): the vertices that fall into one cell of the
    lattice origin + cell * (i, j, k) -- `cell` one number or three, in the mesh's units -- become one vertex at their mean (taken
    in the cell's 2^30 fixed point, so it does not depend on the order of the sum; a vertex alone in its cell keeps its floats bit
    for bit).  A face becomes the triple of its corners' clusters; it goes if two corners share a cluster, and of the faces that end
    on one vertex set the one of the majority orientation with the smallest id stays, or none where both orientations are as many
    (the two sides of a collapsed sheet cancel).  Kept faces keep their order and winding; clusters no kept face uses are dropped,
    which includes vertices no face used.  A NaN or infinite vertex, or one past 2^20 cells from the origin, is a cluster of its
    own; a face with an index outside [0, V) takes no part.  A closed mesh usually stays closed and keeps its Euler characteristic;
    vertex clustering never guarantees it.

    Returns (vertices, faces, normals or None, vertex_map, MeshDecimateStats): vertex_map (V,) int32 holds the new id of every old
    vertex's cluster, -1 for a dropped one -- what carries a caller's own attributes across; normals, if given, are replaced by
    vertex_normals of the result (nothing is averaged).  An empty result is made of (0, 3) tensors.  Integer atomics only
    (csrc/nf_mesh_decimate.hip): the same bits from run to run.  Exactly one host read here (the counts that size the outputs)."""
    n_vertices, n_faces, cell32, origin32 = _check_decimate_args(vertices, faces, normals, cell, origin, "decimate_mesh")
    dev = _require_same_device("decimate_mesh", vertices, faces, normals)
    vertices_in, faces_in = vertices.detach().contiguous(), faces.detach().contiguous()
    lib = H.lib()
    ws, ws_bytes = _workspace(lib, "nf_mesh_decimate_workspace_bytes", (n_vertices, n_faces), dev,
                              f"decimate_mesh: {n_vertices} vertices and {n_faces} faces are past the plan of csrc/nf_mesh_decimate.hip (both at most 2^30)")
    c_origin, c_cell = (C.c_float * 3)(*origin32.tolist()), (C.c_float * 3)(*cell32.tolist())
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        stream = H.stream_ptr(dev)
        H.check(lib.nf_mesh_decimate_count(H.ptr(vertices_in), H.ptr(faces_in), n_vertices, n_faces, C.addressof(c_origin), C.addressof(c_cell), H.ptr(ws),
                                           ws_bytes, H.ptr(counts), stream), "nf_mesh_decimate_count")
        kept_v, kept_f, degenerate, coincident, invalid, unclustered, largest, overflow = counts.tolist()       # the one host read
        if overflow:
            raise RuntimeError("decimate_mesh: a hash set of csrc/nf_mesh_decimate.hip ran full, which its load of at most 0.5 excludes: nothing is returned")
        if normals is not None:
            _check_smooth_sizes(kept_v, kept_f, "decimate_mesh (the normals of the result)")
        out_v = torch.empty((kept_v, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((kept_f, 3), dtype=torch.int32, device=dev)
        vertex_map = torch.empty(n_vertices, dtype=torch.int32, device=dev)
        if n_vertices:
            H.check(lib.nf_mesh_decimate_emit(H.ptr(vertices_in), H.ptr(faces_in), n_vertices, n_faces, C.addressof(c_origin), C.addressof(c_cell),
                                              H.ptr(ws), ws_bytes, H.ptr(out_v), kept_v, H.ptr(out_f), kept_f, H.ptr(vertex_map), stream),
                    "nf_mesh_decimate_emit")
        out_n = None
        if normals is not None:
            out_n = _vertex_normals(lib, out_v, out_f, kept_v, kept_f, dev) if kept_v else torch.empty((0, 3), dtype=torch.float32, device=dev)
    return out_v, out_f, out_n, vertex_map, MeshDecimateStats(n_vertices, kept_v, n_faces, kept_f, degenerate, coincident, invalid, unclustered, largest)


# ---------------------------------------------------------------------------------------- per-vertex radiance of a mesh
MESH_COLOUR_MAX_SAMPLES = 64                    # nfk::MAX_SAMPLES of csrc/nf_mesh_colour.hip


class MeshColours(NamedTuple):
    colours: torch.Tensor                        # (V, 3) float32 in [0, 1]
    opacity: torch.Tensor                        # (V,) float32: what the shell through the vertex absorbs; below min_opacity the colour is the middle sample's


def _check_colour_args(samples, depth, pose, view_z, what: str):
    """What the colour pass can refuse without a device; returns (samples, depth as float32, view_z as float32 or None)."""
    try:
        whole = not isinstance(samples, bool) and int(samples) == samples and 1 <= int(samples) <= MESH_COLOUR_MAX_SAMPLES
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole:
        raise ValueError(f"{what}: samples is a whole number in [1, {MESH_COLOUR_MAX_SAMPLES}], got {samples!r}")
    try:
        depth32 = float(np.float32(depth))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: depth is a number, got {depth!r}")
    if not depth32 >= 0.0:                                                          # a NaN fails
        raise ValueError(f"{what}: depth is the half-thickness of the shell, at least 0, got {depth!r}")
    if (pose is None) == (view_z is None):
        raise ValueError(f"{what}: exactly one of pose (a camera-to-world (3, 4) or (4, 4) tensor) and view_z (a number) is given")
    if pose is not None and (not torch.is_tensor(pose) or pose.dtype != torch.float32 or tuple(pose.shape) not in ((3, 4), (4, 4))):
        raise ValueError(f"{what}: pose is a float32 tensor of shape (3, 4) or (4, 4)")
    return int(samples), depth32, None if view_z is None else float(np.float32(view_z))


def mesh_colour_step(depth, samples: int) -> float:
    """The spacing of the samples of mesh_colour_rays, as the kernel forms it in float32: 2 * (depth / samples)."""
    return float(np.float32(2.0) * (np.float32(depth) / np.float32(samples)))


def mesh_colour_rays(vertices: torch.Tensor, normals: torch.Tensor, *, samples: int, depth: float, pose: Optional[torch.Tensor] = None, view_z=None):
    """The short ray through the surface at every vertex of a mesh on a ROCm device (DESIGN.md "Mesh colours"), in the layout
    model.hip_forward takes with the vertices as origins: (rd (V, 3), rd_view (V, 3), z (V, samples)).  rd = -normals (the normals
    point towards lower density); z[k] = float(2 k - samples + 1) * (depth / samples), from outside to inside, the middle sample of
    an odd count on the vertex; rd_view is the direction the camera `pose` (camera-to-world [R | o]) would have fed the network
    for the pixel that sees the vertex, (v - o) / d with d the vertex's distance along the camera's axis -- the central ray
    -R[:, 2] for a vertex that is not in front of the camera -- or (0, 0, view_z) for every vertex.  Every float32 operation
    rounded on its own (tests/mesh_colour_ref.py gives the same bits).  No host read."""
    _check_vertices(vertices, "mesh_colour_rays")
    _check_normals(normals, vertices, "mesh_colour_rays")
    if normals is None:
        raise ValueError("mesh_colour_rays: normals must be a float32 tensor of the vertices' shape")
    samples, depth, view_z = _check_colour_args(samples, depth, pose, view_z, "mesh_colour_rays")
    dev = _require_same_device("mesh_colour_rays", vertices, normals, pose)
    n_vertices = int(vertices.shape[0])
    vertices, normals = vertices.detach().contiguous(), normals.detach().contiguous()
    pose = None if pose is None else pose.detach().contiguous()
    rd, rd_view = torch.empty_like(vertices), torch.empty_like(vertices)
    z = torch.empty((n_vertices, samples), dtype=torch.float32, device=dev)
    lib = H.lib()
    with torch.cuda.device(dev):
        H.check(lib.nf_mesh_colour_rays(H.ptr(vertices), H.ptr(normals), n_vertices, H.ptr(pose), 4, view_z or 0.0, samples, depth, H.ptr(rd),
                                        H.ptr(rd_view), H.ptr(z), H.stream_ptr(dev)), "nf_mesh_colour_rays")
    return rd, rd_view, z


def mesh_colour_integrate(raw: torch.Tensor, step: float, min_opacity: float = 1e-3) -> MeshColours:
    """The composite of the network's output raw (V, K, 4) along the rays of mesh_colour_rays, samples `step` apart: sigma =
    relu(raw[..., 3]), alpha = 1 - exp(-sigma * step), w_k = alpha_k * prod_{j<k}(1 - alpha_j), opacity = sum w, colours = sum w *
    sigmoid(raw[..., :3]) / opacity where opacity >= min_opacity, else the sigmoid of sample K // 2 (the vertex itself for an odd K).
    No background sample and nothing added at the far end, unlike the camera-ray integrator.  Sums in ascending k, no float
    atomics: the same bits from run to run.  A min_opacity of 0 divides 0 by 0 where nothing absorbs.  No host read."""
    if not torch.is_tensor(raw) or raw.dtype != torch.float32 or raw.dim() != 3 or raw.shape[2] != 4 or not 1 <= raw.shape[1] <= MESH_COLOUR_MAX_SAMPLES:
        raise ValueError(f"mesh_colour_integrate: raw is a float32 tensor of shape (V, K, 4) with K in [1, {MESH_COLOUR_MAX_SAMPLES}]")
    step, min_opacity = float(np.float32(step)), float(np.float32(min_opacity))
    if not step >= 0.0 or min_opacity != min_opacity:
        raise ValueError(f"mesh_colour_integrate: step is at least 0 and min_opacity a number, got {step!r} and {min_opacity!r}")
    dev = _require_same_device("mesh_colour_integrate", raw)
    raw = raw.detach().contiguous()
    n_vertices, samples = int(raw.shape[0]), int(raw.shape[1])
    colours = torch.empty((n_vertices, 3), dtype=torch.float32, device=dev)
    opacity = torch.empty((n_vertices,), dtype=torch.float32, device=dev)
    lib = H.lib()
    with torch.cuda.device(dev):
        H.check(lib.nf_mesh_colour_integrate(H.ptr(raw), n_vertices, samples, step, min_opacity, H.ptr(colours), H.ptr(opacity), H.stream_ptr(dev)),
                "nf_mesh_colour_integrate")
    return MeshColours(colours, opacity)


def vertex_colours(forward, vertices: torch.Tensor, normals: torch.Tensor, *, samples: int = 8, depth: float, pose: Optional[torch.Tensor] = None,
                   view_z=None, min_opacity: float = 1e-3, chunk_points: int = 1 << 22) -> MeshColours:
    """The colour of every vertex of a mesh under the radiance field `forward(ro, rd, z, rd_view) -> raw (n, samples, 4)`:
    mesh_colour_rays, the field, mesh_colour_integrate, in slabs of max(1, chunk_points // samples) whole vertices.  Every vertex
    is on its own, so the result does not depend on chunk_points.  No vertices: empty tensors, and nothing is launched."""
    _check_vertices(vertices, "vertex_colours")
    _check_normals(normals, vertices, "vertex_colours")
    samples, depth, _ = _check_colour_args(samples, depth, pose, view_z, "vertex_colours")
    dev = _require_same_device("vertex_colours", vertices, normals, pose)
    n_vertices = int(vertices.shape[0])
    colours = torch.empty((n_vertices, 3), dtype=torch.float32, device=dev)
    opacity = torch.empty((n_vertices,), dtype=torch.float32, device=dev)
    slab = max(1, int(chunk_points) // samples)
    step = mesh_colour_step(depth, samples)
    vertices, normals = vertices.detach().contiguous(), normals.detach().contiguous()
    for v0 in range(0, n_vertices, slab):
        ro = vertices[v0:v0 + slab]
        rd, rd_view, z = mesh_colour_rays(ro, normals[v0:v0 + slab], samples=samples, depth=depth, pose=pose, view_z=view_z)
        colours[v0:v0 + slab], opacity[v0:v0 + slab] = mesh_colour_integrate(forward(ro, rd, z, rd_view), step, min_opacity)
    return MeshColours(colours, opacity)


# ---------------------------------------------------------------------------------------- sparse evaluation of a dense grid
class SparseGridStats(NamedTuple):
    bricks: int                                  # bricks of the grid
    seed_bricks: int                             # bricks whose 8 corners are not all on one side of the level (by more than the margin)
    active_bricks: int                           # bricks within `dilate` bricks of a seed
    points: int                                  # points of the grid
    evaluated_points: int                        # points fn was asked for: the coarse lattice and the points of the active bricks


def _resolution(resolution):
    r = [int(resolution)] * 3 if np.isscalar(resolution) else [int(x) for x in resolution]
    if len(r) == 1:
        r = r * 3
    if len(r) != 3 or min(r) < 2:
        raise ValueError(f"resolution: one number or (nx, ny, nz), at least 2 points per axis, got {resolution}")
    return r


def check_sparse_grid_args(brick, margin, dilate, what: str = "sparse_grid"):
    """(brick, margin, dilate) as int, float, int; ValueError for brick < 2, margin < 0 (or NaN) and dilate < 0."""
    if int(brick) != brick or int(brick) < 2:
        raise ValueError(f"{what}: brick is a whole number of cells, at least 2, got {brick}")
    if not float(margin) >= 0.0:
        raise ValueError(f"{what}: margin must be >= 0, got {margin}")
    if int(dilate) != dilate or int(dilate) < 0:
        raise ValueError(f"{what}: dilate is a whole number of bricks, at least 0, got {dilate}")
    return int(brick), float(margin), int(dilate)


def sparse_grid(fn, level: float, lo, hi, resolution, *, brick: int = 8, margin: float = 0.0, dilate: int = 1, chunk_points: int = 1 << 22,
                device=None):
    """The grid (nz, ny, nx) of fn on the `resolution` points spanning the box [lo, hi] (the points of nerf.mesh.grid_axes), with fn
    evaluated only near the surface fn == level (DESIGN.md "Sparse density grid"; csrc/nf_sparse_grid.hip).  The grid is cut into
    bricks of `brick` cells.  fn is first asked for the brick corners (the coarse lattice); a brick is a seed unless all 8 corners
    are > level + margin or all are < level - margin; bricks within `dilate` bricks of a seed are active, and fn is asked for every
    point of the active bricks.  Every other point holds +inf (its bricks' corners are inside, fn > level) or -inf (outside), which
    ops.isosurface takes as any other value.

    Provided every brick that is no seed really lies on one side of the level, and dilate >= 1, ops.isosurface gives on this grid
    the vertices, faces and normals it gives on the dense grid, bit for bit (dilate = 0 keeps vertices and faces).  A feature thinner
    than a brick that passes between the lattice points is missed: `margin` makes bricks whose corners come near the level seeds too.

    fn maps an (n, 3) float32 device tensor to (n,) float32; it is called with at most `chunk_points` points per call, first for the
    lattice and then for the other points, each in ascending linear index, and never twice for one point.  One host read: the three
    counts.  Returns (grid, SparseGridStats); `device` defaults to the current ROCm device."""
    nx, ny, nz = _resolution(resolution)
    brick, margin, dilate = check_sparse_grid_args(brick, margin, dilate)
    chunk = int(chunk_points)
    if chunk < 1:
        raise ValueError(f"sparse_grid: chunk_points must be at least 1, got {chunk_points}")
    lo32, hi32 = _box(lo, hi, "sparse_grid")
    lib = H.lib()
    b = min(brick, 0x7fffffff)
    _, ws_bytes = _workspace(lib, "nf_sparse_grid_workspace_bytes", (nx, ny, nz, b), None, f"sparse_grid: a grid of {nx} x {ny} x {nz} points is past the plan "
                             "of csrc/nf_isosurface.hip (7 * points and 12 * cells stay below 2^31: vertex and face ids are int32)")
    if not torch.cuda.is_available():
        raise RuntimeError("nerf (MI355X build): sparse_grid runs on a ROCm device; there is no CPU path in this package")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    bricks_per_axis = [-(-(n - 1) // brick) for n in (nx, ny, nz)]
    n_bricks = int(np.prod(bricks_per_axis))
    n_lattice = int(np.prod([m + 1 for m in bricks_per_axis]))
    c_lo, c_hi = (C.c_float * 3)(*lo32.tolist()), (C.c_float * 3)(*hi32.tolist())
    grid = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)

    def evaluate(coords, index):
        for c0 in range(0, coords.shape[0], chunk):
            pts, idx = coords[c0:c0 + chunk], index[c0:c0 + chunk]
            val = fn(pts)
            if not torch.is_tensor(val) or val.shape != (pts.shape[0],) or val.device != grid.device:
                raise ValueError(f"sparse_grid: fn must map ({pts.shape[0]}, 3) points to ({pts.shape[0]},) values on {grid.device}")
            val = val.detach().to(torch.float32).contiguous()
            H.check(lib.nf_sparse_grid_scatter(H.ptr(val), H.ptr(idx), idx.shape[0], H.ptr(grid), nx, ny, nz, H.stream_ptr(dev)),
                    "nf_sparse_grid_scatter")

    with torch.cuda.device(dev):
        index = torch.empty(n_lattice, dtype=torch.int32, device=dev)
        coords = torch.empty((n_lattice, 3), dtype=torch.float32, device=dev)
        H.check(lib.nf_sparse_grid_lattice(nx, ny, nz, b, C.addressof(c_lo), C.addressof(c_hi), H.ptr(index), H.ptr(coords), n_lattice,
                                           H.stream_ptr(dev)), "nf_sparse_grid_lattice")
        evaluate(coords, index)
        H.check(lib.nf_sparse_grid_classify(H.ptr(grid), nx, ny, nz, b, float(level), margin, min(dilate, 0x7fffffff), H.ptr(ws), ws_bytes,
                                            H.stream_ptr(dev)), "nf_sparse_grid_classify")
        H.check(lib.nf_sparse_grid_mark(nx, ny, nz, b, H.ptr(ws), ws_bytes, H.ptr(counts), H.stream_ptr(dev)), "nf_sparse_grid_mark")
        n_seed, n_active, n_more = counts.tolist()                       # the one host read
        index = torch.empty(n_more, dtype=torch.int32, device=dev)
        coords = torch.empty((n_more, 3), dtype=torch.float32, device=dev)
        H.check(lib.nf_sparse_grid_emit(H.ptr(grid), nx, ny, nz, b, C.addressof(c_lo), C.addressof(c_hi), H.ptr(ws), ws_bytes, H.ptr(index),
                                        H.ptr(coords), n_more, H.stream_ptr(dev)), "nf_sparse_grid_emit")
        evaluate(coords, index)
    return grid, SparseGridStats(n_bricks, n_seed, n_active, nx * ny * nz, n_lattice + n_more)
