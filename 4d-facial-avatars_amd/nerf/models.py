"""Model classes of the reference's nerf/models.py that lie on the NeRFace hot path.

`ConditionalBlendshapePaperNeRFModel` (reference nerf/models.py:189-261, the model of 88 of the 108
`type:` entries under config/) keeps the reference's constructor signature, parameter names, shapes and
default initialisation, so checkpoints (`model_{coarse,fine}_state_dict`) load unchanged.  Its compute is
the fused HIP kernel K4: `run_one_iter_of_nerf` hands the module to the kernel wrapper, which reads the
live parameter storages (no copies besides the cached fragment-ordered image).
"""
from __future__ import annotations

import torch

from . import ops
from .ops import BSHAPE_KEYS, CBSHAPE_KEYS, LCODE_KEYS, SMALLER_KEYS  # noqa: F401  (parameter orders of the other families, as include/nerface_hip.h names them)


class _FusedNeRFModel(torch.nn.Module):
    """What run_one_iter_of_nerf, run_network and the benches call on a fused model family.  A subclass names its family
    (FAMILY, an ops.MLPFamily) and says which geometries the kernels serve (fused_supported)."""

    FAMILY: ops.MLPFamily
    NEEDS_LATENT = True           # forward() without latent_code raises (False: the class's reference forward ignores it)

    def hip_param_list(self):
        sd = dict(self.named_parameters())
        return [sd[k] for k in self.FAMILY.keys]

    def hip_weights(self) -> ops.MLPWeights:
        params = self.hip_param_list()
        hw = self.__dict__.get("_hip_weights")
        if hw is None or any(a is not b for a, b in zip(hw._params, params)):
            hw = self._hip_weights = ops.MLPWeights(self.FAMILY, params)
        return hw

    def hip_forward(self, ro, rd, z, rd_view, expr, latent, near, far, need_grad, live_only=False):
        """raw (R, S, 4) for the points ro + rd*z in the arithmetic of nerf.set_mlp_precision; `state` is what hip_backward needs
        (None when no gradient is wanted).  live_only: the colour of a sample without density, other than a ray's last, may come
        back as 0.0 (ops.mlp_fwd_live) -- for a caller that integrates `raw` without noise; needs ops.live_colour_kernel(FAMILY).
        live_only="gated": such a sample may, besides, come back with ANY NEGATIVE density in place of its own (ops.mlp_fwd_gated:
        fc_feat is skipped where a bound proves the density negative) -- the same caller, the same outputs of the integrator."""
        ops.check_conditioning(expr, latent)
        fam, hw, prec = self.FAMILY, self.hip_weights(), ops.get_mlp_precision()
        fam.require_precision(prec)
        if live_only:
            if need_grad or not ops.live_colour_kernel(fam):
                raise ValueError("live_only is an exact-f32 inference option of the families in ops.LIVE_FAMILIES (ops.live_colour_kernel)")
            packed = hw.get()
            if live_only == "gated":
                return ops.mlp_fwd_gated(fam, packed, hw.get_bound(), ops.mlp_condition(fam, packed, expr, latent, near, far), ro, rd, z, rd_view), None
            return ops.mlp_fwd_live(fam, packed, ops.mlp_condition(fam, packed, expr, latent, near, far), ro, rd, z, rd_view), None
        packed = hw.get()
        cond = ops.mlp_condition(fam, packed, expr, latent, near, far)
        if need_grad:
            ops.require_trainable_precision()
            pb = hw.get_bf16() if prec == "bf16x3" else None
            ph = hw.get_f16() if prec == "f16x3" else None
            if ph is not None:
                ops.f16_guard(self, ro, rd, z, rd_view, expr, latent, near, far, training=True)
            raw, (saved,) = ops.mlp_fwd_train(fam, packed, cond, ro, rd, z, rd_view, packed_b=pb, packed_h=ph)
            return raw, (packed, cond, saved, "f16" if ph is not None else pb is not None)
        if prec in ops.F16_MODES:
            ops.f16_guard(self, ro, rd, z, rd_view, expr, latent, near, far, training=False)
        image = {"f32": hw.get, "bf16x3": hw.get_bf16, "f16x3": hw.get_f16, "f16x2": hw.get_f16}[prec]()
        return ops.mlp_fwd(fam, prec, image, cond, ro, rd, z, rd_view), None

    def hip_sigma(self, ro, rd, z, expr, latent, near, far):
        """Raw sigma (R, S) for the points ro + rd*z in the arithmetic of nerf.set_mlp_precision: hip_forward(..., need_grad=False)[0][..., 3]
        bit for bit, from the kernel that ends with the layer that yields the density.  Inference only; same precision handling,
        conditioning check and f16 guard as hip_forward's inference branch."""
        ops.check_conditioning(expr, latent)
        fam, hw, prec = self.FAMILY, self.hip_weights(), ops.get_mlp_precision()
        fam.require_precision(prec)
        packed = hw.get()
        cond = ops.mlp_condition(fam, packed, expr, latent, near, far)
        if prec in ops.F16_MODES:
            ops.f16_guard(self, ro, rd, z, None, expr, latent, near, far, training=False)
        image = {"f32": hw.get, "bf16x3": hw.get_bf16, "f16x3": hw.get_f16, "f16x2": hw.get_f16}[prec]()
        return ops.mlp_sigma(fam, prec, image, cond, ro, rd, z)

    def hip_backward(self, state, z, d_raw):
        """d_raw -> ([gradients in hip_param_list() order, None where autograd gives the reference None], d_latent (32))."""
        packed, cond, saved, split = state
        return ops.mlp_bwd(self.FAMILY, self.hip_weights(), packed, cond, z, d_raw, saved, split=split)

    def forward(self, x, expr=None, latent_code=None, **kwargs):
        """The reference's forward (paper model M:236-261, second family M:590-636, smaller paper model M:313-338) on pre-encoded inputs x (N, 87) =
        [PE10(xyz) | PE4(dirs)] -> (N, 4), as run_network calls it (T:9-33).  Inference only (kernel <prefix>_forward_encoded);
        training goes through run_one_iter_of_nerf, whose fused kernels own the backward."""
        if not self.fused_supported() or expr is None or (latent_code is None and self.NEEDS_LATENT):
            raise NotImplementedError("forward() is built for the NeRFace geometry and needs expr and latent_code")
        if latent_code is None:                      # a class without a latent code (M:821, M:935): the kernels ignore it
            latent_code = torch.zeros(32, dtype=torch.float32, device=x.device)
        if torch.is_grad_enabled() and (x.requires_grad or latent_code.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(f"{type(self).__name__}.forward has no autograd on the MI355X build: train through "
                                      "nerf.run_one_iter_of_nerf(...), or call forward under torch.no_grad()")
        return ops.mlp_forward_encoded(self.hip_weights(), x, expr, latent_code)


def _point_query(model, points, expr, latent_code, what: str):
    """The guards nerf.density, nerf.radiance and nerf.vertex_colours share -- a fused model of the NeRFace geometry, ROCm tensors,
    (N, 3) points, no autograd -- and the conditioning as the kernels take it: (expr (76,), latent (32,)), float32 and contiguous."""
    if not isinstance(model, _FusedNeRFModel) or not model.fused_supported() or (latent_code is None and model.NEEDS_LATENT):
        raise NotImplementedError(f"{what}() is built for the NeRFace geometry and needs expr and latent_code")
    if not (torch.is_tensor(points) and points.is_cuda and torch.is_tensor(expr) and expr.is_cuda):
        raise RuntimeError("nerf (MI355X build): tensors must live on a ROCm device (`device='cuda'`); there is no CPU path in this package")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("expected points of shape (N, 3)")
    if latent_code is None:
        latent_code = torch.zeros(32, dtype=torch.float32, device=points.device)
    if torch.is_grad_enabled() and (points.requires_grad or latent_code.requires_grad or any(p.requires_grad for p in model.parameters())):
        raise NotImplementedError(f"{type(model).__name__}.forward has no autograd on the MI355X build: train through "
                                  "nerf.run_one_iter_of_nerf(...), or call forward under torch.no_grad()")
    return ops._c(expr.detach().to(torch.float32)).reshape(-1), ops._c(latent_code.detach().to(torch.float32)).reshape(-1)


def density(model, points, expr, latent_code=None):
    """Raw density (N,) of a fused model at arbitrary points (N, 3) for one expression (and latent code): raw[..., 3], before the
    ReLU, in the arithmetic of nerf.set_mlp_precision.  The density depends on neither a view direction nor near / far, so none is
    asked for: the points go through model.hip_sigma as ray origins with a zero direction (ro + 0 * 0 is ro exactly).  Inference
    only; tensors on a ROCm device.  latent_code=None is allowed exactly for the classes whose forward ignores it."""
    expr, latent = _point_query(model, points, expr, latent_code, "density")
    n = points.shape[0]
    if n == 0:
        return torch.empty((0,), dtype=torch.float32, device=points.device)
    ro = ops._c(points.detach().to(torch.float32))
    ops.bump_pack_epoch()              # as run_one_iter_of_nerf: a weight image never outlives one call (ops.MLPWeights)
    sigma = model.hip_sigma(ro, torch.zeros_like(ro), torch.zeros((n, 1), dtype=torch.float32, device=ro.device), expr, latent, 0.0, 0.0)
    if ops.get_mlp_precision() in ops.F16_MODES:
        ops.check_f16_range(model)
    return sigma.reshape(n)


def radiance(model, points, view, expr, latent_code=None, *, near, far):
    """Raw network output (N, 4) -- colour before the sigmoid, density before the ReLU -- of a fused model at arbitrary points (N, 3)
    for one expression (and latent code), in the arithmetic of nerf.set_mlp_precision: density's sibling, with the same guards.
    `view` is (N, 3), or (3,) for all points, and is handed to the network as the view direction; under Quirk Q1 the network's
    "direction" input is PE4(view z, near, far), so only view[..., 2] reaches it, and near / far are network inputs and have no
    default.  The points go through model.hip_forward as ray origins with a zero direction, never with live_only: the result is
    the full forward's output bit for bit.  A family without the arithmetic set refuses by name (NotImplementedError)."""
    expr, latent = _point_query(model, points, expr, latent_code, "radiance")
    n = points.shape[0]
    if not torch.is_tensor(view) or not view.is_cuda or tuple(view.shape) not in ((3,), (n, 3)):
        raise ValueError(f"radiance: view is a ROCm tensor of shape (3,) or (N, 3) = ({n}, 3), got {tuple(view.shape) if torch.is_tensor(view) else view!r}")
    if n == 0:
        return torch.empty((0, 4), dtype=torch.float32, device=points.device)
    ro = ops._c(points.detach().to(torch.float32))
    rd_view = ops._c(view.detach().to(torch.float32).expand(n, 3))
    ops.bump_pack_epoch()              # as density
    raw, _ = model.hip_forward(ro, torch.zeros_like(ro), torch.zeros((n, 1), dtype=torch.float32, device=ro.device), rd_view, expr, latent,
                               float(near), float(far), need_grad=False)
    if ops.get_mlp_precision() in ops.F16_MODES:
        ops.check_f16_range(model)
    return raw.reshape(n, 4)


class ConditionalBlendshapePaperNeRFModel(_FusedNeRFModel):
    r"""NeRFace paper model (Fig. 7 of the paper; reference nerf/models.py:189-261).

    x0 = [PE10(xyz) (63) | expression*1/3 (76) | latent code (32)] -> 3 x (Linear 256 + ReLU) ->
    [x0 | h] -> 3 x (Linear 256 + ReLU) -> feat = fc_feat(h) -> sigma = fc_alpha(feat);
    [feat | PE4(dir) (24)] -> 3 x (Linear 128 + ReLU) -> rgb = fc_rgb.  `layers_dir.3` exists in every
    checkpoint but is never used (Quirk Q3); num_layers / hidden_size / skip_connect_every are accepted
    and ignored exactly as in the reference (widths are hard-coded).
    """

    FAMILY = ops.PAPER

    def __init__(self, num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4,
                 include_input_xyz=True, include_input_dir=True, use_viewdirs=True, include_expression=True,
                 latent_code_dim=32):
        super().__init__()
        include_input_xyz = 3 if include_input_xyz else 0
        include_input_dir = 3 if include_input_dir else 0
        include_expression = 76 if include_expression else 0
        self.dim_xyz = include_input_xyz + 2 * 3 * num_encoding_fn_xyz
        self.dim_dir = include_input_dir + 2 * 3 * num_encoding_fn_dir
        self.dim_expression = include_expression
        self.dim_latent_code = latent_code_dim
        self.use_viewdirs = use_viewdirs
        d_in = self.dim_xyz + self.dim_expression + self.dim_latent_code
        self.layers_xyz = torch.nn.ModuleList()
        self.layers_xyz.append(torch.nn.Linear(d_in, 256))
        for i in range(1, 6):
            self.layers_xyz.append(torch.nn.Linear(d_in + 256 if i == 3 else 256, 256))
        self.fc_feat = torch.nn.Linear(256, 256)
        self.fc_alpha = torch.nn.Linear(256, 1)
        self.layers_dir = torch.nn.ModuleList()
        self.layers_dir.append(torch.nn.Linear(256 + self.dim_dir, 128))
        for _ in range(3):
            self.layers_dir.append(torch.nn.Linear(128, 128))
        self.fc_rgb = torch.nn.Linear(128, 3)
        self.relu = torch.nn.functional.relu

    def fused_supported(self) -> bool:
        """The HIP kernel is specialised to the one geometry every NeRFace config instantiates."""
        return (self.dim_xyz == 63 and self.dim_dir == 24 and self.dim_expression == 76 and self.dim_latent_code == 32
                and self.use_viewdirs)


class ConditionalBlendshapeLearnableCodeNeRFModel(_FusedNeRFModel):
    r"""Second NeRFace model family (reference nerf/models.py:529-636; 6 config entries): layer1 without activation, three
    256-wide ReLU layers, feat = relu(fc_feat(x)), sigma = fc_alpha(x), one 280 -> 128 direction layer, fc_rgb.
    Same constructor signature, parameter names and shapes as the reference, so its checkpoints load.  The MI355X build
    provides the forward and the backward (exact-f32 fused kernels) for the geometry the configs use: num_layers=4,
    hidden_size=256 (the trainer never passes skip_connect_every, TR:100-109), 10/4 encoding functions."""

    FAMILY = ops.LCODE

    def __init__(self, num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4,
                 include_input_xyz=True, include_input_dir=True, use_viewdirs=True, include_expression=True, latent_code_dim=32):
        super().__init__()
        include_input_xyz = 3 if include_input_xyz else 0
        include_input_dir = 3 if include_input_dir else 0
        include_expression = 76 if include_expression else 0
        self.dim_xyz = include_input_xyz + 2 * 3 * num_encoding_fn_xyz
        self.dim_dir = include_input_dir + 2 * 3 * num_encoding_fn_dir if use_viewdirs else 0
        self.dim_expression = include_expression
        self.skip_connect_every = skip_connect_every
        self.dim_latent_code = latent_code_dim
        self.layers_expr = None
        d_in = self.dim_xyz + self.dim_expression + self.dim_latent_code
        self.layer1 = torch.nn.Linear(d_in, hidden_size)
        self.layers_xyz = torch.nn.ModuleList()
        for i in range(num_layers - 1):
            skip = i % self.skip_connect_every == 0 and i > 0 and i != num_layers - 1
            self.layers_xyz.append(torch.nn.Linear(self.dim_xyz + hidden_size + self.dim_expression + self.dim_latent_code if skip
                                                   else hidden_size, hidden_size))
        self.use_viewdirs = use_viewdirs
        if self.use_viewdirs:
            self.layers_dir = torch.nn.ModuleList()
            self.layers_dir.append(torch.nn.Linear(self.dim_dir + hidden_size, hidden_size // 2))
            self.fc_alpha = torch.nn.Linear(hidden_size, 1)
            self.fc_rgb = torch.nn.Linear(hidden_size // 2, 3)
            self.fc_feat = torch.nn.Linear(hidden_size, hidden_size)
        else:
            self.fc_out = torch.nn.Linear(hidden_size, 4)
        self.relu = torch.nn.functional.relu
        self.sigmoid = torch.sigmoid

    def fused_supported(self) -> bool:
        return (self.use_viewdirs and self.dim_xyz == 63 and self.dim_dir == 24 and self.dim_expression == 76
                and self.dim_latent_code == 32 and self.layer1.out_features == 256 and len(self.layers_xyz) == 3
                and all(l.in_features == 256 for l in self.layers_xyz))


class _BlendshapeNoCodeNeRFModel(_FusedNeRFModel):
    """What the two blendshape classes without a learnable code share: the second family's trunk behind a layer1 that reads
    [PE(xyz) | conditioning vector].  The reference's constructor signature (no latent_code_dim), parameter names, shapes and
    registration order.  A latent code handed to forward / hip_forward is accepted and ignored, as the reference does (it arrives in
    **kwargs); its gradient from these models is zero -- only the trainer's regulariser (nerf.training_loss) moves it."""

    NEEDS_LATENT = False
    DIM_CONDITION: int            # columns of layer1.weight behind the 63 of PE(xyz)

    def _build_trunk(self, num_layers, hidden_size, skip_connect_every, num_encoding_fn_xyz, num_encoding_fn_dir, include_input_xyz,
                     include_input_dir, use_viewdirs):
        self.dim_xyz = (3 if include_input_xyz else 0) + 2 * 3 * num_encoding_fn_xyz
        self.dim_dir = (3 if include_input_dir else 0) + 2 * 3 * num_encoding_fn_dir if use_viewdirs else 0
        self.skip_connect_every = skip_connect_every
        self.layer1 = torch.nn.Linear(self.dim_xyz + self.dim_expression, hidden_size)
        self.layers_xyz = torch.nn.ModuleList()
        for i in range(num_layers - 1):
            skip = i % self.skip_connect_every == 0 and i > 0 and i != num_layers - 1
            self.layers_xyz.append(torch.nn.Linear(self.dim_xyz + hidden_size + self.dim_expression if skip else hidden_size, hidden_size))
        self.use_viewdirs = use_viewdirs
        if self.use_viewdirs:
            self.layers_dir = torch.nn.ModuleList()
            self.layers_dir.append(torch.nn.Linear(self.dim_dir + hidden_size, hidden_size // 2))
            self.fc_alpha = torch.nn.Linear(hidden_size, 1)
            self.fc_rgb = torch.nn.Linear(hidden_size // 2, 3)
            self.fc_feat = torch.nn.Linear(hidden_size, hidden_size)
        else:
            self.fc_out = torch.nn.Linear(hidden_size, 4)
        self.relu = torch.nn.functional.relu
        self.sigmoid = torch.sigmoid

    def fused_supported(self) -> bool:
        return (self.use_viewdirs and self.dim_xyz == 63 and self.dim_dir == 24 and self.layer1.out_features == 256
                and self.layer1.in_features == 63 + self.DIM_CONDITION and len(self.layers_xyz) == 3
                and all(l.in_features == 256 for l in self.layers_xyz))


class ConditionalCompressedBlendshapeNeRFModel(_BlendshapeNoCodeNeRFModel):
    r"""Reference nerf/models.py:750-868 (the `*_nolcode_fixed_bg_256_compressed` configs, 6 entries): the expression goes through
    layers_expr = Linear 76 -> 38 -> 20 -> 20 with a ReLU after EACH layer and without the division by 3 (M:832-834), and layer1
    reads [PE10(xyz) (63) | e3 (20)]; behind it the second family's trunk.  dim_expression is 20 whatever include_expression says,
    as in the reference (M:779).  22 tensors; every arithmetic of nerf.set_mlp_precision.  The encoder is evaluated once per call
    on the device (nf_cbshape_condition) and trained by the backward of the same kernels' gradient scatter."""

    FAMILY = ops.CBSHAPE
    DIM_CONDITION = 20

    def __init__(self, num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4,
                 include_input_xyz=True, include_input_dir=True, use_viewdirs=True, include_expression=True):
        super().__init__()
        self.dim_expression = 20
        self.layers_expr = torch.nn.ModuleList([torch.nn.Linear(76, 38), torch.nn.Linear(38, 20), torch.nn.Linear(20, 20)])
        self._build_trunk(num_layers, hidden_size, skip_connect_every, num_encoding_fn_xyz, num_encoding_fn_dir, include_input_xyz,
                          include_input_dir, use_viewdirs)


class ConditionalBlendshapeNeRFModel(_BlendshapeNoCodeNeRFModel):
    r"""Reference nerf/models.py:872-976 (`ji_nolcode_fixed_bg_256`, `..._train_cams`; 4 entries): the second family without the
    latent code -- layer1 reads [PE10(xyz) (63) | expression*1/3 (76)].  16 tensors; every arithmetic of nerf.set_mlp_precision."""

    FAMILY = ops.BSHAPE
    DIM_CONDITION = 76

    def __init__(self, num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4,
                 include_input_xyz=True, include_input_dir=True, use_viewdirs=True, include_expression=True):
        super().__init__()
        self.dim_expression = 76 if include_expression else 0
        self.layers_expr = None
        self._build_trunk(num_layers, hidden_size, skip_connect_every, num_encoding_fn_xyz, num_encoding_fn_dir, include_input_xyz,
                          include_input_dir, use_viewdirs)


class ConditionalBlendshapePaperSmallerNeRFModel(_FusedNeRFModel):
    r"""The paper model made smaller (reference nerf/models.py:266-338; the `ji` "smaller paper model" configs): the model a user
    picks to trade quality for speed.

    x0 = [PE10(xyz) (63) | expression*1/3 (76) | latent code (32)] -> 3 x (Linear 256 + ReLU) -> [x0 | h] -> 2 x (Linear 256 + ReLU)
    -> feat = fc_feat(h) -> sigma = fc_alpha(feat); [feat | PE4(dir) (24) | expression*1/3 (76)] -> 3 x (Linear 128 + ReLU) ->
    rgb = fc_rgb.  Against the paper model: no layers_xyz.5, no dead layers_dir.3, the expression a second time in front of the
    colour branch; 22 tensors, 496,132 parameters, all live.  Constructor signature, parameter names, shapes and default
    initialisation are the reference's, so its checkpoints load unchanged; num_layers / hidden_size / skip_connect_every are
    accepted and ignored exactly as there.  Exact f32 only: under another nerf.set_mlp_precision it raises NotImplementedError.
    """

    FAMILY = ops.SMALLER

    def __init__(self, num_layers=8, hidden_size=256, skip_connect_every=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4,
                 include_input_xyz=True, include_input_dir=True, use_viewdirs=True, include_expression=True,
                 latent_code_dim=32):
        super().__init__()
        include_input_xyz = 3 if include_input_xyz else 0
        include_input_dir = 3 if include_input_dir else 0
        include_expression = 76 if include_expression else 0
        self.dim_xyz = include_input_xyz + 2 * 3 * num_encoding_fn_xyz
        self.dim_dir = include_input_dir + 2 * 3 * num_encoding_fn_dir
        self.dim_expression = include_expression
        self.dim_latent_code = latent_code_dim
        self.layers_xyz = torch.nn.ModuleList()
        self.use_viewdirs = use_viewdirs
        d_in = self.dim_xyz + self.dim_expression + self.dim_latent_code
        self.layers_xyz.append(torch.nn.Linear(d_in, 256))
        for i in range(1, 5):
            self.layers_xyz.append(torch.nn.Linear(d_in + 256 if i == 3 else 256, 256))
        self.fc_feat = torch.nn.Linear(256, 256)
        self.fc_alpha = torch.nn.Linear(256, 1)
        self.layers_dir = torch.nn.ModuleList()
        self.layers_dir.append(torch.nn.Linear(256 + self.dim_dir + self.dim_expression, 128))
        for _ in range(2):
            self.layers_dir.append(torch.nn.Linear(128, 128))
        self.fc_rgb = torch.nn.Linear(128, 3)
        self.relu = torch.nn.functional.relu

    def fused_supported(self) -> bool:
        """The HIP kernels are specialised to the geometry of the configs that use this class."""
        return (self.dim_xyz == 63 and self.dim_dir == 24 and self.dim_expression == 76 and self.dim_latent_code == 32
                and self.use_viewdirs)


class FlexibleNeRFModel(torch.nn.Module):
    r"""Reference nerf/models.py:351-422: constructor signature, parameter names, shapes and default initialisation as there, so
    its state_dicts load unchanged.

    The HIP path is built for the configuration that reads BASELINE config 1 literally ("tiny_nerf ... 4-layer MLP"):
    `FlexibleNeRFModel(num_layers=L, hidden_size=128, num_encoding_fn_xyz=10, include_input_xyz=True, use_viewdirs=False)` with
    L = 2 .. 5 (no skip connection fires below 6 layers, M:373 / 404-409):
    PE10(xyz) (63) -> layer1 (Linear 128, NO activation, M:402) -> (L - 1) x (Linear 128 + ReLU) -> fc_out (Linear 4).
    It is evaluated inside the fused tiny-path kernels (`tiny_nerf.run_one_iter_of_tinynerf(..., model, 10)`: nf_flex_mlp_fwd and, with
    gradients enabled, nf_flex_mlp_fwd_train / nf_flex_mlp_bwd); other geometries construct and load but have no kernel and raise."""

    def __init__(self, num_layers=4, hidden_size=128, skip_connect_every=4, num_encoding_fn_xyz=6, num_encoding_fn_dir=4,
                 include_input_xyz=True, include_input_dir=True, use_viewdirs=True):
        super().__init__()
        include_input_xyz = 3 if include_input_xyz else 0
        include_input_dir = 3 if include_input_dir else 0
        self.dim_xyz = include_input_xyz + 2 * 3 * num_encoding_fn_xyz
        self.dim_dir = include_input_dir + 2 * 3 * num_encoding_fn_dir
        self.skip_connect_every = skip_connect_every
        if not use_viewdirs:
            self.dim_dir = 0
        self.layer1 = torch.nn.Linear(self.dim_xyz, hidden_size)
        self.layers_xyz = torch.nn.ModuleList()
        for i in range(num_layers - 1):
            skip = i % self.skip_connect_every == 0 and i > 0 and i != num_layers - 1                                  # M:373
            self.layers_xyz.append(torch.nn.Linear(self.dim_xyz + hidden_size if skip else hidden_size, hidden_size))
        self.use_viewdirs = use_viewdirs
        if self.use_viewdirs:
            self.layers_dir = torch.nn.ModuleList()
            self.layers_dir.append(torch.nn.Linear(self.dim_dir + hidden_size, hidden_size // 2))
            self.fc_alpha = torch.nn.Linear(hidden_size, 1)
            self.fc_rgb = torch.nn.Linear(hidden_size // 2, 3)
            self.fc_feat = torch.nn.Linear(hidden_size, hidden_size)
        else:
            self.fc_out = torch.nn.Linear(hidden_size, 4)
        self.relu = torch.nn.functional.relu

    @property
    def num_layers(self) -> int:
        return len(self.layers_xyz) + 1

    def fused_supported(self) -> bool:
        return (not self.use_viewdirs and self.dim_xyz == 63 and self.layer1.out_features == 128 and 2 <= self.num_layers <= 5
                and all(l.in_features == 128 for l in self.layers_xyz))

    def hip_param_list(self):
        """state_dict order: layer1, layers_xyz.0 .. , fc_out (weight, bias each) -- the order of nf_flex_pack / nf_flex_mlp_bwd."""
        ps = [self.layer1.weight, self.layer1.bias]
        for l in self.layers_xyz:
            ps += [l.weight, l.bias]
        return ps + [self.fc_out.weight, self.fc_out.bias]

    def forward(self, x):
        raise NotImplementedError("FlexibleNeRFModel is evaluated inside the fused tiny-path kernel: call "
                                  "tiny_nerf.run_one_iter_of_tinynerf(..., model, 10)")
