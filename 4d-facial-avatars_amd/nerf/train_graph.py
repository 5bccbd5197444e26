"""`nerf.GraphedTrainer` -- one NeRFace training iteration (the loop body of launch/train_sharded.py, i.e. TR:289-400) captured ONCE
in a HIP graph and replayed.

An iteration is ~74 dispatches, most of them 5-10 us fills, copies, packs and probes, driven by a Python loop body that re-packs
weight images, builds ctypes pointer tables, steps the optimizer and rewrites `lr` on the host.  The graph removes the host from the
loop: ray choice, ray batch, the weight packs, both MLP passes with their integrators, the fused loss, the backward, the Adam step
(nf_adam_step_dev: step count and learning-rate schedule on the device) and the gradient zeroing are recorded on ONE stream -- a
linear graph without parallel branches -- and replayed per step.  Not in the reference (an MI355X extension).

What differs from the eager loop body, and only where a captured graph demands it:
  * pose, expression, target image, importance map and the ROW of the latent-code table are copied into static device buffers before
    each replay; the row is a device int64 scalar, so the gather of the code and the scatter-add of its gradient into the (N, 32)
    table happen inside the graph;
  * every random draw (ray choice, stratified jitter, density noise, inverse-CDF u) comes from torch's graph-safe device generator:
    the same seed gives the same numbers as the eager loop;
  * the optimizer must be nerf.optim.Adam(..., capturable=True); gradients are dropped after the step as in the eager loop, and the
    buffers the captured backward assigns live in the graph's private memory pool (`p.grad` is None between steps);
  * the split-fp16 range probe runs once before the capture and never inside it; check_range() polls the kernels' sticky flag;
  * `parts` (the loss terms) stays on the device; read it when you log.
The one iteration that allocates the weight images, Adam moments and the library's one-time tables before the capture (workspaces,
saved activations and gradients of the replays come from the graph's private pool, fixed at capture) is run on a side stream
and then UNDONE (parameters, latent codes, background, Adam state and the generator are restored), so that step n of a graphed run
computes what step n of the eager loop computes.

Single rank only: an RCCL collective inside a captured graph is not supported, and a process group of more than one rank raises.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops
from . import optim as _optim
from .nerf_helpers import choose_rays, get_embedding_function, get_ray_batch
from .train_utils import run_one_iter_of_nerf

_PRECISIONS = ("f32", "f16x3", "bf16x3")


class GraphedTrainer:
    def __init__(self, model_coarse, model_fine, latent_codes: torch.Tensor, background: Optional[torch.Tensor], optimizer,
                 height: int, width: int, intrinsics, cfg, precision: str = "f32", supervised_background: bool = False):
        """latent_codes: the (N, 32) table the optimizer steps; background: the (H, W, 3) prior or None (a leaf that requires grad
        is trained through the optimizer's group that holds it); cfg: the config node (nerf.train.*, dataset.near / far);
        supervised_background: add the term of TR:376-381 inside the fused loss (needs a background that requires grad)."""
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise NotImplementedError("nerf.GraphedTrainer is single-rank: a gradient all-reduce cannot be recorded in the captured "
                                      f"graph (world size {torch.distributed.get_world_size()}); train without --graph")
        if precision not in _PRECISIONS:
            raise ValueError(f"precision must be one of {_PRECISIONS}")
        if not isinstance(optimizer, _optim.Adam) or not optimizer.capturable:
            raise TypeError("nerf.GraphedTrainer needs nerf.optim.Adam(..., capturable=True): its step count and learning rate live on "
                            "the device")
        if latent_codes.dim() != 2 or latent_codes.shape[1] != 32:
            raise ValueError("latent_codes must be the (N, 32) table")
        if supervised_background and (background is None or not background.requires_grad):
            raise ValueError("supervised_background needs a background that requires grad (the trainer's train_background)")
        if not latent_codes.is_cuda:
            raise RuntimeError("nerf (MI355X build): the latent-code table must be on a ROCm device; there is no CPU path")
        self.model_coarse, self.model_fine = model_coarse, model_fine
        self.latent_codes, self.background, self.optimizer = latent_codes, background, optimizer
        self.h, self.w, self.intrinsics, self.cfg = int(height), int(width), intrinsics, cfg
        self.precision, self.supervised = precision, bool(supervised_background)
        self.n_rays = int(cfg.nerf.train.num_random_rays)
        self.has_fine = model_fine is not None and int(cfg.nerf.train.num_fine) > 0
        self.enc_xyz = get_embedding_function(num_encoding_functions=10, include_input=True, log_sampling=True)
        self.enc_dir = get_embedding_function(num_encoding_functions=4, include_input=False, log_sampling=True)
        dev = latent_codes.device
        self.device = dev
        self.row = torch.zeros((), dtype=torch.int64, device=dev)
        self.parts = torch.zeros(8, dtype=torch.float32, device=dev)      # [loss, coarse, fine, code, coarse + fine, psnr, ||latent||, bg]
        self.pose = self.expr = self.target_img = self.imap = None        # static inputs, shaped by the first step
        self.selected = None                                              # (n_rays,) int64: the pixels the last step drew
        self.graph = None

    # ------------------------------------------------------------------------------------------------------------ the step
    def _iteration(self):
        """The loop body of launch/train_sharded.py on the static buffers."""
        latent = self.latent_codes.index_select(0, self.row.view(1)).view(32)
        sel = choose_rays(self.imap, self.n_rays)
        self.selected = sel                # kept alive, so its block of the graph's pool is never reused: the last replay's pixels
        ro, rd, target, bg = get_ray_batch(self.h, self.w, self.intrinsics, self.pose, sel, self.target_img, self.background)
        rgb_c, _, _, rgb_f, _, _, w_last = run_one_iter_of_nerf(
            self.h, self.w, self.intrinsics, self.model_coarse, self.model_fine, ro, rd, self.cfg, mode="train",
            encode_position_fn=self.enc_xyz, encode_direction_fn=self.enc_dir, expressions=self.expr, background_prior=bg,
            latent_code=latent)
        term = dict(background=bg[..., :3], last_weight=w_last) if self.supervised else {}
        loss, parts = ops.training_loss(rgb_c[..., :3], rgb_f[..., :3] if rgb_f is not None else None, target[..., :3], latent, **term)
        loss.backward()
        self.optimizer.step()
        # as the eager loop: the next backward ASSIGNS its gradients (no fill and no accumulate kernel per tensor); under capture the
        # buffers return to the graph's private pool, whose addresses every replay reuses
        self.optimizer.zero_grad(set_to_none=True)
        self.parts[:parts.numel()].copy_(parts)

    def _stepped(self):
        """Every tensor a step writes: (tensor, its Adam moments or None)."""
        out = []
        for group in self.optimizer.param_groups:
            for p in group["params"]:
                st = self.optimizer.state.get(p) or {}
                out.append((p, st.get("exp_avg"), st.get("exp_avg_sq")))
        return out

    def _capture(self):
        dev = self.device
        prev = ops.get_mlp_precision()
        ops.set_mlp_precision(self.precision)
        try:
            for m in (self.model_coarse, self.model_fine):
                if m is not None:
                    m.__dict__["_f16_train_calls"] = 0                    # the pre-flight range probe (split-fp16) runs in the pass below
            # ---- one iteration outside any capture: allocates Adam moments, weight images and the library's one-time tables -- and
            # is then undone
            with torch.no_grad():
                before = [(p, p.detach().clone(), None if m is None else m.clone(), None if v is None else v.clone())
                          for p, m, v in self._stepped()]
                blocks = {gi: b.clone() for gi, b in self.optimizer._blocks.items()}
            rng = torch.cuda.get_rng_state(dev)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                self.optimizer.zero_grad(set_to_none=True)
                self._iteration()
            torch.cuda.current_stream(dev).wait_stream(side)
            with torch.no_grad():
                for p, p0, m0, v0 in before:
                    p.copy_(p0)
                    st = self.optimizer.state.get(p) or {}
                    for name, old in (("exp_avg", m0), ("exp_avg_sq", v0)):
                        if name in st:
                            st[name].zero_() if old is None else st[name].copy_(old)
                for gi, b in self.optimizer._blocks.items():
                    b[:2].copy_(blocks[gi][:2]) if gi in blocks else b[:2].zero_()
            torch.cuda.set_rng_state(rng, dev)
            # ---- the capture: one stream, a linear graph
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph):
                    self._iteration()
            except RuntimeError as e:
                # the runtime's refusal of an operation a capture cannot record; anything else (a shape error, a kernel wrapper's
                # NF_EINVAL, the optimizer's own refusals) propagates as it is
                if "captur" not in str(e).lower():
                    raise
                raise RuntimeError("nerf.GraphedTrainer: the training step could not be captured -- something in it reads the device "
                                   f"or synchronises with the host, which a graph cannot record ({type(e).__name__}: {e})") from e
            self.graph = graph
        finally:
            ops.set_mlp_precision(prev)

    def _stage(self, name: str, value: torch.Tensor, dtype=torch.float32):
        buf = getattr(self, name)
        if buf is None:
            if self.graph is not None:
                raise RuntimeError("nerf.GraphedTrainer: internal error, static buffer missing after capture")
            buf = torch.empty(tuple(value.shape), dtype=dtype, device=self.device)
            setattr(self, name, buf)
        if tuple(value.shape) != tuple(buf.shape):
            raise ValueError(f"nerf.GraphedTrainer.step: {name} has shape {tuple(value.shape)}, the captured graph was built for "
                             f"{tuple(buf.shape)}")
        buf.copy_(value, non_blocking=True)

    def step(self, pose, expression, target_img, importance_map, latent_row):
        """One iteration on a frame: pose (3|4, 4), expression (76), target image (H, W, C), importance map (H * W, row-major
        selection weights) and latent_row = the frame's row of the latent-code table (an int64 scalar, on the device for a step
        without a host-to-device copy).  Returns the loss: a device scalar that the NEXT call overwrites (as all of `parts`)."""
        self._stage("pose", pose)
        self._stage("expr", expression.reshape(-1))
        self._stage("target_img", target_img)
        self._stage("imap", importance_map.reshape(-1))
        self.row.copy_(latent_row if torch.is_tensor(latent_row) else torch.tensor(int(latent_row)), non_blocking=True)
        if self.graph is None:
            self._capture()
        self.graph.replay()
        for p, _, _ in self._stepped():                                   # the graph wrote through raw pointers (see nerf.optim.Adam.step)
            torch.autograd.graph.increment_version(p)
        return self.parts[0]

    def check_range(self) -> None:
        """Raise if a split-fp16 kernel of any replay since the last poll flagged a non-finite output (one host read-back; the
        launcher calls it on the iterations that log or save).  A no-op for the other arithmetics."""
        if self.precision == "f16x3":
            ops.check_f16_range(self.model_coarse, self.model_fine)
