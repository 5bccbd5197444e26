"""`nerf.optim.Adam` -- the trainer's optimizer step as ONE kernel launch (nf_adam_step, csrc/nf_optim.hip).

The reference steps torch.optim.Adam over [coarse model, fine model, latent codes] (train_transformed_rays.py:193-199, 391-392).
torch's multi-tensor paths spend ~110 us per step on the 54 tensors of that list (two multi_tensor_apply kernels, one of them only to
increment 54 step counters); this class runs torch's update rule for every tensor of a parameter group in one launch (~8 us).

Drop-in for torch.optim.Adam where the trainer uses it: same constructor arguments, same `param_groups`, and the SAME state layout
(`state[p] = {"step": 0-d float32 CPU tensor, "exp_avg", "exp_avg_sq"}`), so `state_dict()` / `load_state_dict()` round-trip with
torch.optim.Adam and with the reference's checkpoints.  Supported: fp32 parameters on a ROCm device, weight_decay = 0, amsgrad =
False, maximize = False -- what the reference uses; anything else raises (no fallback).

`Adam(..., capturable=True)` is the form a captured HIP graph can replay (nerf.GraphedTrainer): the step count and the trainer's
learning-rate schedule live in one small DEVICE block per parameter group (nf_adam_step_dev), `state[p]["step"]` is a 0-d float32
view onto it, and step() neither reads the device nor passes a host scalar that changes between steps.  `state_dict()` still
writes torch's default layout (0-d float32 CPU steps; `lr` = the rate the schedule has reached), `load_state_dict()` accepts
every layout `__setstate__` normalises, so checkpoints move freely between this form, the default one and torch.optim.Adam.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _hip as H


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 capturable=False, **unused):
        if weight_decay != 0 or amsgrad or maximize:
            raise NotImplementedError("nerf.optim.Adam implements the trainer's configuration: weight_decay=0, amsgrad=False, maximize=False")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("invalid Adam hyper-parameters")
        # not a param-group key: the groups (and so state_dict()) keep the default layout in both forms
        self._capturable = bool(capturable)
        self._blocks = {}               # capturable: group index -> device block of nf_adam_step_dev (8 x float32, see _block)
        self._schedule = None           # capturable: (lr0, decay_factor, decay_steps) of set_lr_schedule
        self._plans = {}                # capturable: group index -> the pointer tables of the last launch
        self._written_lr = {}           # capturable: group index -> the schedule its block holds
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False))

    @property
    def capturable(self) -> bool:
        return self._capturable

    def __setstate__(self, state):
        """torch.optim.Adam.__setstate__'s normalisation: checkpoints written by the reference's torch versions (<= 1.11) hold
        `step` as a Python int, fused / capturable ones as a device tensor; here it is always a 0-d float32 CPU tensor -- or, with
        capturable=True, a view onto the group's device block, which receives the loaded count."""
        super().__setstate__(state)
        if self.__dict__.get("_capturable", False):
            self._adopt_steps()
            return
        for st in self.state.values():
            if "step" in st:
                s_ = st["step"]
                st["step"] = torch.tensor(float(s_.item() if torch.is_tensor(s_) else s_), dtype=torch.float32)

    # ------------------------------------------------------------------------------------------------ capturable=True
    def _block(self, gi: int, device) -> torch.Tensor:
        """The group's state block (include/nerface_hip.h, nf_adam_step_dev): float32[0] = step, [1] = ticket, [2:8] viewed as
        three doubles = lr0, decay_factor, decay_steps."""
        blk = self._blocks.get(gi)
        if blk is None or blk.device != torch.device(device):
            old = blk
            blk = torch.zeros(8, dtype=torch.float32, device=device)
            if old is not None:
                blk.copy_(old)
            self._blocks[gi] = blk
            self._written_lr.pop(gi, None)
        return blk

    def _write_schedule(self, gi: int, blk: torch.Tensor, lr0: float, factor: float, steps: float) -> None:
        if self._written_lr.get(gi) == (lr0, factor, steps):
            return
        if blk.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("nerf.optim.Adam(capturable=True): the learning rate changed on the host inside a graph capture; "
                               "a captured step follows set_lr_schedule(...) on the device and leaves param_groups[...]['lr'] alone")
        blk[2:8].view(torch.float64).copy_(torch.tensor([lr0, factor, steps], dtype=torch.float64))
        self._written_lr[gi] = (lr0, factor, steps)

    def set_lr_schedule(self, lr0: float, decay_factor: float, decay_steps: float) -> None:
        """The trainer's schedule (TR:395-400), evaluated by the kernel from its own step count: step i runs with
        lr0 * decay_factor ** ((i - 1) / decay_steps), step 0 with lr0 -- what a loop that rewrites `lr` after each step feeds
        its optimizer.  ONE schedule serves every param group, as the trainer's loop writes one lr_new into all of them: from here
        on param_groups[...]['lr'] (a per-group rate included) is not read by step(), and state_dict() reports the rate the
        schedule has reached in every group -- also in a group that never stepped -- as that loop leaves it."""
        if not self._capturable:
            raise RuntimeError("set_lr_schedule needs nerf.optim.Adam(..., capturable=True)")
        if not (lr0 >= 0.0 and decay_factor > 0.0 and decay_steps > 0.0):
            raise ValueError("invalid learning-rate schedule")
        self._schedule = (float(lr0), float(decay_factor), float(decay_steps))

    def scheduled_lr(self, steps_done: float, group_lr: float) -> float:
        """The rate step number `steps_done` (0-based) runs with: the host-side restatement of the kernel's expression."""
        if self._schedule is None:
            return float(group_lr)
        lr0, factor, steps = self._schedule
        return lr0 if steps_done <= 0 else lr0 * factor ** ((steps_done - 1.0) / steps)

    def _adopt_steps(self) -> None:
        """Point every state[p]['step'] at its group's block; a loaded count (int, CPU or device tensor) moves into the block."""
        for gi, group in enumerate(self.param_groups):
            loaded = set()
            for p in group["params"]:
                st = self.state.get(p)
                if not st or "step" not in st:
                    continue
                s_ = st["step"]
                blk = self._blocks.get(gi)
                if blk is not None and torch.is_tensor(s_) and s_.data_ptr() == blk.data_ptr():
                    continue
                loaded.add(float(s_.item() if torch.is_tensor(s_) else s_))
            if len(loaded) > 1:
                raise ValueError(f"nerf.optim.Adam(capturable=True): the tensors of param group {gi} have taken different numbers of "
                                 f"steps ({sorted(loaded)}); one device counter serves a group")
            for p in group["params"]:
                st = self.state.get(p)
                if not st or "step" not in st:
                    continue
                blk = self._block(gi, p.device)
                if loaded:
                    blk[0] = loaded.pop()
                    loaded = set()
                st["step"] = blk[0]

    def state_dict(self):
        """torch.optim.Adam's default layout in both forms (capturable: a host read of one float per group)."""
        sd = super().state_dict()
        if not self._capturable:
            return sd
        sd["state"] = {k: {n: (torch.tensor(float(v.item()), dtype=torch.float32) if n == "step" else v) for n, v in st.items()}
                       for k, st in sd["state"].items()}
        sd["param_groups"] = [dict(g) for g in sd["param_groups"]]
        if self._schedule is not None:
            done = max([float(b[0].item()) for b in self._blocks.values()], default=0.0)
            for g in sd["param_groups"]:
                g["lr"] = self.scheduled_lr(done, g["lr"])
        return sd

    def _step_capturable(self, lib) -> None:
        for gi, group in enumerate(self.param_groups):
            if group.get("weight_decay", 0) != 0 or group.get("amsgrad", False) or group.get("maximize", False):
                raise NotImplementedError("nerf.optim.Adam: weight_decay / amsgrad / maximize are not part of the trainer's configuration")
            items = []
            for p in group["params"]:
                if p.grad is None or p.numel() == 0:
                    continue
                g = p.grad
                if g.is_sparse:
                    raise RuntimeError("nerf.optim.Adam does not support sparse gradients")
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                    raise RuntimeError("nerf.optim.Adam (MI355X build): parameters must be contiguous float32 tensors on a ROCm device")
                if g.dtype != torch.float32 or g.device != p.device:
                    raise RuntimeError("nerf.optim.Adam: gradients must be float32 on the parameter's device")
                items.append((p, g if g.is_contiguous() else g.contiguous()))
            if not items:
                continue
            dev = items[0][0].device
            if any(p.device != dev for p, _ in items):
                raise RuntimeError("nerf.optim.Adam(capturable=True): the tensors of a param group must live on one device")
            blk = self._block(gi, dev)
            fresh = [p for p, _ in items if len(self.state[p]) == 0]
            if fresh:
                # a tensor that joins a group whose counter already runs would get the bias corrections of the others' step count
                if len(fresh) != len(items) and (torch.cuda.is_current_stream_capturing() or float(blk[0].item()) != 0.0):
                    raise RuntimeError("nerf.optim.Adam(capturable=True): a tensor received its first gradient after its param group "
                                       "had started stepping; one device counter serves a group")
                for p in fresh:
                    st = self.state[p]
                    st["step"] = blk[0]
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            lr0, factor, steps = self._schedule if self._schedule is not None else (float(group["lr"]), 1.0, 1.0)
            self._write_schedule(gi, blk, lr0, factor, steps)
            beta1, beta2 = group["betas"]
            n = len(items)
            key = tuple((int(p.data_ptr()), int(g.data_ptr()), int(self.state[p]["exp_avg"].data_ptr()),
                         int(self.state[p]["exp_avg_sq"].data_ptr())) for p, g in items)
            plan = self._plans.get(gi)
            if plan is None or plan[0] != key:
                arr = lambda ts: (C.c_void_p * n)(*[int(t.data_ptr()) for t in ts])
                plan = (key, arr([p for p, _ in items]), arr([g for _, g in items]), arr([self.state[p]["exp_avg"] for p, _ in items]),
                        arr([self.state[p]["exp_avg_sq"] for p, _ in items]), (C.c_int64 * n)(*[int(p.numel()) for p, _ in items]))
                self._plans[gi] = plan
            with torch.cuda.device(dev):
                H.check(lib.nf_adam_step_dev(plan[1], plan[2], plan[3], plan[4], plan[5], n, float(beta1), float(beta2),
                                             float(group["eps"]), int(blk.data_ptr()), H.stream_ptr(dev)), "nf_adam_step_dev")
            for p, _ in items:
                torch.autograd.graph.increment_version(p)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = H.lib()
        if self._capturable:
            self._step_capturable(lib)
            return loss
        for group in self.param_groups:
            if group.get("weight_decay", 0) != 0 or group.get("amsgrad", False) or group.get("maximize", False):
                raise NotImplementedError("nerf.optim.Adam: weight_decay / amsgrad / maximize are not part of the trainer's configuration")
            todo = []
            for p in group["params"]:                      # validate EVERYTHING first: a refused tensor must not leave others half-stepped
                if p.grad is None or p.numel() == 0:       # (zero-element parameters: nothing to update, as in torch.optim.Adam)
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("nerf.optim.Adam does not support sparse gradients")
                g = p.grad
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                    raise RuntimeError("nerf.optim.Adam (MI355X build): parameters must be contiguous float32 tensors on a ROCm device")
                if g.dtype != torch.float32 or g.device != p.device:
                    raise RuntimeError("nerf.optim.Adam: gradients must be float32 on the parameter's device")
                todo.append((p, g if g.is_contiguous() else g.contiguous()))
            by_step = {}                                   # tensors that have taken the same number of steps go into one launch
            for p, g in todo:
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif not torch.is_tensor(st["step"]) or st["step"].is_cuda:      # int (old checkpoints) / device tensor: normalise once
                    s_ = st["step"]
                    st["step"] = torch.tensor(float(s_.item() if torch.is_tensor(s_) else s_), dtype=torch.float32)
                st["step"] += 1
                by_step.setdefault((int(st["step"].item()), p.device), []).append((p, g, st["exp_avg"], st["exp_avg_sq"]))
            beta1, beta2 = group["betas"]
            for (step, dev), items in by_step.items():
                n = len(items)
                arr = lambda k: (C.c_void_p * n)(*[int(it[k].data_ptr()) for it in items])
                numel = (C.c_int64 * n)(*[int(it[0].numel()) for it in items])
                with torch.cuda.device(dev):
                    H.check(lib.nf_adam_step(arr(0), arr(1), arr(2), arr(3), numel, n, float(group["lr"]), float(beta1), float(beta2),
                                             float(group["eps"]), step, H.stream_ptr(dev)), "nf_adam_step")
                # the kernel wrote through raw pointers: tell autograd (in-place checks, and every cache keyed on `_version`:
                # the split-fp16 range probe of nerf/models.py) that these tensors changed
                for it in items:
                    torch.autograd.graph.increment_version(it[0])
        return loss
