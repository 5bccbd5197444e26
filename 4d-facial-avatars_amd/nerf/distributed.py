"""Multi-GPU sharding of the NeRFace hot path (one process per GPU, torch.distributed; backend "nccl" is RCCL
over xGMI on ROCm, "gloo" in CPU tests).  The reference is single-process / single-device; what
is added here is exactly what the path needs:

* eval  -- frames are independent: rank r renders frames r, r+W, r+2W, ... ; no data-path collective.
* train -- data parallel over frames: every rank draws its own frame and rays, then ONE all-reduce per step over a
           single flat fp32 buffer [coarse grads | fine grads | latent-table grads] (~4.5 MB + 128 B x N_train),
           averaged, followed by the identical Adam step on every rank.  At this size the collective is latency
           bound on a fully connected xGMI node (tens of microseconds against milliseconds of compute), so it is
           issued once, un-bucketed, after backward; there is nothing to overlap.
"""
from __future__ import annotations

import os
from typing import Iterable, List, Optional, Sequence

import torch
import torch.distributed as dist


def force_collectives_requested() -> bool:
    """NERFACE_DIST_FORCE=1: exercise the N > 1 path at world size 1 (see launch.common.init_distributed)."""
    return os.environ.get("NERFACE_DIST_FORCE", "0") not in ("", "0")


def _skip_collectives(world: int) -> bool:
    """At world size 1 a collective is the identity and is skipped -- unless a process group exists and the run asked for
    them (then RCCL really runs: a 1-rank all-reduce / broadcast on device memory)."""
    return world == 1 and not (force_collectives_requested() and dist.is_available() and dist.is_initialized())


def world_info():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def shard_frames(n_frames: int, rank: Optional[int] = None, world: Optional[int] = None) -> List[int]:
    """Frame indices rendered by `rank`: i = rank (mod world) -- interleaved so that every rank sees the same mix of
    head poses / expressions along a sequence and finishes at the same time."""
    r, w = world_info()
    rank = r if rank is None else rank
    world = w if world is None else world
    return list(range(rank, n_frames, world))


def gather_frame_order(n_frames: int, world: int) -> List[tuple]:
    """(rank, local index) that produced global frame i -- for writing the sequence back in order."""
    return [(i % world, i // world) for i in range(n_frames)]


def gather_rows(rows: Sequence[tuple], group=None) -> List[tuple]:
    """Host rows (tuples that start with the global frame index) of every rank, on every rank, sorted by frame: what the eval
    launcher needs to write one per-sequence table from frames that were rendered rank r, r + W, ...  The identity at world size 1."""
    _, world = world_info()
    if _skip_collectives(world):
        return sorted(rows)
    parts = [None] * dist.get_world_size(group)
    dist.all_gather_object(parts, list(rows), group=group)
    return sorted(r for part in parts for r in part)


class GradientAllReducer:
    """Flat-buffer gradient averaging for [model_coarse, model_fine, latent table]: per step ONE multi-tensor copy into a
    persistent flat buffer, ONE all-reduce, one scale, one multi-tensor copy back -- no per-parameter kernels and no
    host/device synchronisation.

    Which parameters carry a gradient is a static property of the path (only `layers_dir.3`, Quirk Q3, never does): the
    pattern is taken from `p.grad is None` on the host at the first step and agreed on once across ranks (union); later
    steps assert it still holds.  Parameters without a gradient anywhere keep grad=None; a parameter of the union whose
    local gradient is None contributes zeros.  The fused backward returns a model's gradients as views of one flat tensor
    (ops.paper_mlp_bwd), so neighbouring views are coalesced into single runs: the copies move a handful of large spans
    (coarse | fine | latent table), not 50 small tensors."""

    def __init__(self, params: Sequence[torch.Tensor], group=None):
        self.params = list(params)
        self.group = group
        self.sizes = [p.numel() for p in self.params]
        self.mask = None               # agreed has-gradient pattern (list of bool), fixed after the first reduce()
        self._buf = None
        self._views = None
        self._timing = None            # enable_timing(): (start, end) event pairs / host seconds of the flat all-reduce
        self.calls = 0

    # ---- evidence for the N > 1 path (bench.py --gpus N, launch/train_sharded.py): how many ranks the communicator saw, how many
    # bytes one step moves, what the collective cost.  Off by default: no events, no host work.
    def enable_timing(self, keep: int = 512) -> None:
        self._timing = {"keep": int(keep), "pairs": [], "host_s": []}

    def stats(self) -> dict:
        """{"ranks_seen", "bytes_allreduced", "allreduce_us" (median over the recorded steps, first step excluded), "calls"}.
        Synchronises the device (reads the events): call it outside the timed region."""
        import statistics
        _, world = world_info()
        ranks = dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1
        us = []
        if self._timing is not None:
            if self._timing["pairs"]:
                torch.cuda.synchronize()
                us = [1e3 * a.elapsed_time(b) for a, b in self._timing["pairs"]]
            else:
                us = [1e6 * t for t in self._timing["host_s"]]
        us = us[1:] if len(us) > 1 else us                                  # the first call negotiates / warms the communicator
        return {"ranks_seen": int(ranks), "world_size": int(world), "calls": int(self.calls),
                "bytes_allreduced": int(self._buf.numel() * self._buf.element_size()) if self._buf is not None else 0,
                "allreduce_us": float(statistics.median(us)) if us else None, "allreduce_samples": len(us),
                "backend": dist.get_backend(self.group) if dist.is_available() and dist.is_initialized() else None}

    def reset(self) -> None:
        """Forget the agreed gradient pattern (after (un)freezing parameters).  Collective: call on every rank."""
        self.mask, self._buf, self._views = None, None, None

    def _negotiate(self, device) -> None:
        local = [p.grad is not None for p in self.params]
        flags = torch.tensor([1.0 if f else 0.0 for f in local], dtype=torch.float32, device=device)
        dist.all_reduce(flags, op=dist.ReduceOp.SUM, group=self.group)
        self.mask = [v > 0 for v in flags.tolist()]                       # the only host sync, once per run
        total = sum(n for n, m in zip(self.sizes, self.mask) if m)
        self._buf = torch.zeros(total, dtype=torch.float32, device=device)
        self._views, off = [], 0
        for p, n, m in zip(self.params, self.sizes, self.mask):
            self._views.append(self._buf[off:off + n].view_as(p) if m else None)
            off += n if m else 0

    @staticmethod
    def _runs(grads, views):
        """Coalesce (gradient, buffer view) pairs whose gradients are adjacent views of one storage into flat spans."""
        out_g, out_v = [], []
        i, n = 0, len(grads)
        while i < n:
            g, v = grads[i], views[i]
            j, span = i + 1, g.numel()
            if g.is_contiguous():
                base, esz = g.untyped_storage().data_ptr(), g.element_size()
                while (j < n and grads[j].is_contiguous() and grads[j].untyped_storage().data_ptr() == base
                       and grads[j].storage_offset() == g.storage_offset() + span):
                    span += grads[j].numel()
                    j += 1
            if j - i > 1:
                out_g.append(torch.as_strided(g, (span,), (1,)))
                out_v.append(torch.as_strided(v, (span,), (1,)))
            else:
                out_g.append(g)
                out_v.append(v)
            i = j
        return out_g, out_v

    def reduce(self) -> None:
        _, world = world_info()
        if _skip_collectives(world):
            return
        device = self.params[0].device
        if self.mask is None:
            self._negotiate(device)
        grads, views = [], []
        for p, v, m in zip(self.params, self._views, self.mask):
            if not m:
                if p.grad is not None:
                    raise RuntimeError("GradientAllReducer: a parameter gained a gradient after the first step; call reset() on every rank")
                continue
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            grads.append(p.grad)
            views.append(v)
        with torch.no_grad():
            run_g, run_v = self._runs(grads, views)
            torch._foreach_copy_(run_v, run_g)
            tm = self._timing
            if tm is None:
                dist.all_reduce(self._buf, op=dist.ReduceOp.SUM, group=self.group)
            elif self._buf.is_cuda:                                       # HIP events on the launch stream around the collective
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dist.all_reduce(self._buf, op=dist.ReduceOp.SUM, group=self.group)
                e1.record()
                tm["pairs"].append((e0, e1))
                del tm["pairs"][:-tm["keep"]]
            else:
                import time
                t0 = time.perf_counter()
                dist.all_reduce(self._buf, op=dist.ReduceOp.SUM, group=self.group)
                tm["host_s"].append(time.perf_counter() - t0)
                del tm["host_s"][:-tm["keep"]]
            self.calls += 1
            self._buf.mul_(1.0 / world)
            torch._foreach_copy_(run_g, run_v)


def broadcast_parameters(params: Sequence[torch.Tensor], src: int = 0, group=None) -> None:
    """Identical initial state on every rank (model weights, latent table).  c10d collectives write into the storage
    without touching the autograd version counter, and the packed-weight caches (ops.MLPWeights) are keyed on
    (data_ptr, version): so the counters are bumped explicitly afterwards (one multi-tensor `x *= 1`), which invalidates
    every cached weight image that was packed before the broadcast."""
    _, world = world_info()
    if _skip_collectives(world):
        return
    with torch.no_grad():
        for p in params:
            dist.broadcast(p.detach(), src=src, group=group)
        torch._foreach_mul_([p.detach() for p in params], 1.0)


def rank_seed(base_seed: int) -> int:
    """Per-rank seed for frame / ray selection (identical model init comes from broadcast_parameters)."""
    rank, _ = world_info()
    return int(base_seed) + rank
