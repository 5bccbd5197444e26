"""Host model of the schedule of k_paper_mlp_fwd_live (csrc/nf_mlp_live.hip): which wave sees which points in which pass, how many
rows its ring holds, and which branch every pass takes.  No arithmetic: the model says where a live point's colour is computed, the
GPU tests say that it is the full forward's.

A pass of a wave covers 32 consecutive points.  With L live rows among them, D = 32 - L holes and R rows in the wave's ring:
    R >= D   "fill":   the D oldest ring rows fill the holes (the first ops.LIVE_PREFETCH_ROWS of them were requested ahead and sit in
                       registers, the others are loaded behind the ballot) and the colour layers run on 32 rows;
    R <  D   "append": the L live rows go to the ring, nothing runs;
behind its last block a wave with R > 0 runs a "flush" on the R rows.  The constants come from nerf.ops, where they stand next to the
scratch sizing."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

WAVES, ROWS = 4, 32                     # waves per workgroup, points per wave pass


@dataclass
class Pass:
    wg: int
    wave: int
    k: int                              # pass number of the workgroup
    branch: str                         # "fill" | "append" | "flush"
    R: int                              # ring rows when the pass starts
    L: int                              # live rows of the pass's own block (0 for a flush)
    D: int                              # holes (32 - L); for a flush the 32 - R rows that stay padding
    taken: list = field(default_factory=list)        # point indices moved from the ring into the slab, in the order taken
    appended: list = field(default_factory=list)     # point indices appended to the ring, in ring order
    from_registers: int = 0             # of those, rows that the prefetch had requested
    loaded: int = 0                     # and rows loaded behind the ballot ("holes beyond the prefetch depth")


def live_points(sig_pos, n_points: int, S: int) -> np.ndarray:
    """The kernel's liveness rule on a mask of !(sigma_raw <= 0): the last sample of every ray is live too."""
    live = np.asarray(sig_pos, dtype=bool).reshape(-1)[:n_points].copy()
    assert live.size == n_points and n_points % S == 0
    live[S - 1::S] = True
    return live


def replay(sig_pos, n_points: int, S: int, grid: int):
    """-> (passes, coloured): every pass of every wave of a launch on `grid` workgroups at most, and how often each point's colour
    was computed.  Asserts the ring's bounds on the way."""
    from nerf import ops
    live = live_points(sig_pos, n_points, S)
    G = min(grid, (n_points + WAVES * ROWS - 1) // (WAVES * ROWS))
    step = ops.live_rotation_step(G)
    passes, coloured = [], np.zeros(n_points, dtype=np.int64)
    for b in range(G):
        for wave in range(WAVES):
            ring, rot, k = [], b, 0                      # the ring as a FIFO of point indices
            while True:
                blk = k * G + rot
                rot = rot + step - G if rot + step >= G else rot + step
                p0 = (blk * WAVES + wave) * ROWS
                R = len(ring)
                assert 0 <= R <= ROWS - 1 and R < ops.LIVE_RING_ROWS, R
                if p0 >= n_points:
                    if R:
                        n_reg = min(R, ops.LIVE_PREFETCH_ROWS)
                        passes.append(Pass(b, wave, k, "flush", R, 0, ROWS - R, taken=list(ring), from_registers=n_reg, loaded=R - n_reg))
                        coloured[ring] += 1
                    break
                own = [p for p in range(p0, min(p0 + ROWS, n_points)) if live[p]]
                L, D = len(own), ROWS - len(own)
                if R >= D:
                    taken, ring = ring[:D], ring[D:]
                    n_reg = min(D, ops.LIVE_PREFETCH_ROWS)
                    passes.append(Pass(b, wave, k, "fill", R, L, D, taken=taken, from_registers=n_reg, loaded=D - n_reg))
                    coloured[own + taken] += 1
                else:
                    ring = ring + own
                    passes.append(Pass(b, wave, k, "append", R, L, D, appended=own))
                k += 1
    return passes, coloured


def branches(passes) -> set:
    """Names of the schedule's corner cases that a list of passes hits (what the GPU tests require their cases to cover together)."""
    from nerf import ops
    hit = set()
    for p in passes:
        if p.branch == "fill":
            hit.add("fill")
            if p.R == p.D and p.D > 0:
                hit.add("fill_R_eq_D")
            if p.L == ROWS and p.R > 0:
                hit.add("all_live_R_pos")
            if p.L == ROWS and p.R == 0:
                hit.add("all_live_R_zero")
            if p.loaded > 0:                            # (a fill never has L == 0: it would need R == 32)
                hit.add("beyond_prefetch")
        elif p.branch == "append":
            hit.add("append")
            if p.R + p.L == ROWS - 1:
                hit.add("append_to_31")
            if p.L == 0 and p.R > 0:
                hit.add("L_zero_R_pos")
        else:
            hit.add("flush")
            if p.R == 1:
                hit.add("flush_1")
            if p.R >= 30:
                hit.add("flush_30")
            if p.R > ops.LIVE_PREFETCH_ROWS:
                hit.add("beyond_prefetch_flush")
    return hit


REQUIRED = {"fill_R_eq_D", "append_to_31", "all_live_R_pos", "L_zero_R_pos", "beyond_prefetch", "flush_1", "flush_30"}
