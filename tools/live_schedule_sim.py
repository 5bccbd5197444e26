"""Replay the schedule of the exact-f32 live-colour kernel (k_paper_mlp_fwd_live) on the CPU, in the former static order and in the
dynamic order the kernel runs, and set both against the launch's MFMA count.

    python tools/live_schedule_sim.py [--frames 2 3 4 5 6] [--measure] [--out FILE]

The model: a wave's pass over a unit of 32 consecutive points costs PASS_COST (the trunk's MFMA count per pass, 13,440) and a colour
run or the final flush RUN_COST more (2,176); row moves are ignored.  A wave with R ring rows that takes a unit with L live points
runs the colour layers when R + L >= 32 (R becomes R + L - 32) and appends otherwise (R becomes R + L); behind its last unit it
flushes what the ring holds.
    static:  wave w of workgroup b of G takes unit 4 (k G + (b + k step) mod G) + w in pass k (ops.live_rotation_step);
    greedy:  the wave that is free first takes the next unit in point order (ties: the lowest wave number) -- the kernel's counter.
    ideal:   (units * PASS_COST + live / 32 * RUN_COST) / waves -- the MFMA count spread evenly, no flush padding.
For each the slowest wave (the launch's length in the model) and the mean over the waves are printed.

On a ROCm device the masks come from ops.mlp_fwd(...)[..., 3] > 0 on the benchmark's chunks (bench_common's models, poses and
validation settings; the chunk of a frame as tools/time_live_colour.py picks it).  --measure also runs each launch through the
kernel's statistics instantiation (ops.mlp_fwd_live_stats) and prints what the waves report: the spread of their exit clocks, and
the colour runs they counted beside the model's.  simulate() itself needs neither torch nor a device (tests/test_live_dynamic_host.py).
"""
from __future__ import annotations

import argparse
import heapq
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PASS_COST = 13440                       # MFMA-count units of a pass's trunk (through fc_feat and fc_alpha)
RUN_COST = 2176                         # ... of a colour run (layers_dir.0 .. fc_rgb on 32 rows)
ROWS, WAVES = 32, 4                     # points per unit, waves per workgroup
WALL_CLOCK_MHZ = 100.0                  # wall_clock64() counts at a constant 100 MHz on gfx950


def live_per_unit(live) -> np.ndarray:
    """Live points of every unit of 32 consecutive points (the last unit may be short)."""
    live = np.asarray(live, dtype=bool).reshape(-1)
    pad = (-live.size) % ROWS
    return np.concatenate([live, np.zeros(pad, dtype=bool)]).reshape(-1, ROWS).sum(axis=1).astype(np.int64)


def rotation_step(workgroups: int) -> int:
    """nerf.ops.live_rotation_step, restated so that the replay needs no torch."""
    step = (workgroups * 5 // 13) | 1
    return step if step < workgroups else 0


def _take(R: int, L: int):
    """(cost, ring rows afterwards, colour runs) of a pass with L live rows on a ring of R."""
    if R + L >= ROWS:
        return PASS_COST + RUN_COST, R + L - ROWS, 1
    return PASS_COST, R + L, 0


def simulate(live, workgroups: int) -> dict:
    """-> {"units", "live", "waves", "ideal", "static": {...}, "greedy": {...}}; each order: "slowest", "mean" (cost units), "runs"
    (colour runs, flushes included) and "finish" (per wave).  `workgroups` caps the grid as max_workgroups / the CU count does."""
    per_unit = live_per_unit(live)
    units = per_unit.size
    G = max(1, min(int(workgroups), (units + WAVES - 1) // WAVES))
    waves = G * WAVES
    out = {"units": units, "live": int(per_unit.sum()), "waves": waves,
           "ideal": (units * PASS_COST + per_unit.sum() / ROWS * RUN_COST) / waves}
    # static: every wave walks its own list of units
    step = rotation_step(G)
    finish, runs = np.zeros(waves), 0
    for b in range(G):
        for w in range(WAVES):
            t, R, rot, k = 0, 0, b, 0
            while True:
                u = (k * G + rot) * WAVES + w
                rot = rot + step - G if rot + step >= G else rot + step
                if u >= units:
                    break
                c, R, r = _take(R, int(per_unit[u]))
                t, runs, k = t + c, runs + r, k + 1
            if R:
                t, runs = t + RUN_COST, runs + 1
            finish[b * WAVES + w] = t
    out["static"] = {"slowest": float(finish.max()), "mean": float(finish.mean()), "runs": runs, "finish": finish}
    # greedy: the wave that is free first takes the next unit
    heap = [(0, i) for i in range(waves)]
    ring = [0] * waves
    finish, runs = np.zeros(waves), 0
    for u in range(units):
        t, i = heapq.heappop(heap)
        c, ring[i], r = _take(ring[i], int(per_unit[u]))
        runs += r
        heapq.heappush(heap, (t + c, i))
    for t, i in heap:
        if ring[i]:
            t, runs = t + RUN_COST, runs + 1
        finish[i] = t
    out["greedy"] = {"slowest": float(finish.max()), "mean": float(finish.mean()), "runs": runs, "finish": finish}
    return out


def report_line(name: str, sim: dict) -> str:
    s, g, ideal = sim["static"], sim["greedy"], sim["ideal"]
    return (f"| {name} | {sim['live'] / (sim['units'] * ROWS):.3f} | {ideal:,.0f} | {s['slowest']:,.0f} ({100 * (s['slowest'] / s['mean'] - 1):+.2f} %) | "
            f"{s['mean']:,.0f} | {g['slowest']:,.0f} ({100 * (g['slowest'] / g['mean'] - 1):+.2f} %) | {g['mean']:,.0f} | "
            f"{100 * (1 - g['slowest'] / s['slowest']):.2f} | {100 * (s['slowest'] / ideal - 1):.2f} | {100 * (g['slowest'] / ideal - 1):.2f} |")


HEADER = ["| launch | live | ideal | static: slowest wave (over its mean) | static: mean | greedy: slowest wave (over its mean) | greedy: mean | "
          "greedy under static, % | static over ideal, % | greedy over ideal, % |", "|---|---|---|---|---|---|---|---|---|---|"]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[2, 3, 4, 5, 6])
    ap.add_argument("--measure", action="store_true", help="also run the kernel's statistics instantiation on every launch")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("live_schedule_sim.py takes its masks from the full forward on a ROCm device; none is visible")
    import bench_common as BC
    import nerf
    from nerf import ops
    dev = torch.device("cuda:0")
    nerf.set_mlp_precision("f32")
    models = (BC.synth_params(0, dev), BC.synth_params(1, dev))
    fam = models[0].FAMILY
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    R = BC.CHUNK
    lines = [f"Cost model: {PASS_COST:,} per pass + {RUN_COST:,} per colour run or flush; {cus} workgroups of {WAVES} waves.", ""] + HEADER
    measured = ["| launch | waves | units (sum) | colour runs: kernel / greedy model / static model | exit clocks: max - min, us | max - mean, us | "
                "model, greedy: slowest - mean, % of launch | model, static: slowest - mean, % of launch |", "|---|---|---|---|---|---|---|---|"]
    for f in a.frames:
        g = torch.Generator().manual_seed(1000 + f)
        expr, latent = (0.5 * torch.randn(76, generator=g)).to(dev), (0.1 * torch.randn(32, generator=g)).to(dev)
        ro, rd = nerf.get_ray_bundle(BC.H, BC.W, BC.INTRINSICS, BC.frame_pose(f).to(dev))
        k = f % (BC.H * BC.W // R)
        ro, rd = (t.reshape(-1, 3)[k * R:(k + 1) * R].contiguous() for t in (ro, rd))
        torch.manual_seed(1234 + f)
        z = ops.sample_coarse(R, BC.N_COARSE, BC.NEAR, BC.FAR, dev, torch.rand((R, BC.N_COARSE), device=dev), lindisp=False)
        raw = None
        for name, m in zip(("coarse", "fine"), models):
            if name == "fine":
                w_c = ops.volume_render_fwd(raw, z, rd, None, None, False)[3]
                z = ops.resample_merge(z, w_c, BC.N_FINE, torch.rand((R, BC.N_FINE), device=dev))
            packed = m.hip_weights().get()
            cond = ops.mlp_condition(fam, packed, expr, latent, BC.NEAR, BC.FAR)
            raw = ops.mlp_fwd(fam, "f32", packed, cond, ro, rd, z)
            live = raw[..., 3] > 0
            live[:, -1] = True                                          # the last sample of a ray is live too
            sim = simulate(live.reshape(-1).cpu().numpy(), cus)
            label = f"frame {f}, rays {k * R}.., {name} {R} x {z.shape[1]}"
            lines.append(report_line(label, sim))
            if a.measure:
                _, stats = ops.mlp_fwd_live_stats(fam, packed, cond, ro, rd, z)
                torch.cuda.synchronize()
                st = stats.cpu().numpy()
                st = st[st[:, 0] > 0]
                clk = st[:, 3].astype(np.float64) / WALL_CLOCK_MHZ
                gs, ss = sim["greedy"], sim["static"]
                measured.append(f"| {label} | {st.shape[0]} | {int(st[:, 0].sum())} | {int(st[:, 1].sum())} / {gs['runs']} / {ss['runs']} | "
                                f"{clk.max() - clk.min():.1f} | {clk.max() - clk.mean():.1f} | {100 * (gs['slowest'] - gs['mean']) / gs['slowest']:.2f} | "
                                f"{100 * (ss['slowest'] - ss['mean']) / ss['slowest']:.2f} |")
    if a.measure:
        lines += ["", "What the waves of the statistics instantiation report (one launch each):", ""] + measured
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
