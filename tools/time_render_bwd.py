"""Time the integrator's full backward (k_volume_render_bwd_full) beside the rgb-only kernel (k_volume_render_bwd) -- same GPU, same
process, same inputs.  Prints the table of profiles/render_full_bwd.md.

    python tools/time_render_bwd.py [--rays 2048] [--samples 128] [--repeats 200] [--warmup 20]

NeRFace mode with background prior and density noise.  The three calls alternate inside one timed loop (device events around every
`nerf.ops` call, so every figure includes the wrapper's output allocations); the figures are the median and the minimum.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))

import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_render_bwd.py measures on a ROCm device; none is visible")
    from nerf import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    n, s = a.rays, a.samples
    rnd = lambda *shape: torch.randn(shape, generator=g).to(dev)
    raw = rnd(n, s, 4)
    z = torch.sort(torch.rand((n, s), generator=g) * 0.6 + 0.2, dim=-1)[0].to(dev)
    rd = torch.nn.functional.normalize(torch.randn((n, 3), generator=g), dim=-1).to(dev)
    noise, bg = rnd(n, s) * 0.1, torch.rand((n, 3), generator=g).to(dev)
    d_rgb, d_disp, d_acc, d_w, d_wl = rnd(n, 3), rnd(n), rnd(n), rnd(n, s), rnd(n)
    nch = (s + 63) // 64
    tmpl = nch if nch <= 4 else (8 if nch <= 8 else 16)
    fns = {
        f"`ops.volume_render_bwd` -> `k_volume_render_bwd<{tmpl}>` (d_rgb only)":
            lambda: ops.volume_render_bwd(raw, z, rd, noise, bg, d_rgb, False),
        f"`ops.volume_render_bwd_full` -> `k_volume_render_bwd_full<{tmpl}>`, d_rgb only":
            lambda: ops.volume_render_bwd_full(raw, z, rd, noise, bg, d_rgb=d_rgb),
        "`ops.volume_render_bwd_full`, all five cotangents and d_bg":
            lambda: ops.volume_render_bwd_full(raw, z, rd, noise, bg, d_rgb, d_disp, d_acc, d_w, d_wl, False, need_d_bg=True),
    }
    for _ in range(a.warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(a.repeats):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3)
    props = torch.cuda.get_device_properties(dev)
    print(f"Command: `python tools/time_render_bwd.py --rays {n} --samples {s} --repeats {a.repeats} --warmup {a.warmup}`\n")
    print(f"Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}; {n} rays x {s} samples.\n")
    print("| call | median | min |\n|---|---|---|")
    for k, v in us.items():
        print(f"| {k} | {statistics.median(v):.1f} us | {min(v):.1f} us |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
