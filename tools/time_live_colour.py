"""Time the exact-f32 live-colour kernel (k_paper_mlp_fwd_live) beside the full inference kernel -- same GPU, same process, same
points.  Prints a markdown report (profiles/live_colour_fill.md and profiles/live_colour.md keep them, with the whole-frame figures
of bench.py beside them).  NERFACE_HIP_LIB selects another build of the library, e.g. one with -DNF_LIVE_PF=N.

    python tools/time_live_colour.py [--frames 2 3 4 5 6] [--repeats 9] [--out FILE]

The points are those of the benchmark: bench_common's models, poses, conditioning and validation settings (64 coarse + 128 fine
samples, chunks of 65536 rays, perturbed depths, no noise).  For every frame one chunk of 65536 rays goes through a real coarse
pass (full kernel, integrator, resample + merge), which yields the z values of the coarse launch (65536 x 64) and of the fine launch
(65536 x 192).  At each of the two the full and the live launch alternate inside one timed loop with device events around every
launch and preallocated outputs; the figure is the median, the spread min .. max.  The live fraction of a launch is counted from the
full kernel's sigma; the two outputs are compared as the tests compare them.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))

import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[2, 3, 4, 5, 6])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_live_colour.py measures on a ROCm device; none is visible")
    import bench_common as BC
    import nerf
    from nerf import _hip as H
    from nerf import ops
    dev = torch.device("cuda:0")
    nerf.set_mlp_precision("f32")
    models = (BC.synth_params(0, dev), BC.synth_params(1, dev))
    stream = H.stream_ptr(dev)
    R = BC.CHUNK
    fam = models[0].FAMILY
    scratch = torch.empty(fam.fn("mlp_fwd_live_scratch_floats")(0), dtype=torch.float32, device=dev)

    def timed(fns):
        for _ in range(a.warmup):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(a.repeats):
            for k, f in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return ms

    def cell(v):
        return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"

    props = torch.cuda.get_device_properties(dev)
    lines = [f"Command: `python tools/time_live_colour.py --frames {' '.join(map(str, a.frames))} --repeats {a.repeats} --warmup {a.warmup}`", "",
             f"Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}.  One process; the two launches of a row "
             f"alternate in one loop; device events around every launch; median of {a.repeats} after {a.warmup} warm-up rounds (min .. max in "
             "brackets).  `gain` = full - live medians; `spread` = max - min of the full kernel.", "",
             "| frame | launch | live fraction | full, ms | live, ms | live / full | gain, ms | spread of full, ms | outputs |",
             "|---|---|---|---|---|---|---|---|---|"]
    totals = {"coarse": ([], []), "fine": ([], [])}
    for f in a.frames:
        g = torch.Generator().manual_seed(1000 + f)
        expr, latent = (0.5 * torch.randn(76, generator=g)).to(dev), (0.1 * torch.randn(32, generator=g)).to(dev)
        ro, rd = nerf.get_ray_bundle(BC.H, BC.W, BC.INTRINSICS, BC.frame_pose(f).to(dev))
        k = f % (BC.H * BC.W // R)                                        # a different quarter of the image per frame
        ro, rd = (t.reshape(-1, 3)[k * R:(k + 1) * R].contiguous() for t in (ro, rd))
        torch.manual_seed(1234 + f)
        z_c = ops.sample_coarse(R, BC.N_COARSE, BC.NEAR, BC.FAR, dev, torch.rand((R, BC.N_COARSE), device=dev), lindisp=False)
        z = None
        for name, m in zip(("coarse", "fine"), models):
            if name == "fine":
                w_c = ops.volume_render_fwd(raw, z, rd, None, None, False)[3]
                z = ops.resample_merge(z, w_c, BC.N_FINE, torch.rand((R, BC.N_FINE), device=dev))
            else:
                z = z_c
            S = z.shape[1]
            packed = m.hip_weights().get()
            cond = ops.mlp_condition(fam, packed, expr, latent, BC.NEAR, BC.FAR)
            raw, raw_l = (torch.empty((R, S, 4), dtype=torch.float32, device=dev) for _ in range(2))
            args = (H.ptr(packed), H.ptr(cond), H.ptr(ro), H.ptr(rd), 0, H.ptr(z), R, S)
            full_fn, live_fn = fam.fn("mlp_fwd"), fam.fn("mlp_fwd_live")
            ms = timed({"full": lambda: H.check(full_fn(*args, H.ptr(raw), stream), "full"),
                        "live": lambda: H.check(live_fn(*args, H.ptr(raw_l), H.ptr(scratch), scratch.numel(), 0, stream), "live")})
            live = ~(raw[..., 3] <= 0)
            live[:, -1] = True
            same = (torch.equal(raw_l[..., 3], raw[..., 3]) and torch.equal(raw_l[..., :3][live], raw[..., :3][live])
                    and bool((raw_l[..., :3][~live].view(torch.int32) == 0).all()))
            mf, ml = statistics.median(ms["full"]), statistics.median(ms["live"])
            totals[name][0].append(mf)
            totals[name][1].append(ml)
            lines.append(f"| {f} | {name} {R} x {S} | {float(live.float().mean()):.3f} | {cell(ms['full'])} | {cell(ms['live'])} | {ml / mf:.3f} | "
                         f"{mf - ml:.3f} | {max(ms['full']) - min(ms['full']):.3f} | {'as specified' if same else 'DIFFER'} |")
    lines += [""]
    per_frame = 0.0
    for name, (full, live) in totals.items():
        gain = statistics.mean(full) - statistics.mean(live)
        per_frame += 4 * gain
        lines.append(f"Mean over the frames, {name} launch: full {statistics.mean(full):.3f} ms, live {statistics.mean(live):.3f} ms, "
                     f"gain {gain:.3f} ms ({100 * gain / statistics.mean(full):.1f} %).")
    lines.append(f"Four launches of each per 512 x 512 frame: {per_frame:.2f} ms per frame expected from the launches alone.")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
