"""Time the gated exact-f32 forward (nf_paper_mlp_fwd_gated: fc_feat, too, only where a bound on sigma cannot prove the sample dead)
beside the live-colour kernel -- same GPU, same process, same points, in the manner of tools/time_live_colour.py.  Prints a markdown
report (profiles/sigma_gate.md keeps it).

    python tools/time_sigma_gate.py [--frames 2 3 4 5 6] [--repeats 9] [--out FILE] [--parent-lib LIB] [--phases]

The points are the benchmark's (bench_common's models, poses and validation settings; one chunk of 65536 rays per frame through a
real coarse pass, which yields the z values of the coarse launch, 65536 x 64, and of the fine launch, 65536 x 192).  At each of the
two the live and the gated launch alternate inside one timed loop with device events around every launch and preallocated outputs;
the figure is the median, the spread min .. max.  `live` is the share of points with density or last on their ray, `kept` the share
the gate could not prove dead (from the statistics instantiation, run once); the model column is the MFMA count per 32 points,
(11,392 + 4,360 kept) / (13,440 + 2,176 live), times the live kernel's median.

--parent-lib LIB: a third launch in the same loop, nf_paper_mlp_fwd_gated of another build of the library (the parent commit's), and a
column for it.  --phases: a second table from the statistics instantiations of both kernels, shader clocks per pass (a pass = one
32-point unit of one wave) by phase, beside what the phase's MFMAs alone cost at 32 clocks each.
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
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--phases", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_sigma_gate.py measures on a ROCm device; none is visible")
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
    parent_fn = None
    if a.parent_lib:                                          # its own copies of every symbol: nothing of it binds to the library loaded first
        import ctypes
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib), mode=os.RTLD_LOCAL | os.RTLD_NOW | os.RTLD_DEEPBIND)
        parent_fn = parent.nf_paper_mlp_fwd_gated
        parent_fn.restype, parent_fn.argtypes = H._PROTOTYPES["nf_paper_mlp_fwd_gated"]

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
    lines = [f"Command: `python tools/time_sigma_gate.py --frames {' '.join(map(str, a.frames))} --repeats {a.repeats} --warmup {a.warmup}`", "",
             f"Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}.  One process; the two launches of a row "
             f"alternate in one loop; device events around every launch; median of {a.repeats} after {a.warmup} warm-up rounds (min .. max in "
             "brackets).  `gain` = live - gated medians; `spread` = max - min of the live kernel.", "",
             "| frame | launch | live | kept | live kernel, ms | gated kernel, ms | gated / live | model | gain, ms | spread of live, ms | outputs |"
             + (" parent's gated kernel, ms | gated - parent's, ms | spread of parent's, ms |" if parent_fn else ""),
             "|---|---|---|---|---|---|---|---|---|---|---|" + ("---|---|---|" if parent_fn else "")]
    phase_lines = ["| frame | launch | kernel | passes | runs | trunk | lone tile | ballot + append | run entry, per run | run, per run | dead-row stores | "
                   "sum per pass |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    totals = {"coarse": ([], []), "fine": ([], [])}
    bound_ms = []
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
            bound = m.hip_weights().get_bound()
            cond = ops.mlp_condition(fam, packed, expr, latent, BC.NEAR, BC.FAR)
            raw, raw_l, raw_g = (torch.empty((R, S, 4), dtype=torch.float32, device=dev) for _ in range(3))
            H.check(fam.fn("mlp_fwd")(H.ptr(packed), H.ptr(cond), H.ptr(ro), H.ptr(rd), 0, H.ptr(z), R, S, H.ptr(raw), stream), "full")
            tail = (H.ptr(cond), H.ptr(ro), H.ptr(rd), 0, H.ptr(z), R, S)
            live_fn, gated_fn, bound_fn = fam.fn("mlp_fwd_live"), fam.fn("mlp_fwd_gated"), fam.fn("sigma_bound")
            fns = {"live": lambda: H.check(live_fn(H.ptr(packed), *tail, H.ptr(raw_l), H.ptr(scratch), scratch.numel(), 0, stream), "live"),
                   "gated": lambda: H.check(gated_fn(H.ptr(packed), H.ptr(bound), *tail, H.ptr(raw_g), H.ptr(scratch), scratch.numel(), 0,
                                                     stream), "gated"),
                   "bound": lambda: H.check(bound_fn(H.ptr(packed), H.ptr(bound), stream), "bound")}
            if parent_fn:
                raw_p = torch.empty_like(raw_g)
                fns["parent"] = lambda: H.check(parent_fn(H.ptr(packed), H.ptr(bound), *tail, H.ptr(raw_p), H.ptr(scratch), scratch.numel(), 0,
                                                          stream), "parent's gated")
            ms = timed(fns)
            bound_ms += ms["bound"]
            live = ~(raw[..., 3] <= 0)
            live[:, -1] = True
            same = (torch.equal(raw_g[live], raw[live]) and bool((raw_g[..., :3][~live].view(torch.int32) == 0).all())
                    and bool(((raw_g[..., 3] == raw[..., 3]) | (raw_g[..., 3] < 0))[~live].all()))
            for x, y in zip(ops.volume_render_fwd(raw_g, z, rd), ops.volume_render_fwd(raw, z, rd)):
                same = same and torch.equal(x, y)
            _, st = ops.mlp_fwd_gated_stats(fam, packed, bound, cond, ro, rd, z)
            fl = float(live.float().mean())
            kept = 1.0 - float(st[:, 4].sum()) / (R * S)
            ml, mg = statistics.median(ms["live"]), statistics.median(ms["gated"])
            model = (11392 + 4360 * kept) / (13440 + 2176 * fl)
            totals[name][0].append(ml)
            totals[name][1].append(mg)
            row = (f"| {f} | {name} {R} x {S} | {fl:.3f} | {kept:.3f} | {cell(ms['live'])} | {cell(ms['gated'])} | {mg / ml:.3f} | {model:.3f} = "
                   f"{model * ml:.3f} ms | {ml - mg:.3f} | {max(ms['live']) - min(ms['live']):.3f} | {'as specified' if same else 'DIFFER'} |")
            if parent_fn:
                same_p = torch.equal(raw_p.view(torch.int32), raw_g.view(torch.int32))
                row += (f" {cell(ms['parent'])} | {mg - statistics.median(ms['parent']):+.3f} | {max(ms['parent']) - min(ms['parent']):.3f}"
                        f"{'' if same_p else ' (RAW DIFFERS)'} |")
            lines.append(row)
            if a.phases:
                _, sl = ops.mlp_fwd_live_stats(fam, packed, cond, ro, rd, z)
                for kern, t, c0, mfma in (("live", sl, 4, (13312, 128, 2176)), ("gated", st, 5, (11264, 128, 4360))):
                    units, runs = int(t[:, 0].sum()), int(t[:, 1].sum())
                    ph = [int(x) for x in t[:, c0:c0 + 6].sum(dim=0)]
                    per = [ph[0] / units, ph[1] / units, ph[2] / units, ph[3] / max(runs, 1), ph[4] / max(runs, 1), ph[5] / units]
                    phase_lines.append(f"| {f} | {name} | {kern} | {units} | {runs} | {per[0]:.0f} ({32 * mfma[0]}) | {per[1]:.0f} ({32 * mfma[1]}) | "
                                       f"{per[2]:.0f} | {per[3]:.0f} | {per[4]:.0f} ({32 * mfma[2]}) | {per[5]:.0f} | {sum(ph) / units:.0f} |")
    lines += [""]
    per_frame = 0.0
    for name, (live_t, gated_t) in totals.items():
        gain = statistics.mean(live_t) - statistics.mean(gated_t)
        per_frame += 4 * gain
        lines.append(f"Mean over the frames, {name} launch: live {statistics.mean(live_t):.3f} ms, gated {statistics.mean(gated_t):.3f} ms, "
                     f"gain {gain:.3f} ms ({100 * gain / statistics.mean(live_t):.1f} %).")
    lines.append(f"Four launches of each per 512 x 512 frame: {per_frame:.2f} ms per frame expected from the launches alone.")
    lines.append(f"The bound image's kernel (two per frame): {cell(bound_ms)} ms.")
    if a.phases:
        lines += ["", "Shader clocks (s_memtime) by phase, from the statistics instantiations, mean per pass over all waves (run entry and run: per "
                  "run); in brackets the phase's MFMAs at 32 clocks each.", ""] + phase_lines
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
