"""Time the density-only kernels beside the full inference kernels -- same GPU, same process, same points.  Writes
profiles/density_only.md (and prints it).

    python tools/time_density.py [--rays 262144] [--samples 64] [--repeats 9] [--frames 6] [--out profiles/density_only.md]

1. <prefix>_mlp_sigma* against <prefix>_mlp_fwd* for every family and arithmetic at the workload's coarse pass (512 x 512 rays x 64
   samples).  The full kernels compile to the same code as before the density-only kernels existed (their resource-usage remarks
   are unchanged), so the full kernel timed here is the one the render path ran before.  The two launches alternate inside one
   timed loop with device events around every launch and preallocated outputs; the figure is the median, the spread min .. max.
2. nf_volume_weights_fwd against nf_volume_render_fwd at the same shape, the same way.
3. launch/eval_sharded.py on a synthetic 512 x 512 sequence (64 + 128 samples), with and without --coarse-density-only, the two
   alternating; GPU seconds per frame from the launcher's own events.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

ALL = ("f32", "bf16x3", "f16x3", "f16x2")
CLASSES = {"paper": ("ConditionalBlendshapePaperNeRFModel", ALL), "smaller": ("ConditionalBlendshapePaperSmallerNeRFModel", ("f32",)),
           "lcode": ("ConditionalBlendshapeLearnableCodeNeRFModel", ALL), "bshape": ("ConditionalBlendshapeNeRFModel", ALL),
           "cbshape": ("ConditionalCompressedBlendshapeNeRFModel", ALL)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=512 * 512)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=6, help="test frames of the synthetic sequence (0: skip the launcher part)")
    ap.add_argument("--eval-rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_only.md"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_density.py measures on a ROCm device; none is visible")
    import nerf
    from nerf import _hip as H
    from nerf import ops
    dev = torch.device("cuda:0")
    kw = dict(num_encoding_fn_xyz=10, num_encoding_fn_dir=4, include_input_xyz=True, include_input_dir=False, use_viewdirs=True,
              num_layers=4, hidden_size=256, include_expression=True)
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    expr = (torch.randn(76, generator=g) * 0.5).to(dev)
    latent = (torch.randn(32, generator=g) * 0.1).to(dev)
    near, far = 0.2, 0.8
    R, S = a.rays, a.samples
    ro = (torch.randn((R, 3), generator=g) * 0.05 + torch.tensor([0.0, 0.0, 0.5])).to(dev)
    rd = torch.nn.functional.normalize(torch.randn((R, 3), generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0]), dim=-1).to(dev)
    z = torch.sort(torch.rand((R, S), generator=g) * (far - near) + near, dim=-1)[0].to(dev)
    raw = torch.empty((R, S, 4), dtype=torch.float32, device=dev)
    sigma = torch.empty((R, S), dtype=torch.float32, device=dev)
    stream = H.stream_ptr(dev)

    def timed(fns):
        """fns: name -> callable that enqueues one launch.  Alternates them; returns name -> list of milliseconds (device events)."""
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

    def verdict(full, lean):
        """`wired`: the lean launch beats the full one by more than the full one's own run-to-run spread."""
        gain = statistics.median(full) - statistics.median(lean)
        return gain, max(full) - min(full), gain > max(full) - min(full)

    lines = ["# Density-only forward: measured", "",
             f"Command: `python tools/time_density.py --rays {R} --samples {S} --repeats {a.repeats} --warmup {a.warmup} --frames {a.frames}`", ""]
    props = torch.cuda.get_device_properties(dev)
    lines += [f"Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}.  One process; the two launches of a row "
              f"alternate in one loop; device events around every launch; median of {a.repeats} after {a.warmup} warm-up rounds (min .. max in "
              "brackets).  `gain` = full - sigma medians; `spread` = max - min of the full kernel; a variant is worth wiring only if gain > spread.", "",
              f"## MLP: sigma-only kernel against the full inference kernel, {R} rays x {S} samples", "",
              "| family | arithmetic | full, ms | sigma only, ms | sigma / full | gain, ms | spread of full, ms | gain > spread |", "|---|---|---|---|---|---|---|---|"]
    for kind, (cls, precisions) in CLASSES.items():
        m = getattr(nerf.models, cls)(**{k: v for k, v in kw.items()}).to(dev)
        fam, hw = m.FAMILY, m.hip_weights()
        cond = ops.mlp_condition(fam, hw.get(), expr, latent, near, far)
        for prec in precisions:
            image = {"f32": hw.get, "bf16x3": hw.get_bf16, "f16x3": hw.get_f16, "f16x2": hw.get_f16}[prec]()
            args = (H.ptr(image), H.ptr(cond), H.ptr(ro), H.ptr(rd), 0, H.ptr(z), R, S)
            full_fn, sig_fn = fam.fn(ops._FWD_ENTRY[prec]), fam.fn(ops._SIGMA_ENTRY[prec])
            ms = timed({"full": lambda: H.check(full_fn(*args, H.ptr(raw), stream), "full"),
                        "sigma": lambda: H.check(sig_fn(*args, H.ptr(sigma), stream), "sigma")})
            same = torch.equal(sigma, raw[..., 3])
            gain, spread, ok = verdict(ms["full"], ms["sigma"])
            lines.append(f"| {kind} | {prec} | {cell(ms['full'])} | {cell(ms['sigma'])} | {statistics.median(ms['sigma']) / statistics.median(ms['full']):.3f} "
                         f"| {gain:.3f} | {spread:.3f} | {'yes' if ok else 'NO'}{'' if same else ' (OUTPUTS DIFFER)'} |")
        del m, hw, cond

    noise = torch.randn((R, S), generator=torch.Generator(device=dev).manual_seed(2), device=dev)
    bg = torch.rand((R, 3), generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    rgb, disp, acc, w = (torch.empty(s, dtype=torch.float32, device=dev) for s in ((R, 3), (R,), (R,), (R, S)))
    disp2, acc2, w2 = torch.empty_like(disp), torch.empty_like(acc), torch.empty_like(w)
    sigma.copy_(raw[..., 3])
    L = H.lib()
    ms = timed({"full": lambda: H.check(L.nf_volume_render_fwd(H.ptr(raw), H.ptr(z), H.ptr(rd), H.ptr(noise), H.ptr(bg), R, S, 0, H.ptr(rgb),
                                                               H.ptr(disp), H.ptr(acc), H.ptr(w), stream), "full"),
                "lean": lambda: H.check(L.nf_volume_weights_fwd(H.ptr(sigma), H.ptr(z), H.ptr(rd), H.ptr(noise), R, S, H.ptr(disp2), H.ptr(acc2),
                                                                H.ptr(w2), stream), "lean")})
    same = torch.equal(w, w2) and torch.equal(disp, disp2) and torch.equal(acc, acc2)
    gain, spread, ok = verdict(ms["full"], ms["lean"])
    lines += ["", f"## Integrator: k_volume_weights_fwd against k_volume_render_fwd, {R} rays x {S} samples (noise and background given)", "",
              "| full, ms | weights only, ms | lean / full | gain, ms | spread of full, ms | gain > spread |", "|---|---|---|---|---|---|",
              f"| {cell(ms['full'])} | {cell(ms['lean'])} | {statistics.median(ms['lean']) / statistics.median(ms['full']):.3f} | {gain:.3f} | {spread:.3f} | "
              f"{'yes' if ok else 'NO'}{'' if same else ' (OUTPUTS DIFFER)'} |"]
    del raw, sigma, noise, w, w2

    if a.frames > 0:
        import yaml
        import make_synthetic_dataset as MS
        from launch import common as CM
        from launch import eval_sharded
        lines += ["", f"## Whole frames: launch/eval_sharded.py, synthetic 512 x 512 sequence, 64 + 128 samples, {a.frames} frames per run, "
                      f"{a.eval_rounds} alternating runs each", "",
                  "GPU seconds per frame from the launcher's own device events (render + post-processing); the first frame of every run is dropped "
                  "(it carries the run's first-launch costs).", "",
                  "| model | arithmetic | default, ms / frame | --coarse-density-only, ms / frame | lean / default |", "|---|---|---|---|---|"]
        with tempfile.TemporaryDirectory() as base:
            MS.write(os.path.join(base, "data"), size=512, n_train=1, n_val=1, n_test=a.frames)
            for kind in ("paper", "lcode"):
                cfg = MS.config(os.path.join(base, "data"), os.path.join(base, "logs"), model_type=CLASSES[kind][0])
                cfg["nerf"]["validation"].update(num_coarse=64, num_fine=128, chunksize=65536)
                cfg_path = os.path.join(base, f"{kind}.yml")
                with open(cfg_path, "w") as f:
                    yaml.safe_dump(cfg, f)
                torch.manual_seed(7)
                mc, mf = CM.build_models(CM.load_config(cfg_path), dev)
                ck = os.path.join(base, f"{kind}.ckpt")
                torch.save({"model_coarse_state_dict": mc.state_dict(), "model_fine_state_dict": mf.state_dict()}, ck)
                for prec in CLASSES[kind][1]:
                    t = {"default": [], "lean": []}
                    try:
                        for _ in range(a.eval_rounds):
                            for name, extra in (("default", []), ("lean", ["--coarse-density-only"])):
                                with contextlib.redirect_stdout(io.StringIO()):
                                    eval_sharded.main(["--config", cfg_path, "--checkpoint", ck, "--savedir", os.path.join(base, "out"), "--precision", prec,
                                                       "--verify-gate", "0", *extra])
                                t[name] += [1e3 * s for s in eval_sharded.main.last_stats["frame_s"][1:]]
                    finally:
                        nerf.set_mlp_precision("f32")
                    lines.append(f"| {kind} | {prec} | {cell(t['default'])} | {cell(t['lean'])} | {statistics.median(t['lean']) / statistics.median(t['default']):.3f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
