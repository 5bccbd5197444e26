"""Time the exact-f32 kernels of the smaller paper model family beside their paper-model counterparts -- same GPU, same process,
same points.  Writes profiles/smaller_family.md (and prints it).

    python tools/time_smaller.py [--rays 65536] [--samples 192] [--repeats 15] [--out profiles/smaller_family.md]

Inference forward: the benchmark's fine-pass shape (65,536 rays x 192 samples).  The two families' launches alternate inside one
timed loop (device events around every launch), so drift of the clocks or a busy host meets both alike; the figure is the median.
Training forward and the three backward stages (dX chain | weight-gradient GEMMs | reduce + scatter): a training step's fine pass,
2048 rays x 128 samples, timed the same way (the stages by the libraries' own nf_*_mlp_bwd_stage_ms hooks).
Yardstick (the issue that introduced the family): per 16 points the forward issues 6788 MFMAs against the paper kernel's 7812,
ratio 0.869; the inference forward should take at most 0.869 x 1.05 of the paper kernel's time.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))

import torch  # noqa: E402

MFMA = {"paper": 7812, "smaller": 6788}            # v_mfma_f32_16x16x4_f32 per 16 points, forward


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=192)
    ap.add_argument("--train-rays", type=int, default=2048)
    ap.add_argument("--train-samples", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smaller_family.md"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_smaller.py measures on a ROCm device; none is visible")
    import nerf
    from nerf import _hip as H
    from nerf import ops
    dev = torch.device("cuda:0")
    kw = dict(num_encoding_fn_xyz=10, num_encoding_fn_dir=4, include_input_xyz=True, include_input_dir=False, use_viewdirs=True,
              num_layers=4, hidden_size=256, include_expression=True)
    torch.manual_seed(0)
    models = {"paper": nerf.models.ConditionalBlendshapePaperNeRFModel(**kw).to(dev),
              "smaller": nerf.models.ConditionalBlendshapePaperSmallerNeRFModel(**kw).to(dev)}
    g = torch.Generator().manual_seed(1)
    expr = (torch.randn(76, generator=g) * 0.5).to(dev)
    latent = (torch.randn(32, generator=g) * 0.1).to(dev)
    near, far = 0.2, 0.8

    def rays(n_rays, n_samples):
        ro = (torch.randn((n_rays, 3), generator=g) * 0.05 + torch.tensor([0.0, 0.0, 0.5])).to(dev)
        rd = torch.nn.functional.normalize(torch.randn((n_rays, 3), generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0]), dim=-1).to(dev)
        z = torch.sort(torch.rand((n_rays, n_samples), generator=g) * (far - near) + near, dim=-1)[0].to(dev)
        return ro, rd, z

    def timed(fns, repeats, warmup):
        """fns: name -> callable that enqueues one launch.  Alternates them; returns name -> list of milliseconds (device events)."""
        for _ in range(warmup):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(repeats):
            for k, f in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return ms

    med = lambda v: statistics.median(v)
    rows = []                                           # (what, paper ms, smaller ms, paper spread, smaller spread)

    # ---- inference forward at the fine-pass shape --------------------------------------------------------------------------------
    ro, rd, z = rays(a.rays, a.samples)
    state = {}
    for name, m in models.items():
        fam, hw = m.FAMILY, m.hip_weights()
        packed = hw.get()
        state[name] = (fam, packed, ops.mlp_condition(fam, packed, expr, latent, near, far))
    ms = timed({name: (lambda s=s: ops.mlp_fwd(s[0], "f32", s[1], s[2], ro, rd, z)) for name, s in state.items()}, a.repeats, a.warmup)
    fwd = {k: med(v) for k, v in ms.items()}
    rows.append((f"inference forward, {a.rays} x {a.samples}", ms["paper"], ms["smaller"]))

    # ---- training forward and backward stages at a training step's fine pass -------------------------------------------------------
    ro_t, rd_t, z_t = rays(a.train_rays, a.train_samples)
    n_pts = a.train_rays * a.train_samples
    d_raw = (torch.randn((a.train_rays, a.train_samples, 4), generator=g) * 1e-4).to(dev)
    ms = timed({name: (lambda s=s: ops.mlp_fwd_train(s[0], s[1], s[2], ro_t, rd_t, z_t)) for name, s in state.items()}, a.repeats, a.warmup)
    rows.append((f"training forward, {a.train_rays} x {a.train_samples}", ms["paper"], ms["smaller"]))
    stage = {name: [[], [], []] for name in models}
    bwd = {}
    for name, m in models.items():
        fam, packed, cond = state[name]
        _, (saved,) = ops.mlp_fwd_train(fam, packed, cond, ro_t, rd_t, z_t)
        ws_floats = fam.fn("bwd_workspace_floats")(n_pts)
        ws = torch.empty(ws_floats, dtype=torch.float32, device=dev)
        flat = torch.empty(fam.fn("grad_floats")(), dtype=torch.float32, device=dev)
        packed_t = m.hip_weights().get_t()
        out = (C.c_float * 3)()
        common = (H.ptr(cond), H.ptr(saved), H.ptr(d_raw), a.train_rays, a.train_samples, H.ptr(ws), ws_floats, H.ptr(flat), out,
                  H.stream_ptr(dev))
        if name == "paper":
            bwd[name] = (lambda packed=packed, packed_t=packed_t, common=common, out=out, keep=(saved, ws, flat):
                         (H.check(H.lib().nf_paper_mlp_bwd_stage_ms(H.ptr(packed), H.ptr(packed_t), 0, *common), "nf_paper_mlp_bwd_stage_ms"), list(out))[1])
        else:
            bwd[name] = (lambda packed=packed, packed_t=packed_t, common=common, out=out, keep=(saved, ws, flat):
                         (H.check(H.lib().nf_smaller_mlp_bwd_stage_ms(H.ptr(packed), H.ptr(packed_t), *common), "nf_smaller_mlp_bwd_stage_ms"), list(out))[1])
    for it in range(a.warmup + a.repeats):
        for name in models:
            t3 = bwd[name]()
            if it >= a.warmup:
                for k in range(3):
                    stage[name][k].append(t3[k])
    for k, what in enumerate(("backward: dX chain", "backward: weight-gradient GEMMs", "backward: reduce + scatter")):
        rows.append((f"{what}, {a.train_rays} x {a.train_samples}", stage["paper"][k], stage["smaller"][k]))

    # ---- report --------------------------------------------------------------------------------------------------------------------
    ratio = fwd["smaller"] / fwd["paper"]
    instr = MFMA["smaller"] / MFMA["paper"]
    bound = instr * 1.05
    props = torch.cuda.get_device_properties(dev)
    lines = ["# Smaller paper model family: exact-f32 kernels beside the paper family's", "",
             f"Command: `python tools/time_smaller.py --rays {a.rays} --samples {a.samples} --train-rays {a.train_rays} "
             f"--train-samples {a.train_samples} --repeats {a.repeats} --warmup {a.warmup}`", "",
             f"Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}.  One process; the two families' launches "
             f"alternate in one loop; device events around every launch; median of {a.repeats} after {a.warmup} warm-up rounds "
             "(min .. max in brackets).", "",
             "| kernel | paper family, ms | smaller family, ms | smaller / paper |", "|---|---|---|---|"]
    for what, p, s in rows:
        lines.append(f"| {what} | {med(p):.3f} ({min(p):.3f} .. {max(p):.3f}) | {med(s):.3f} ({min(s):.3f} .. {max(s):.3f}) | {med(s) / med(p):.3f} |")
    n_points = a.rays * a.samples
    lines += ["",
              f"Inference forward: {n_points} points.  MFMAs per 16 points: paper {MFMA['paper']}, smaller {MFMA['smaller']} "
              f"(instruction ratio {instr:.3f}).  Achieved exact-f32 matrix rate (2 x 16 x 16 x 4 FLOP per MFMA over kernel time): "
              f"paper {MFMA['paper'] * 2048 * (n_points / 16) / (fwd['paper'] * 1e-3) / 1e12:.1f} TFLOP/s, "
              f"smaller {MFMA['smaller'] * 2048 * (n_points / 16) / (fwd['smaller'] * 1e-3) / 1e12:.1f} TFLOP/s.", "",
              f"Yardstick: smaller / paper time <= {instr:.3f} x 1.05 = {bound:.3f}.  Measured {ratio:.3f}: "
              + ("**met**." if ratio <= bound else "**MISSED**."), ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
