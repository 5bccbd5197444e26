"""Time the two blendshape families (nf_bshape_*, nf_cbshape_*) beside the second family (nf_lcode_*), whose per-point kernels they
launch -- same GPU, same process, same points.  Writes profiles/blendshape_families.md (and prints it).

    python tools/time_blendshape.py [--rays 65536] [--samples 192] [--repeats 15] [--out profiles/blendshape_families.md]

The three families' launches alternate inside one timed loop (device events around every launch, the backward's stages by the
library's <prefix>_mlp_bwd_stage_ms hooks); the figure is the median of `repeats` after `warmup` rounds.  Inference forward at the
benchmark's fine-pass shape, training forward and the three backward stages at a training step's fine pass, each in "f32" and
"f16x3"; the `condition` launch of each family on its own.
Yardstick: a new family runs the second family's code objects on same-sized images, so its time is held to the second family's time
IN THE SAME RUN; the margin is twice the second family's own (max - min) / median spread over its repeats.  The reduce + scatter row of
nf_cbshape carries the encoder's backward workgroup: reported, not gated.
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

FAMILIES = ("lcode", "bshape", "cbshape")
CLASSES = {"lcode": "ConditionalBlendshapeLearnableCodeNeRFModel", "bshape": "ConditionalBlendshapeNeRFModel",
           "cbshape": "ConditionalCompressedBlendshapeNeRFModel"}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=192)
    ap.add_argument("--train-rays", type=int, default=2048)
    ap.add_argument("--train-samples", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blendshape_families.md"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_blendshape.py measures on a ROCm device; none is visible")
    import nerf
    from nerf import _hip as H
    from nerf import ops
    dev = torch.device("cuda:0")
    kw = dict(num_encoding_fn_xyz=10, num_encoding_fn_dir=4, include_input_xyz=True, include_input_dir=False, use_viewdirs=True,
              num_layers=4, hidden_size=256, include_expression=True)
    torch.manual_seed(0)
    models = {f: getattr(nerf.models, CLASSES[f])(**kw).to(dev) for f in FAMILIES}
    g = torch.Generator().manual_seed(1)
    expr = (torch.randn(76, generator=g) * 0.5).to(dev)
    latent = (torch.randn(32, generator=g) * 0.1).to(dev)
    near, far = 0.2, 0.8

    def rays(n_rays, n_samples):
        ro = (torch.randn((n_rays, 3), generator=g) * 0.05 + torch.tensor([0.0, 0.0, 0.5])).to(dev)
        rd = torch.nn.functional.normalize(torch.randn((n_rays, 3), generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0]), dim=-1).to(dev)
        z = torch.sort(torch.rand((n_rays, n_samples), generator=g) * (far - near) + near, dim=-1)[0].to(dev)
        return ro, rd, z

    def timed(fns):
        """fns: family -> callable that enqueues one launch.  Alternates them; returns family -> list of milliseconds (device events)."""
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

    rows = []                                           # (what, gated, family -> list of ms)
    ro, rd, z = rays(a.rays, a.samples)
    ro_t, rd_t, z_t = rays(a.train_rays, a.train_samples)
    n_pts = a.train_rays * a.train_samples
    d_raw = (torch.randn((a.train_rays, a.train_samples, 4), generator=g) * 1e-4).to(dev)
    fams = {f: m.FAMILY for f, m in models.items()}
    hws = {f: m.hip_weights() for f, m in models.items()}
    packed = {f: hws[f].get() for f in FAMILIES}
    cond = {f: ops.mlp_condition(fams[f], packed[f], expr, latent, near, far) for f in FAMILIES}

    rows.append(("condition (bias table of one call)", False,
                 timed({f: (lambda f=f: ops.mlp_condition(fams[f], packed[f], expr, latent, near, far)) for f in FAMILIES})))
    for prec in ("f32", "f16x3"):
        image = {f: packed[f] if prec == "f32" else hws[f].get_f16() for f in FAMILIES}
        rows.append((f"inference forward {prec}, {a.rays} x {a.samples}", True,
                     timed({f: (lambda f=f: ops.mlp_fwd(fams[f], prec, image[f], cond[f], ro, rd, z)) for f in FAMILIES})))
        ph = {f: None if prec == "f32" else image[f] for f in FAMILIES}
        rows.append((f"training forward {prec}, {a.train_rays} x {a.train_samples}", True,
                     timed({f: (lambda f=f: ops.mlp_fwd_train(fams[f], packed[f], cond[f], ro_t, rd_t, z_t, packed_h=ph[f])) for f in FAMILIES})))
        stage = {f: [[], [], []] for f in FAMILIES}
        bwd = {}
        for f in FAMILIES:
            _, (saved,) = ops.mlp_fwd_train(fams[f], packed[f], cond[f], ro_t, rd_t, z_t, packed_h=ph[f])
            ws_floats = fams[f].fn("bwd_workspace_floats")(n_pts)
            ws = torch.empty(ws_floats, dtype=torch.float32, device=dev)
            flat = torch.empty(fams[f].fn("grad_floats")(), dtype=torch.float32, device=dev)
            packed_t = hws[f].get_t() if prec == "f32" else hws[f].get_f16_t()
            out = (C.c_float * 3)()
            args = (H.ptr(packed[f]), H.ptr(packed_t), 0 if prec == "f32" else 2, H.ptr(cond[f]), H.ptr(saved), H.ptr(d_raw), a.train_rays,
                    a.train_samples, H.ptr(ws), ws_floats, H.ptr(flat), out, H.stream_ptr(dev))
            bwd[f] = (lambda f=f, args=args, out=out, keep=(saved, ws, flat, packed_t):
                      (fams[f].call("mlp_bwd_stage_ms", *args), list(out))[1])
        for it in range(a.warmup + a.repeats):
            for f in FAMILIES:
                t3 = bwd[f]()
                if it >= a.warmup:
                    for k in range(3):
                        stage[f][k].append(t3[k])
        for k, what in enumerate(("backward: dX chain", "backward: weight-gradient GEMMs", "backward: reduce + scatter")):
            rows.append((f"{what} {prec}, {a.train_rays} x {a.train_samples}", True, {f: stage[f][k] for f in FAMILIES}))

    # ---- report --------------------------------------------------------------------------------------------------------------------
    med = statistics.median
    props = torch.cuda.get_device_properties(dev)
    lines = ["# The two blendshape families beside the second family, whose per-point kernels they launch", "",
             f"Command: `python tools/time_blendshape.py --rays {a.rays} --samples {a.samples} --train-rays {a.train_rays} "
             f"--train-samples {a.train_samples} --repeats {a.repeats} --warmup {a.warmup}`", "",
             f"Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}.  One process; the three families' launches "
             f"alternate in one loop; device events around every launch; median of {a.repeats} after {a.warmup} warm-up rounds.", "",
             "Yardstick per row: new family's median <= second family's median x (1 + margin), margin = 2 x the second family's own "
             "(max - min) / median over its repeats in this run (same code object: only run-to-run noise separates them).  The `condition` "
             "rows and nf_cbshape's reduce + scatter rows (the encoder's backward workgroup rides there) are reported, not gated.", "",
             "| launch | nf_lcode ms (min .. max) | spread | margin | nf_bshape ms | / lcode | verdict | nf_cbshape ms | / lcode | verdict |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    notes = []
    for what, gated, ms in rows:
        l = ms["lcode"]
        spread = (max(l) - min(l)) / med(l)
        margin = 2 * spread
        cells = [what, f"{med(l):.4f} ({min(l):.4f} .. {max(l):.4f})", f"{spread:.3f}", f"{margin:.3f}"]
        for f in ("bshape", "cbshape"):
            r = med(ms[f]) / med(l)
            gate = gated and not (f == "cbshape" and "reduce + scatter" in what)
            verdict = ("met" if r <= 1 + margin else "NOT met") if gate else "reported"
            if not gate and r > 1 + margin:
                notes.append(f"{what}, nf_{f}: {med(ms[f]) - med(l):+.4f} ms against the second family ({r:.3f} x), beyond the noise margin {margin:.3f}.")
            cells += [f"{med(ms[f]):.4f}", f"{r:.3f}", verdict]
        lines.append("| " + " | ".join(cells) + " |")
    lines += ["", "Rows reported beyond the noise margin (nf_cbshape's condition launch evaluates the 76 -> 38 -> 20 -> 20 encoder in every "
              "workgroup before it fills the table; its reduce + scatter launch ends with one workgroup that runs the encoder's backward, "
              "a chain of seven block-wide barriers, while the second family's last workgroup sums 32 latent gradients):", ""]
    lines += [f"* {n}" for n in notes] or ["* none"]
    lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
