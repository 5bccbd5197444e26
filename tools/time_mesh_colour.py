"""Time the mesh colour pass -- the rays kernel, the composite, the network's share and the whole of nerf.vertex_colours -- on the sphere
meshes of profiles/mesh_components.md.  Writes the table of profiles/mesh_colour.md (and prints it).

    python tools/time_mesh_colour.py [--sizes 128 256 512] [--samples 8] [--repeats 7] [--warmup 2] [--out profiles/mesh_colour.md]

Per grid size N^3: ops.isosurface (normals on) of r^2 - |p|^2 with r = 0.7 on [-1, 1]^3 at level 0, then, on preallocated buffers,
nf_mesh_colour_rays (with a camera pose) and nf_mesh_colour_integrate on the network's own output; the full forward of a paper model
on the V x K points of those rays (model.hip_forward) in f32 and f16x2; and nerf.vertex_colours as a user calls it, in both
arithmetics (slabs, allocations and the split-fp16 range read included).  The launches of a row alternate inside one loop with device
events around each; the figure is the median, the spread min .. max.  The yardstick is the mesh pipeline's: a mesh step stays below
5 % of the f16x2 density evaluation of the same grid, whose medians are taken from profiles/isosurface.md; it is held against the
two new kernels -- the network's V x K full forwards are the network's cost.  The byte floor of a kernel is what it must read and
write over 6.3 TB/s, the copy rate of the device.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))

import torch  # noqa: E402

DENSITY_F16X2_MS = {128: 3.7, 256: 28.0, 512: 214.0}          # profiles/isosurface.md: nerf.density_grid of the paper model, f16x2
HBM_BYTES_PER_MS = 6.3e9                                      # 6.3 TB/s: what a float4 copy reaches
NEAR, FAR = 0.2, 0.8


def sphere(n, dev):
    ax = torch.linspace(-1.0, 1.0, n, device=dev)
    return (0.49 - (ax.view(1, 1, n) ** 2 + ax.view(1, n, 1) ** 2 + ax.view(n, 1, 1) ** 2)).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_colour.md"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_colour.py measures on a ROCm device; none is visible")
    import nerf
    from nerf import _hip as H
    from nerf import ops
    dev = torch.device("cuda:0")
    lib, stream = H.lib(), H.stream_ptr(dev)
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    k = a.samples
    torch.manual_seed(3)
    model = nerf.models.ConditionalBlendshapePaperNeRFModel(num_encoding_fn_xyz=10, num_encoding_fn_dir=4, include_input_dir=False).to(dev).eval()
    expr, latent = torch.randn(76, device=dev) * 0.3, torch.randn(32, device=dev) * 0.1
    pose = torch.tensor([[1.0, 0.0, 0.0, 0.1], [0.0, 1.0, 0.0, -0.05], [0.0, 0.0, 1.0, 3.0]], device=dev)       # in front of the box, looking down -z

    def timed(fns):
        for _ in range(a.warmup):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        ms = {name: [] for name in fns}
        for _ in range(a.repeats):
            for name, f in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        return ms

    def cell(v):
        return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"

    props = torch.cuda.get_device_properties(dev)
    lines = ["# Mesh colours: measured", "",
             f"Command: `python tools/time_mesh_colour.py --sizes {' '.join(map(str, a.sizes))} --samples {k} --repeats {a.repeats} --warmup {a.warmup}`", "",
             f"Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}.  One process; the launches of a row alternate in "
             f"one loop; device events around each; median of {a.repeats} after {a.warmup} warm-up rounds (min .. max in brackets), milliseconds.  "
             f"Meshes: ops.isosurface (normals on) of r^2 - |p|^2 with r = 0.7 on [-1, 1]^3 at level 0; K = {k} samples, depth = a cell's diagonal, a "
             "camera pose.  `rays`: nf_mesh_colour_rays on preallocated buffers; `integrate`: nf_mesh_colour_integrate on the network's output; their "
             "`floor`: the bytes each must move (rays: 24 V read, (24 + 4 K) V written; integrate: 16 K V read, 16 V written) over 6.3 TB/s; `MLP`: "
             "model.hip_forward of a paper model on the V x K points, no slabs; `vertex_colours`: nerf.vertex_colours as a user calls it (slabs of "
             "2^22 points, allocations, in f16x2 the range read); `bound`: 5 % of the f16x2 density evaluation of the same grid "
             "(profiles/isosurface.md), held against rays + integrate.", "",
             "| grid | V | rays, ms | floor, ms | integrate, ms | floor, ms | rays + integrate, ms | bound, ms | within | MLP f32, ms | MLP f16x2, ms | "
             "vertex_colours f32, ms | vertex_colours f16x2, ms | MLP share f32 | MLP share f16x2 |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in a.sizes:
        verts, faces, norm = ops.isosurface(sphere(n, dev), 0.0, lo, hi, normals=True)
        mesh = nerf.Mesh(verts, faces, norm)
        n_v = verts.shape[0]
        depth = float(3 ** 0.5 * 2.0 / (n - 1))
        step = ops.mesh_colour_step(depth, k)
        rd, rd_view = torch.empty_like(verts), torch.empty_like(verts)
        z = torch.empty((n_v, k), dtype=torch.float32, device=dev)
        colour, opacity = torch.empty_like(verts), torch.empty(n_v, dtype=torch.float32, device=dev)

        def rays():
            H.check(lib.nf_mesh_colour_rays(H.ptr(verts), H.ptr(norm), n_v, H.ptr(pose), 4, 0.0, k, depth, H.ptr(rd), H.ptr(rd_view), H.ptr(z), stream),
                    "nf_mesh_colour_rays")

        rays()
        raw = {}
        with torch.no_grad():
            for prec in ("f32", "f16x2"):
                nerf.set_mlp_precision(prec)
                ops.bump_pack_epoch()
                raw[prec] = model.hip_forward(verts, rd, z, rd_view, expr, latent, NEAR, FAR, False)[0]

        def integrate():
            H.check(lib.nf_mesh_colour_integrate(H.ptr(raw["f32"]), n_v, k, step, 1e-3, H.ptr(colour), H.ptr(opacity), stream), "nf_mesh_colour_integrate")

        def mlp(prec):
            nerf.set_mlp_precision(prec)
            with torch.no_grad():
                model.hip_forward(verts, rd, z, rd_view, expr, latent, NEAR, FAR, False)

        def whole(prec):
            nerf.set_mlp_precision(prec)
            return nerf.vertex_colours(model, mesh, expr, latent, near=NEAR, far=FAR, pose=pose, samples=k, depth=depth)

        ms = timed({"rays": rays, "integrate": integrate, "mlp32": lambda: mlp("f32"), "mlp16": lambda: mlp("f16x2"), "all32": lambda: whole("f32"),
                    "all16": lambda: whole("f16x2")})
        nerf.set_mlp_precision("f32")
        got = whole("f32")
        same = torch.equal(got.colours.view(torch.int32), colour.view(torch.int32)) and torch.equal(got.opacity.view(torch.int32), opacity.view(torch.int32))
        both = [x + y for x, y in zip(ms["rays"], ms["integrate"])]
        floor_rays, floor_int = (24 + 24 + 4 * k) * n_v / HBM_BYTES_PER_MS, (16 * k + 16) * n_v / HBM_BYTES_PER_MS
        bound = 0.05 * DENSITY_F16X2_MS[n] if n in DENSITY_F16X2_MS else None
        verdict = "n/a" if bound is None else ("yes" if statistics.median(both) <= bound else "NO")
        share = lambda part, total: f"{100.0 * statistics.median(ms[part]) / statistics.median(ms[total]):.0f} %"
        lines.append(f"| {n}^3 | {n_v} | {cell(ms['rays'])} | {floor_rays:.4f} | {cell(ms['integrate'])} | {floor_int:.4f} | {cell(both)} | "
                     f"{'n/a' if bound is None else f'{bound:.2f}'} | {verdict}{'' if same else ' (OUTPUTS DIFFER)'} | {cell(ms['mlp32'])} | {cell(ms['mlp16'])} | "
                     f"{cell(ms['all32'])} | {cell(ms['all16'])} | {share('mlp32', 'all32')} | {share('mlp16', 'all16')} |")
        del verts, faces, norm, mesh, rd, rd_view, z, colour, opacity, raw
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
