"""Time the isosurface extraction beside the density evaluation that feeds it -- same GPU, same process, same grid.  Writes
profiles/isosurface.md (and prints it).

    python tools/time_isosurface.py [--sizes 128 256 512] [--repeats 7] [--warmup 2] [--out profiles/isosurface.md]

Per grid size N^3: nf_isosurface_count + nf_isosurface_emit (with normals) on a sphere field r^2 - |p|^2 with preallocated outputs,
ops.isosurface as a user calls it (allocations and the one host read included), and nerf.density_grid of the paper model on the same
grid in "f32" and "f16x2".  The launches of a row alternate inside one loop with device events around each; the figure is the median,
the spread min .. max.  `floor` is the bytes the four kernels must move (12 per point: the grid once, mask / inside bits written and
read, the vertex bases written; plus the outputs) over 8 TB/s.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4d-facial-avatars_amd"))

import torch  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isosurface.md"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_isosurface.py measures on a ROCm device; none is visible")
    import nerf
    from nerf import _hip as H
    from nerf import ops
    dev = torch.device("cuda:0")
    lib, stream = H.lib(), H.stream_ptr(dev)
    torch.manual_seed(0)
    model = nerf.models.ConditionalBlendshapePaperNeRFModel(num_encoding_fn_xyz=10, num_encoding_fn_dir=4, include_input_xyz=True,
                                                            include_input_dir=False, use_viewdirs=True, num_layers=4, hidden_size=256,
                                                            include_expression=True).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    expr, latent = (torch.randn(76, generator=g) * 0.5).to(dev), (torch.randn(32, generator=g) * 0.1).to(dev)
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    d_lo, d_hi = (-0.4, -0.4, -0.4), (0.4, 0.4, 0.4)                    # the density is timed where the model's test points lie
    c_lo, c_hi = (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi)

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
    lines = ["# Isosurface extraction: measured", "",
             f"Command: `python tools/time_isosurface.py --sizes {' '.join(map(str, a.sizes))} --repeats {a.repeats} --warmup {a.warmup}`", "",
             f"Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}.  One process; the launches of a row alternate in "
             f"one loop; device events around each; median of {a.repeats} after {a.warmup} warm-up rounds (min .. max in brackets), milliseconds.  "
             "Field of the extraction: r^2 - |p|^2, r = 0.7, on [-1, 1]^3, level 0, normals on.  `count + emit`: the four kernels on preallocated "
             "outputs; `ops.isosurface`: the same with its allocations and its one host read; `floor`: bytes the kernels must move "
             "(12 per point + 24 per vertex + 12 per face) / 8 TB/s.  Density: nerf.density_grid of the paper model (default initialisation) "
             "on the same number of points.", "",
             "| grid | V | F | count + emit, ms | floor, ms | floor / measured | ops.isosurface, ms | density f32, ms | density f16x2, ms | "
             "count + emit / density f16x2 | below 5 % |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in a.sizes:
        ax = torch.linspace(-1.0, 1.0, n, device=dev)
        field = (0.49 - (ax.view(1, 1, n) ** 2 + ax.view(1, n, 1) ** 2 + ax.view(n, 1, 1) ** 2)).contiguous()
        ws_bytes = int(lib.nf_isosurface_workspace_bytes(n, n, n))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        H.check(lib.nf_isosurface_count(H.ptr(field), n, n, n, 0.0, H.ptr(ws), ws_bytes, H.ptr(counts), stream), "nf_isosurface_count")
        n_v, n_f = counts.tolist()
        verts, norm = torch.empty((n_v, 3), device=dev), torch.empty((n_v, 3), device=dev)
        faces = torch.empty((n_f, 3), dtype=torch.int32, device=dev)

        def kernels():
            H.check(lib.nf_isosurface_count(H.ptr(field), n, n, n, 0.0, H.ptr(ws), ws_bytes, H.ptr(counts), stream), "nf_isosurface_count")
            H.check(lib.nf_isosurface_emit(H.ptr(field), n, n, n, 0.0, ctypes.addressof(c_lo), ctypes.addressof(c_hi), H.ptr(ws), ws_bytes,
                                           H.ptr(verts), n_v, H.ptr(faces), n_f, H.ptr(norm), stream), "nf_isosurface_emit")

        def density(precision):
            def run():
                nerf.set_mlp_precision(precision)
                try:
                    nerf.density_grid(model, expr, latent, lo=d_lo, hi=d_hi, resolution=n)
                finally:
                    nerf.set_mlp_precision("f32")
            return run

        ms = timed({"kernels": kernels, "python": lambda: ops.isosurface(field, 0.0, lo, hi, normals=True), "f32": density("f32"),
                    "f16x2": density("f16x2")})
        same = all(torch.equal(x, y) for x, y in zip(ops.isosurface(field, 0.0, lo, hi, normals=True), (verts, faces, norm)))
        floor_ms = 1e3 * (12.0 * n ** 3 + 24.0 * n_v + 12.0 * n_f) / HBM_BYTES_PER_S
        k, d = statistics.median(ms["kernels"]), statistics.median(ms["f16x2"])
        lines.append(f"| {n}^3 | {n_v} | {n_f} | {cell(ms['kernels'])} | {floor_ms:.3f} | {floor_ms / k:.2f} | {cell(ms['python'])} | {cell(ms['f32'])} | "
                     f"{cell(ms['f16x2'])} | {100.0 * k / d:.2f} % | {'yes' if k <= 0.05 * d else 'NO'}{'' if same else ' (OUTPUTS DIFFER)'} |")
        del field, ws, verts, norm, faces
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
