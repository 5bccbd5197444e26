"""Time mesh smoothing -- the adjacency build, one pass, ten Taubin iterations, the vertex normals -- on the sphere meshes of
profiles/mesh_components.md.  Writes the table of profiles/mesh_smooth.md (and prints it).

    python tools/time_mesh_smooth.py [--sizes 128 256 512] [--repeats 7] [--warmup 2] [--out profiles/mesh_smooth.md]

Per grid size N^3: ops.isosurface (normals on) of r^2 - |p|^2 with r = 0.7 on [-1, 1]^3 at level 0, then, on preallocated buffers,
nf_mesh_smooth_adjacency, nf_mesh_smooth_run with one pass (iterations = 1, mu = 0) and with ten Taubin iterations (20 passes), and
nf_mesh_smooth_normals; ops.smooth_mesh as a user calls it (ten iterations, normals, allocations and the one host read included).
The launches of a row alternate inside one loop with device events around each; the figure is the median, the spread min .. max.
The yardstick is the mesh pipeline's: a mesh step stays below 5 % of the f16x2 density evaluation of the same grid, whose medians
are taken from profiles/isosurface.md.
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


def sphere(n, dev):
    ax = torch.linspace(-1.0, 1.0, n, device=dev)
    return (0.49 - (ax.view(1, 1, n) ** 2 + ax.view(1, n, 1) ** 2 + ax.view(n, 1, 1) ** 2)).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_smooth.md"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_smooth.py measures on a ROCm device; none is visible")
    from nerf import _hip as H
    from nerf import ops
    dev = torch.device("cuda:0")
    lib, stream = H.lib(), H.stream_ptr(dev)
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)

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
    lines = ["# Mesh smoothing: measured", "",
             f"Command: `python tools/time_mesh_smooth.py --sizes {' '.join(map(str, a.sizes))} --repeats {a.repeats} --warmup {a.warmup}`", "",
             f"Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}.  One process; the launches of a row alternate in "
             f"one loop; device events around each; median of {a.repeats} after {a.warmup} warm-up rounds (min .. max in brackets), milliseconds.  "
             "Meshes: ops.isosurface (normals on) of r^2 - |p|^2 with r = 0.7 on [-1, 1]^3 at level 0 (closed: nothing is pinned).  `adjacency`: "
             "nf_mesh_smooth_adjacency (eleven kernels) on preallocated buffers; `one pass`: nf_mesh_smooth_run with iterations = 1, mu = 0; "
             "`ten iterations`: nf_mesh_smooth_run with the defaults (20 passes); `normals`: nf_mesh_smooth_normals (nine kernels); `ops.smooth_mesh`: "
             "all of it as a user calls it -- adjacency, 20 passes, normals, the allocations and the one host read; `bound`: 5 % of the f16x2 density "
             "evaluation of the same grid (profiles/isosurface.md).", "",
             "| grid | V | F | E | adjacency, ms | one pass, ms | ten iterations, ms | normals, ms | adjacency + ten iterations + normals, ms | "
             "ops.smooth_mesh, ms | bound, ms | adjacency | ten iterations | normals | all |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in a.sizes:
        verts, faces, norm = ops.isosurface(sphere(n, dev), 0.0, lo, hi, normals=True)
        n_v, n_f = verts.shape[0], faces.shape[0]
        ws_bytes = int(lib.nf_mesh_smooth_workspace_bytes(n_v, n_f))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
        row_start, neighbours, multiplicity = i32(n_v + 1), i32(6 * n_f), i32(6 * n_f)
        boundary = torch.empty(n_v, dtype=torch.uint8, device=dev)
        tmp, out, out_n = torch.empty_like(verts), torch.empty_like(verts), torch.empty_like(verts)

        def adjacency():
            H.check(lib.nf_mesh_smooth_adjacency(H.ptr(faces), n_v, n_f, H.ptr(ws), ws_bytes, H.ptr(row_start), H.ptr(neighbours), H.ptr(multiplicity),
                                                 H.ptr(boundary), H.ptr(counts), stream), "nf_mesh_smooth_adjacency")

        def run(iterations, mu):
            H.check(lib.nf_mesh_smooth_run(H.ptr(verts), n_v, H.ptr(row_start), H.ptr(neighbours), H.ptr(boundary), iterations, 0.5, mu, H.ptr(tmp),
                                           H.ptr(out), stream), "nf_mesh_smooth_run")

        def normals():
            H.check(lib.nf_mesh_smooth_normals(H.ptr(out), H.ptr(faces), n_v, n_f, H.ptr(ws), ws_bytes, H.ptr(out_n), stream), "nf_mesh_smooth_normals")

        adjacency()
        n_e = int(counts[0].item())
        ms = timed({"adjacency": adjacency, "pass": lambda: run(1, 0.0), "ten": lambda: run(10, -0.53), "normals": normals,
                    "python": lambda: ops.smooth_mesh(verts, faces, norm)})
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(ops.smooth_mesh(verts, faces, norm)[:3:2], (out, out_n)))
        every = [x + y + z for x, y, z in zip(ms["adjacency"], ms["ten"], ms["normals"])]
        bound = 0.05 * DENSITY_F16X2_MS[n] if n in DENSITY_F16X2_MS else None
        verdict = lambda v: "n/a" if bound is None else ("yes" if statistics.median(v) <= bound else "NO")
        lines.append(f"| {n}^3 | {n_v} | {n_f} | {n_e} | {cell(ms['adjacency'])} | {cell(ms['pass'])} | {cell(ms['ten'])} | {cell(ms['normals'])} | {cell(every)} | "
                     f"{cell(ms['python'])} | {'n/a' if bound is None else f'{bound:.2f}'} | {verdict(ms['adjacency'])} | {verdict(ms['ten'])} | "
                     f"{verdict(ms['normals'])} | {verdict(every)}{'' if same else ' (OUTPUTS DIFFER)'} |")
        del ws, row_start, neighbours, multiplicity, boundary, tmp, out, out_n, verts, faces, norm
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
