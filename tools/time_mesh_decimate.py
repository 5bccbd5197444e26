"""Time mesh decimation -- nf_mesh_decimate_count, nf_mesh_decimate_emit, ops.decimate_mesh -- on the sphere meshes of
profiles/mesh_components.md.  Writes the table of profiles/mesh_decimate.md (and prints it).

    python tools/time_mesh_decimate.py [--sizes 128 256 512] [--cells 1 2 4 8] [--repeats 7] [--warmup 2] [--out profiles/mesh_decimate.md]

Per grid size N^3: ops.isosurface (normals on) of r^2 - |p|^2 with r = 0.7 on [-1, 1]^3 at level 0, then, per K, decimation on cells
of K grid cells from the box's corner, and once on a single cell that holds every vertex (every member adds to the same three
accumulators).  On preallocated buffers nf_mesh_decimate_count and nf_mesh_decimate_emit (which reads V' and F' back before it
launches, so its time includes that wait); ops.decimate_mesh as a user calls it (normals recomputed, allocations and the one host
read included).  Beside them nf_mesh_smooth_adjacency on the same mesh, a table build of comparable work.  The launches of a row
alternate inside one loop with device events around each; the figure is the median, the spread min .. max.  No time here is a pass
criterion.
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


def sphere(n, dev):
    ax = torch.linspace(-1.0, 1.0, n, device=dev)
    return (0.49 - (ax.view(1, 1, n) ** 2 + ax.view(1, n, 1) ** 2 + ax.view(n, 1, 1) ** 2)).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--cells", type=float, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_decimate.md"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_decimate.py measures on a ROCm device; none is visible")
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
    lines = ["# Mesh decimation: measured", "",
             f"Command: `python tools/time_mesh_decimate.py --sizes {' '.join(map(str, a.sizes))} --cells {' '.join(f'{k:g}' for k in a.cells)} "
             f"--repeats {a.repeats} --warmup {a.warmup}`", "",
             f"Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}.  One process; the launches of a row alternate in "
             f"one loop; device events around each; median of {a.repeats} after {a.warmup} warm-up rounds (min .. max in brackets), milliseconds.  "
             "Meshes: ops.isosurface (normals on) of r^2 - |p|^2 with r = 0.7 on [-1, 1]^3 at level 0.  `K`: the edge of a decimation cell in grid "
             "cells, the lattice from the box's corner; `one cell`: a single cell round the whole mesh, so that every vertex adds to the same three "
             "accumulators and every face is degenerate.  `count`: nf_mesh_decimate_count (twelve kernels) on preallocated buffers; `emit`: "
             "nf_mesh_decimate_emit (three kernels behind a read of V' and F', whose wait is in the figure); `ops.decimate_mesh`: all of it as a user "
             "calls it -- count, the one host read, the allocations, emit, and the normals of the result; `adjacency`: nf_mesh_smooth_adjacency "
             "(eleven kernels) on the same mesh, a table build of comparable work.  No time here is a pass criterion.", "",
             "| grid | V | F | K | V' | F' | largest cluster | count, ms | emit, ms | count + emit, ms | ops.decimate_mesh, ms | adjacency, ms |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in a.sizes:
        verts, faces, norm = ops.isosurface(sphere(n, dev), 0.0, lo, hi, normals=True)
        n_v, n_f = verts.shape[0], faces.shape[0]
        ws_bytes = int(lib.nf_mesh_decimate_workspace_bytes(n_v, n_f))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(8, dtype=torch.int64, device=dev)
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
        ms_bytes = int(lib.nf_mesh_smooth_workspace_bytes(n_v, n_f))
        ms_ws, ms_counts = torch.empty(ms_bytes, dtype=torch.uint8, device=dev), torch.empty(2, dtype=torch.int64, device=dev)
        row_start, neighbours, multiplicity, boundary = i32(n_v + 1), i32(6 * n_f), i32(6 * n_f), torch.empty(n_v, dtype=torch.uint8, device=dev)
        out_v, out_f, vertex_map = torch.empty_like(verts), torch.empty_like(faces), i32(n_v)
        h = 2.0 / (n - 1)

        def adjacency():
            H.check(lib.nf_mesh_smooth_adjacency(H.ptr(faces), n_v, n_f, H.ptr(ms_ws), ms_bytes, H.ptr(row_start), H.ptr(neighbours), H.ptr(multiplicity),
                                                 H.ptr(boundary), H.ptr(ms_counts), stream), "nf_mesh_smooth_adjacency")

        for k in list(a.cells) + [None]:
            size, origin = (k * h, lo) if k is not None else (4.0, (-2.0, -2.0, -2.0))
            c_origin, c_cell = (ctypes.c_float * 3)(*origin), (ctypes.c_float * 3)(size, size, size)
            found = {}

            def count():
                H.check(lib.nf_mesh_decimate_count(H.ptr(verts), H.ptr(faces), n_v, n_f, ctypes.addressof(c_origin), ctypes.addressof(c_cell), H.ptr(ws),
                                                   ws_bytes, H.ptr(counts), stream), "nf_mesh_decimate_count")

            def emit():
                H.check(lib.nf_mesh_decimate_emit(H.ptr(verts), H.ptr(faces), n_v, n_f, ctypes.addressof(c_origin), ctypes.addressof(c_cell), H.ptr(ws),
                                                  ws_bytes, H.ptr(out_v), found["v"], H.ptr(out_f), found["f"], H.ptr(vertex_map), stream),
                        "nf_mesh_decimate_emit")

            count()
            got = counts.tolist()
            found["v"], found["f"] = got[0], got[1]
            assert got[7] == 0
            ms = timed({"count": count, "emit": emit, "python": lambda: ops.decimate_mesh(verts, faces, norm, cell=size, origin=origin),
                        "adjacency": adjacency})
            both = [x + y for x, y in zip(ms["count"], ms["emit"])]
            py = ops.decimate_mesh(verts, faces, norm, cell=size, origin=origin)
            same = torch.equal(py[0].view(torch.int32), out_v[:got[0]].view(torch.int32)) and torch.equal(py[1], out_f[:got[1]]) and \
                torch.equal(py[3], vertex_map)
            lines.append(f"| {n}^3 | {n_v} | {n_f} | {'one cell' if k is None else f'{k:g}'} | {got[0]} | {got[1]} | {got[6]} | {cell(ms['count'])} | "
                         f"{cell(ms['emit'])} | {cell(both)} | {cell(ms['python'])} | {cell(ms['adjacency'])}{'' if same else ' (OUTPUTS DIFFER)'} |")
        del ws, ms_ws, row_start, neighbours, multiplicity, boundary, out_v, out_f, vertex_map, verts, faces, norm
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
