"""Time the mesh clean-up (connected components, keep the largest) beside the isosurface extraction that feeds it -- same GPU, same
process, same grid.  Writes profiles/mesh_components.md (and prints it).

    python tools/time_mesh_components.py [--sizes 128 256 512] [--repeats 7] [--warmup 2] [--out profiles/mesh_components.md]

Per grid size N^3 and field: nf_mesh_components_label on preallocated buffers, nf_mesh_components_select + _emit (largest, with
normals) on preallocated outputs, ops.filter_mesh as a user calls it (allocations and the one host read included) and ops.isosurface
of the same grid.  Fields: `sphere`, r^2 - |p|^2 with r = 0.7 on [-1, 1]^3 (the field of profiles/isosurface.md), one component; and
`floaters`, the same sphere plus N^3 / 4096 seeded single grid points lifted above the level outside it, each a speck of 14 vertices
and 24 faces (a few touch and merge).  The launches of a row alternate inside one loop with device events around each; the figure is
the median, the spread min .. max.  The yardstick is the isosurface's: a mesh step stays below 5 % of the f16x2 density evaluation of
the same grid, whose medians are taken from profiles/isosurface.md.
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


def fields(n, dev):
    ax = torch.linspace(-1.0, 1.0, n, device=dev)
    sphere = (0.49 - (ax.view(1, 1, n) ** 2 + ax.view(1, n, 1) ** 2 + ax.view(n, 1, 1) ** 2)).contiguous()
    g = torch.Generator().manual_seed(n)
    picks = torch.randint(0, n ** 3, (n ** 3 // 4096,), generator=g).to(dev)
    inner = torch.zeros(n, dtype=torch.bool, device=dev)
    inner[2:n - 2] = True                                                  # specks stay clear of the box faces: closed components
    ok = (sphere.view(-1)[picks] < -0.1) & inner[picks % n] & inner[(picks // n) % n] & inner[picks // (n * n)]
    floaters = sphere.clone()
    floaters.view(-1)[picks[ok]] = 0.05
    return {"sphere": sphere, "floaters": floaters}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_components.md"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_components.py measures on a ROCm device; none is visible")
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
    lines = ["# Mesh components and filtering: measured", "",
             f"Command: `python tools/time_mesh_components.py --sizes {' '.join(map(str, a.sizes))} --repeats {a.repeats} --warmup {a.warmup}`", "",
             f"Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}.  One process; the launches of a row alternate in "
             f"one loop; device events around each; median of {a.repeats} after {a.warmup} warm-up rounds (min .. max in brackets), milliseconds.  "
             "Meshes: ops.isosurface (normals on) of `sphere`, r^2 - |p|^2 with r = 0.7 on [-1, 1]^3 at level 0, and of `floaters`, that sphere "
             "plus N^3 / 4096 seeded single grid points above the level outside it.  `label`: nf_mesh_components_label (six kernels) on "
             "preallocated buffers; `select + emit`: nf_mesh_components_select and _emit (five kernels), rule largest, normals copied, on "
             "preallocated outputs; `ops.filter_mesh`: the three with their allocations and their one host read; `bound`: 5 % of the f16x2 "
             "density evaluation of the same grid (profiles/isosurface.md).", "",
             "| grid | field | V | F | C | kept V | kept F | label, ms | select + emit, ms | label + select + emit, ms | ops.filter_mesh, ms | "
             "ops.isosurface, ms | bound, ms | below the bound |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in a.sizes:
        for name, field in fields(n, dev).items():
            verts, faces, norm = ops.isosurface(field, 0.0, lo, hi, normals=True)
            n_v, n_f = verts.shape[0], faces.shape[0]
            ws_bytes = int(lib.nf_mesh_components_workspace_bytes(n_v, n_f))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            counts = torch.empty(4, dtype=torch.int64, device=dev)
            i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
            vertex_label, face_label, face_counts, vertex_counts = i32(n_v), i32(n_f), i32(n_v), i32(n_v)

            def label():
                H.check(lib.nf_mesh_components_label(H.ptr(faces), n_v, n_f, H.ptr(ws), ws_bytes, H.ptr(vertex_label), H.ptr(face_label),
                                                     H.ptr(face_counts), H.ptr(vertex_counts), H.ptr(counts), stream), "nf_mesh_components_label")

            def select():
                H.check(lib.nf_mesh_components_select(H.ptr(vertex_label), H.ptr(face_label), H.ptr(face_counts), n_v, n_f, 1, 0, H.ptr(ws), ws_bytes,
                                                      H.ptr(counts), stream), "nf_mesh_components_select")

            label()
            select()
            n_c, kept_v, kept_f, _ = counts.tolist()
            out_v, out_n = torch.empty((kept_v, 3), device=dev), torch.empty((kept_v, 3), device=dev)
            out_f = torch.empty((kept_f, 3), dtype=torch.int32, device=dev)

            def select_emit():
                select()
                H.check(lib.nf_mesh_components_emit(H.ptr(verts), H.ptr(faces), H.ptr(norm), H.ptr(vertex_label), H.ptr(face_label), H.ptr(face_counts),
                                                    n_v, n_f, H.ptr(ws), ws_bytes, H.ptr(out_v), kept_v, H.ptr(out_f), kept_f, H.ptr(out_n), stream),
                        "nf_mesh_components_emit")

            ms = timed({"label": label, "select_emit": select_emit, "python": lambda: ops.filter_mesh(verts, faces, norm, largest=True),
                        "isosurface": lambda: ops.isosurface(field, 0.0, lo, hi, normals=True)})
            same = all(torch.equal(x.view(torch.int32), y.view(torch.int32))
                       for x, y in zip(ops.filter_mesh(verts, faces, norm, largest=True)[:3], (out_v, out_f, out_n)))
            both = [x + y for x, y in zip(ms["label"], ms["select_emit"])]
            bound = 0.05 * DENSITY_F16X2_MS[n] if n in DENSITY_F16X2_MS else None
            verdict = "n/a" if bound is None else ("yes" if statistics.median(both) <= bound else "NO")
            lines.append(f"| {n}^3 | {name} | {n_v} | {n_f} | {n_c} | {kept_v} | {kept_f} | {cell(ms['label'])} | {cell(ms['select_emit'])} | {cell(both)} | "
                         f"{cell(ms['python'])} | {cell(ms['isosurface'])} | {'n/a' if bound is None else f'{bound:.2f}'} | "
                         f"{verdict}{'' if same else ' (OUTPUTS DIFFER)'} |")
            del ws, vertex_label, face_label, face_counts, vertex_counts, out_v, out_f, out_n, verts, faces, norm
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
