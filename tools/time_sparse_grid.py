"""Time mesh extraction through a sparse density grid beside the dense path it leaves untouched -- same GPU, same process, same grid.
Writes profiles/sparse_grid.md (and prints it).

    python tools/time_sparse_grid.py [--sizes 256 512] [--bricks 8 16] [--repeats 5] [--warmup 1] [--out profiles/sparse_grid.md]

Two fields per grid size N^3 and precision ("f32", "f16x2"):
  model   the paper model at its default initialisation (the model of tools/time_isosurface.py) on [-0.4, 0.4]^3, level = the median
          of its dense grid: nerf.extract_mesh as a user calls it, dense (brick=None) and sparse.  An untrained field crosses its
          median almost everywhere: nearly every brick is active, so there is next to nothing to gain, and it breaks the
          precondition of the guarantee (bricks whose corners agree still hold crossings), so the meshes differ.
  sphere  the surface of profiles/isosurface.md (r^2 - |p|^2, r = 0.7, on [-1, 1]^3, level 0) at the NETWORK'S cost: the function is
          sphere(p) + 0 * density(model, p / 2.5), so every point that is asked for costs one network evaluation and the geometry
          is a closed surface, as a trained model's is.  dense: the function on every point (in slabs, as nerf.density_grid), then
          ops.isosurface; sparse: ops.sparse_grid, then ops.isosurface.  The meshes are compared (torch.equal).
`new kernels`: the entry points of csrc/nf_sparse_grid.hip alone on the sphere's grid (lattice, scatter, classify, mark, emit,
scatter) with preallocated buffers and no host read, as a fraction of the dense f32 density time at the same size.  The launches of
a row alternate inside one loop with device events around each; the figure is the median, the spread min .. max.
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--bricks", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_grid.md"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("time_sparse_grid.py measures on a ROCm device; none is visible")
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
    s_lo, s_hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    m_lo, m_hi = (-0.4, -0.4, -0.4), (0.4, 0.4, 0.4)                    # the density is timed where the model's test points lie
    c_lo, c_hi = (ctypes.c_float * 3)(*s_lo), (ctypes.c_float * 3)(*s_hi)

    def sphere(pts):
        return 0.49 - (pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1] + pts[:, 2] * pts[:, 2])

    def sphere_at_network_cost(pts):
        with torch.no_grad():
            return sphere(pts) + 0.0 * nerf.density(model, pts / 2.5, expr, latent)

    def dense_sphere(n, chunk_points=1 << 22):
        """sphere_at_network_cost on every grid point, in slabs of z planes as nerf.density_grid evaluates."""
        xs, ys, zs = (torch.from_numpy(x).to(dev) for x in nerf.mesh.grid_axes(s_lo, s_hi, n))
        planes = max(1, chunk_points // (n * n))
        out = torch.empty((n, n, n), dtype=torch.float32, device=dev)
        for k0 in range(0, n, planes):
            shape = (min(n, k0 + planes) - k0, n, n)
            pts = torch.stack([xs.view(1, 1, n).expand(shape), ys.view(1, n, 1).expand(shape), zs[k0:k0 + shape[0]].view(-1, 1, 1).expand(shape)], dim=-1)
            out[k0:k0 + shape[0]] = sphere_at_network_cost(pts.reshape(-1, 3)).view(shape)
        return out

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
        return f"{statistics.median(v):.2f} ({min(v):.2f} .. {max(v):.2f})"

    def in_precision(precision, f):
        def run():
            nerf.set_mlp_precision(precision)
            try:
                return f()
            finally:
                nerf.set_mlp_precision("f32")
        return run

    def kernels_alone(n, brick):
        """The six launches on preallocated buffers; the values that stand for the function's answers are read from the dense sphere."""
        xs = torch.from_numpy(nerf.mesh.grid_axes(s_lo, s_hi, n)[0]).to(dev)
        field = (0.49 - (xs.view(1, 1, n) ** 2 + xs.view(1, n, 1) ** 2 + xs.view(n, 1, 1) ** 2)).contiguous().view(-1)
        m = -(-(n - 1) // brick)
        n_lattice = (m + 1) ** 3
        ws_bytes = int(lib.nf_sparse_grid_workspace_bytes(n, n, n, brick))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        grid = torch.empty(n ** 3, dtype=torch.float32, device=dev)
        counts = torch.empty(3, dtype=torch.int64, device=dev)
        l_index, l_coords = torch.empty(n_lattice, dtype=torch.int32, device=dev), torch.empty((n_lattice, 3), device=dev)
        lo_p, hi_p = ctypes.addressof(c_lo), ctypes.addressof(c_hi)
        state = {}

        def front():
            H.check(lib.nf_sparse_grid_lattice(n, n, n, brick, lo_p, hi_p, H.ptr(l_index), H.ptr(l_coords), n_lattice, stream), "lattice")
            if "l_values" not in state:
                state["l_values"] = field[l_index.long()].contiguous()
            H.check(lib.nf_sparse_grid_scatter(H.ptr(state["l_values"]), H.ptr(l_index), n_lattice, H.ptr(grid), n, n, n, stream), "scatter")
            H.check(lib.nf_sparse_grid_classify(H.ptr(grid), n, n, n, brick, 0.0, 0.0, 1, H.ptr(ws), ws_bytes, stream), "classify")
            H.check(lib.nf_sparse_grid_mark(n, n, n, brick, H.ptr(ws), ws_bytes, H.ptr(counts), stream), "mark")

        front()
        n_more = int(counts[2])
        index, coords = torch.empty(n_more, dtype=torch.int32, device=dev), torch.empty((n_more, 3), device=dev)

        def back():
            H.check(lib.nf_sparse_grid_emit(H.ptr(grid), n, n, n, brick, lo_p, hi_p, H.ptr(ws), ws_bytes, H.ptr(index), H.ptr(coords), n_more, stream),
                    "emit")
            if "values" not in state:
                state["values"] = field[index.long()].contiguous()
            H.check(lib.nf_sparse_grid_scatter(H.ptr(state["values"]), H.ptr(index), n_more, H.ptr(grid), n, n, n, stream), "scatter")

        back()
        return lambda: (front(), back())

    props = torch.cuda.get_device_properties(dev)
    lines = ["# Sparse density grids: measured", "",
             f"Command: `python tools/time_sparse_grid.py --sizes {' '.join(map(str, a.sizes))} --bricks {' '.join(map(str, a.bricks))} "
             f"--repeats {a.repeats} --warmup {a.warmup}`", "",
             f"Device: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}.  One process; the launches of a row alternate in "
             f"one loop; device events around each; median of {a.repeats} after {a.warmup} warm-up rounds (min .. max in brackets), milliseconds.  "
             "`dense`: the path this change leaves untouched (every grid point evaluated, then ops.isosurface), the baseline.  `sparse`: the same "
             "call with `brick`, margin 0, dilate 1, its allocations and its host read included.  `model`: nerf.extract_mesh of the paper model "
             "(default initialisation) on [-0.4, 0.4]^3 at the median of its dense grid -- an untrained field crosses that level almost "
             "everywhere: nearly every brick is active, so there is next to nothing to gain, and `same mesh` is NO because such a field "
             "breaks the precondition of the guarantee (bricks whose corners agree still hold crossings; DESIGN.md \"Sparse density grid\").  `sphere`: r^2 - |p|^2, r = 0.7, on [-1, 1]^3, level 0, evaluated at the "
             "network's cost (sphere(p) + 0 * density(model, p / 2.5)): a closed surface, as a trained model's is.  `new kernels`: the "
             "entry points of csrc/nf_sparse_grid.hip alone on the sphere's grid, preallocated buffers, no host read; the last column sets "
             "them against the dense f32 density of the model at the same size.", "",
             "| grid | field | precision | brick | dense, ms | sparse, ms | dense / sparse | active bricks | evaluated points | same mesh | "
             "new kernels, ms | dense f32 density, ms | new kernels / dense f32 density |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in a.sizes:
        density_ms = statistics.median(timed({"d": lambda: nerf.density_grid(model, expr, latent, lo=m_lo, hi=m_hi, resolution=n)})["d"])
        level = float(nerf.density_grid(model, expr, latent, lo=m_lo, hi=m_hi, resolution=n).flatten()[::7].median())
        kernel_ms = {b: timed({"k": kernels_alone(n, b)})["k"] for b in a.bricks}
        for field in ("model", "sphere"):
            for precision in ("f32", "f16x2"):
                if field == "model":
                    box = dict(lo=m_lo, hi=m_hi, resolution=n, level=level)
                    dense = in_precision(precision, lambda: nerf.extract_mesh(model, expr, latent, **box))
                    sparse = {b: in_precision(precision, lambda b=b: nerf.extract_mesh(model, expr, latent, brick=b, **box)) for b in a.bricks}
                    stats = {b: in_precision(precision, lambda b=b: nerf.density_grid_sparse(model, expr, latent, brick=b, **box)[1])() for b in a.bricks}
                else:
                    dense = in_precision(precision, lambda: ops.isosurface(dense_sphere(n), 0.0, s_lo, s_hi, normals=True))
                    sparse = {b: in_precision(precision, lambda b=b: ops.isosurface(ops.sparse_grid(sphere_at_network_cost, 0.0, s_lo, s_hi, n, brick=b)[0],
                                                                                   0.0, s_lo, s_hi, normals=True)) for b in a.bricks}
                    stats = {b: in_precision(precision, lambda b=b: ops.sparse_grid(sphere_at_network_cost, 0.0, s_lo, s_hi, n, brick=b)[1])() for b in a.bricks}
                ms = timed({"dense": dense, **{f"b{b}": f for b, f in sparse.items()}})
                want = dense()
                d = statistics.median(ms["dense"])
                for b in a.bricks:
                    same = all(torch.equal(x, y) for x, y in zip(want, sparse[b]()))
                    st, s, k = stats[b], statistics.median(ms[f"b{b}"]), statistics.median(kernel_ms[b])
                    lines.append(f"| {n}^3 | {field} | {precision} | {b} | {cell(ms['dense'])} | {cell(ms[f'b{b}'])} | {d / s:.2f} x | "
                                 f"{100.0 * st.active_bricks / st.bricks:.1f} % | {100.0 * st.evaluated_points / st.points:.1f} % | "
                                 f"{'yes' if same else 'NO'} | {cell(kernel_ms[b])} | {density_ms:.2f} | {100.0 * k / density_ms:.2f} % |")
                del want
                torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
