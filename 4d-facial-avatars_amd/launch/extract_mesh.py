"""Triangle mesh of a trained model's density surface for one test frame: the expression and latent code of frame I (picked as
launch/eval_sharded.py picks them), the raw density on a dense grid (nerf.density_grid) and the surface of one level
(ops.isosurface), written as .ply / .obj / .off.  Single rank.

    python -m launch.extract_mesh --config cfg.yml --checkpoint ck --frame I --level L --resolution N [Ny Nz] --out mesh.ply \
        [--bounds x0 y0 z0 x1 y1 z1] [--precision f32|f16x3|f16x2|bf16x3] [--coarse] [--brick B [--margin M] [--dilate D]] \
        [--largest | --min-faces N] [--smooth N [--smooth-lambda L] [--smooth-mu M]] [--decimate K] \
        [--colour [--colour-samples K] [--colour-depth D] [--colour-view-z Z]]

Without --bounds the box is the axis-aligned hull of the frame's camera frustum between the config's near and far planes (the
four image-corner rays of nerf.get_ray_bundle).  --level is in raw-density units (before the renderer's ReLU) and has no default.
With --brick B the network is evaluated only in the bricks of B cells near the surface (nerf.density_grid_sparse): first on the
brick corners, then in every brick whose corners are not all on one side of the level by more than --margin, and in the bricks
within --dilate bricks of those.  A feature thinner than a brick that passes between the corners is missed unless the margin is raised.
--largest keeps the connected component with the most faces, --min-faces N every component with at least N faces (nerf.filter_mesh,
on the device): a trained model's floaters are small components of their own.  --smooth N runs N iterations of Taubin's lambda | mu
smoothing on what is left (nerf.smooth_mesh, on the device; the border a box cuts into the surface stays where it is) and writes
the normals of the smoothed faces in place of the density gradient's.  --decimate K then clusters the vertices on cells of K grid
cells from the box's corner (nerf.decimate_mesh, on the device): the vertices of one cell become one, faces that lose a corner go,
coincident faces are welded; extract fine, clean and smooth, then reduce to the size a viewer takes.  --colour writes a colour per
vertex of that final mesh
(nerf.vertex_colours, from the same network as the density): K samples (default 8) on a ray along the normal through a shell of
half-thickness D round the surface (default: the diagonal of a grid cell, or of a decimation cell under --decimate K with K > 1),
composited and normalised, seen from the frame's camera (its pose and the config's near / far), or with the view direction
(0, 0, Z) under --colour-view-z.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from . import common as CM
from .common import nerf
from nerf import ops


def frustum_box(height: int, width: int, intrinsics, pose, near: float, far: float):
    """(lo, hi): hull of the points o + d * near and o + d * far of the four image-corner rays."""
    ro, rd = nerf.get_ray_bundle(height, width, intrinsics, pose)
    o, d = (t[[0, 0, -1, -1], [0, -1, 0, -1]].double().cpu() for t in (ro, rd))
    pts = torch.cat([o + d * near, o + d * far])
    return pts.min(dim=0).values.tolist(), pts.max(dim=0).values.tolist()


def main(argv=None):
    keep = nerf.get_mlp_precision()          # the precision switch is process-global: leave it as the caller had it
    try:
        return _main(argv)
    finally:
        nerf.set_mlp_precision(keep)


def _main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--checkpoint", type=str, required=True)
    ap.add_argument("--frame", type=int, required=True, help="test frame whose expression, latent code (and, without --bounds, camera) are used")
    ap.add_argument("--level", type=float, required=True, help="raw density of the surface (before the renderer's ReLU)")
    ap.add_argument("--resolution", type=int, nargs="+", required=True, metavar="N", help="grid points per axis: N, or Nx Ny Nz")
    ap.add_argument("--out", type=str, required=True, help="mesh file: .ply (binary), .obj or .off")
    ap.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--precision", choices=["f32", "f16x3", "f16x2", "bf16x3"], default="f32")
    ap.add_argument("--coarse", action="store_true", help="the coarse network's density (default: the fine network's, when the checkpoint has one)")
    ap.add_argument("--brick", type=int, default=None, metavar="B", help="evaluate the density only in bricks of B cells near the surface (default: every point)")
    ap.add_argument("--margin", type=float, default=0.0, metavar="M", help="with --brick: corners within M of the level make their bricks seeds")
    ap.add_argument("--dilate", type=int, default=1, metavar="D", help="with --brick: also evaluate the bricks within D bricks of a seed (the normals need 1)")
    rule = ap.add_mutually_exclusive_group()
    rule.add_argument("--largest", action="store_true", help="keep only the connected component with the most faces")
    rule.add_argument("--min-faces", type=int, default=None, metavar="N", help="keep only the connected components with at least N faces")
    ap.add_argument("--smooth", type=int, default=0, metavar="N", help="iterations of Taubin smoothing after the component filter (default: none)")
    ap.add_argument("--smooth-lambda", type=float, default=0.5, metavar="L", help="with --smooth: the shrinking factor, 0 < L <= 1")
    ap.add_argument("--smooth-mu", type=float, default=-0.53, metavar="M", help="with --smooth: the inflating factor, -1 <= M <= 0 (0: plain Laplacian smoothing)")
    ap.add_argument("--decimate", type=float, default=None, metavar="K", help="cluster the vertices on cells of K grid cells, K > 0, after --smooth and before "
                    "--colour (default: no decimation)")
    ap.add_argument("--colour", action="store_true", help="write a colour per vertex of the final mesh, from the same network as the density")
    ap.add_argument("--colour-samples", type=int, default=8, metavar="K", help="with --colour: samples on the ray through every vertex, 1 .. 64")
    ap.add_argument("--colour-depth", type=float, default=None, metavar="D", help="with --colour: half-thickness of the sampled shell (default: a grid cell's diagonal; with "
                    "--decimate K > 1 a decimation cell's, which is how far the true surface can lie from a clustered vertex)")
    ap.add_argument("--colour-view-z", type=float, default=None, metavar="Z", help="with --colour: the view direction (0, 0, Z) in place of the frame's camera")
    args = ap.parse_args(argv)
    if len(args.resolution) not in (1, 3):
        ap.error("--resolution takes one number or three")
    if os.path.splitext(args.out)[1].lower() not in (".ply", ".obj", ".off"):
        ap.error("--out: the extension names the format (.ply, .obj or .off)")
    if args.brick is not None and (args.brick < 2 or not args.margin >= 0.0 or args.dilate < 1):
        ap.error("--brick takes at least 2 cells, --margin at least 0 and --dilate at least 1 (the mesh is written with normals)")
    if args.min_faces is not None and args.min_faces < 1:
        ap.error("--min-faces takes at least 1")
    if args.smooth < 0 or not 0.0 < args.smooth_lambda <= 1.0 or not -1.0 <= args.smooth_mu <= 0.0:
        ap.error("--smooth takes at least 0 iterations, --smooth-lambda a factor in (0, 1] and --smooth-mu one in [-1, 0]")
    if args.decimate is not None and not 0.0 < args.decimate < float("inf"):
        ap.error("--decimate takes a number of grid cells above 0")
    if not 1 <= args.colour_samples <= ops.MESH_COLOUR_MAX_SAMPLES or (args.colour_depth is not None and not args.colour_depth >= 0.0):
        ap.error(f"--colour-samples takes 1 to {ops.MESH_COLOUR_MAX_SAMPLES} samples and --colour-depth at least 0")
    if not torch.cuda.is_available():
        raise SystemExit("the MI355X `nerf` package needs a ROCm device")
    dev = torch.device("cuda", torch.cuda.current_device())
    nerf.set_mlp_precision(args.precision)
    cfg = CM.load_config(args.config)
    _, poses, _, hwf, _, expressions, _, _ = nerf.load_flame_data(cfg.dataset.basedir, half_res=cfg.dataset.half_res,
                                                                  testskip=cfg.dataset.testskip, test=True)
    if not 0 <= args.frame < poses.shape[0]:
        raise SystemExit(f"--frame {args.frame}: the test sequence has {poses.shape[0]} frames")
    model_c, model_f = CM.build_models(cfg, dev)
    ck = torch.load(args.checkpoint, map_location=dev)
    model_c.load_state_dict(ck["model_coarse_state_dict"])
    has_fine = bool(ck.get("model_fine_state_dict")) and model_f is not None
    if has_fine:
        model_f.load_state_dict(ck["model_fine_state_dict"])
    model = model_c if args.coarse or not has_fine else model_f
    model.eval()
    H, W = int(ck.get("height", hwf[0])), int(ck.get("width", hwf[1]))
    latent_codes = ck.get("latent_codes")
    latent_codes = latent_codes.to(dev) if latent_codes is not None else torch.zeros(1, 32, device=dev)
    row = 0
    p = os.path.join(cfg.dataset.basedir, "index_map.npy")
    if os.path.exists(p):
        idx_map = np.load(p).astype(int)
        row = int(idx_map[args.frame, 1]) if args.frame < len(idx_map) else 0
    latent = latent_codes[min(max(row, 0), latent_codes.shape[0] - 1)]
    expr = expressions[args.frame].float().to(dev)
    if args.bounds is not None:
        lo, hi = args.bounds[:3], args.bounds[3:]
    else:
        lo, hi = frustum_box(H, W, hwf[2], poses[args.frame, :3, :4].float().to(dev), float(cfg.dataset.near), float(cfg.dataset.far))
    res = args.resolution * 3 if len(args.resolution) == 1 else args.resolution
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    sparse = None
    if args.brick is None:
        grid = nerf.density_grid(model, expr, latent, lo=lo, hi=hi, resolution=res)
    else:
        grid, sparse = nerf.density_grid_sparse(model, expr, latent, lo=lo, hi=hi, resolution=res, level=args.level, brick=args.brick,
                                                margin=args.margin, dilate=args.dilate)
    ev[1].record()
    mesh = nerf.Mesh(*ops.isosurface(grid, args.level, lo, hi, normals=True))
    ev[2].record()
    clean = None
    if args.largest or args.min_faces is not None:
        *kept, clean = ops.filter_mesh(*mesh, largest=args.largest, min_faces=args.min_faces)
        mesh = nerf.Mesh(*kept)
    smooth = None
    if args.smooth:
        n_smoothed = int(mesh.vertices.shape[0])
        *smoothed, smooth = ops.smooth_mesh(*mesh, iterations=args.smooth, lam=args.smooth_lambda, mu=args.smooth_mu)
        mesh = nerf.Mesh(*smoothed)
    decimate = None
    if args.decimate is not None:
        cell, origin = nerf.mesh.decimation_lattice(lo, hi, res, args.decimate)
        *lighter, _, decimate = ops.decimate_mesh(*mesh, cell=cell, origin=origin)
        mesh = nerf.Mesh(*lighter)
    colour = None
    if args.colour:
        cell = [max(args.decimate or 1.0, 1.0) * (float(h) - float(l)) / (int(n) - 1) for l, h, n in zip(lo, hi, res)]
        depth = args.colour_depth if args.colour_depth is not None else float(np.sqrt(sum(c * c for c in cell)))
        view = dict(view_z=args.colour_view_z) if args.colour_view_z is not None else dict(pose=poses[args.frame, :3, :4].float().to(dev))
        min_opacity = 1e-3
        colours = nerf.vertex_colours(model, mesh, expr, latent, near=float(cfg.dataset.near), far=float(cfg.dataset.far), samples=args.colour_samples,
                                      depth=depth, min_opacity=min_opacity, **view)
        colour = {"vertices": int(mesh.vertices.shape[0]), "samples": args.colour_samples, "depth": depth, "min_opacity": min_opacity,
                  "below_min_opacity": int((~(colours.opacity >= min_opacity)).sum().item())}       # the one host read
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if colour is None:
        nerf.write_mesh(args.out, mesh)
    else:
        nerf.write_mesh(args.out, mesh, colours=colours.colours)
    stats = {"lo": [float(x) for x in lo], "hi": [float(x) for x in hi], "resolution": [int(r) for r in res], "vertices": int(mesh.vertices.shape[0]),
             "faces": int(mesh.faces.shape[0]), "density_s": ev[0].elapsed_time(ev[1]) * 1e-3, "extract_s": ev[1].elapsed_time(ev[2]) * 1e-3,
             "network": "coarse" if model is model_c else "fine", "out": args.out}
    print(f"frame {args.frame} ({stats['network']} network, {args.precision}): box lo {stats['lo']} hi {stats['hi']}, grid {stats['resolution']}, "
          f"level {args.level}: V = {stats['vertices']}, F = {stats['faces']}; density {stats['density_s']:.4f} s, extraction {stats['extract_s']:.4f} s "
          f"-> {args.out}")
    if clean is not None:
        stats["components"] = clean._asdict()
        print(f"{'largest component' if args.largest else f'components of at least {args.min_faces} faces'}: {clean.components} components, "
              f"{clean.kept_components} kept; vertices {clean.kept_vertices} of {clean.vertices}, faces {clean.kept_faces} of {clean.faces}")
    if smooth is not None:
        stats["smooth"] = smooth._asdict()
        print(f"smoothed: {args.smooth} iterations (lambda {args.smooth_lambda}, mu {args.smooth_mu}) in {smooth.passes} passes over {smooth.edges // 2} edges; "
              f"{smooth.pinned_vertices} boundary vertices of {n_smoothed} stay where they are")
    if decimate is not None:
        stats["decimate"] = decimate._asdict()
        print(f"decimated: cells of {args.decimate:g} grid cells; vertices {decimate.kept_vertices} of {decimate.vertices}, faces {decimate.kept_faces} of "
              f"{decimate.faces} ({decimate.degenerate_faces} degenerate, {decimate.coincident_faces} coincident); the largest cluster holds "
              f"{decimate.largest_cluster} vertices")
    if colour is not None:
        stats["colour"] = colour
        print(f"coloured: {colour['vertices']} vertices, {colour['samples']} samples over a shell of half-thickness {colour['depth']:.6g}; "
              f"{colour['below_min_opacity']} vertices below opacity {colour['min_opacity']:g} take the colour of the sample at the vertex")
    if sparse is not None:
        stats["sparse"] = sparse._asdict()
        print(f"bricks of {args.brick} cells (margin {args.margin}, dilate {args.dilate}): {sparse.seed_bricks} seed and {sparse.active_bricks} active of "
              f"{sparse.bricks} bricks; density evaluated on {sparse.evaluated_points} of {sparse.points} points "
              f"({100.0 * sparse.evaluated_points / sparse.points:.1f} %)")
    if (stats["faces"] if clean is None else clean.faces) == 0:
        seen = grid if sparse is None else grid[torch.isfinite(grid)]       # a sparse grid holds +-inf where nothing was evaluated
        lo_v, hi_v = seen.min().item(), seen.max().item()
        print(f"no surface at level {args.level}: the raw density on this grid spans [{lo_v:.4g}, {hi_v:.4g}]")
    return stats


if __name__ == "__main__":
    main()
