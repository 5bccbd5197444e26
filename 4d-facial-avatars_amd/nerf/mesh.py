"""Geometry of a fused model: its raw density on a dense grid, the triangle mesh of one density level, and mesh files.

    density_grid(model, expr, latent_code, lo=, hi=, resolution=)          -> (nz, ny, nx) raw density on the device
    density_grid_sparse(..., lo=, hi=, resolution=, level=, brick=)        -> the same grid evaluated near the surface only, and its stats
    extract_mesh(model, expr, latent_code, lo=, hi=, resolution=, level=)  -> Mesh(vertices, faces, normals), device tensors
    mesh_components(mesh)                                                  -> MeshComponents: labels and counts of the connected components
    filter_mesh(mesh, largest= | min_faces=)                               -> the Mesh of the largest component, or of those of >= N faces
    smooth_mesh(mesh, iterations=, lam=, mu=, fix_boundary=)               -> the Mesh after Taubin smoothing, its normals recomputed
    vertex_normals(mesh)                                                   -> (V, 3) unit normals from the faces
    decimate_mesh(mesh, cell=, origin=)                                    -> the lighter Mesh of vertex clustering on a lattice of `cell`
    vertex_colours(model, mesh, expr, latent_code, near=, far=, pose= | view_z=, samples=, depth=)
                                                                           -> MeshColours(colours (V, 3) in [0, 1], opacity (V,))
    write_mesh(path, mesh, colours=None)                                   -> .off / .obj / .ply (binary little-endian), host code

The density comes from the density-only kernels (nerf.density), the surface from ops.isosurface (csrc/nf_isosurface.hip), the choice
of the points near the surface from ops.sparse_grid (csrc/nf_sparse_grid.hip), the components from ops.mesh_components and
ops.filter_mesh (csrc/nf_mesh_components.hip), smoothing and face normals from ops.smooth_mesh and ops.vertex_normals
(csrc/nf_mesh_smooth.hip), decimation from ops.decimate_mesh (csrc/nf_mesh_decimate.hip).  The colours come from the model's full forward (the network nerf.radiance queries) on a short ray through
the surface at every vertex, along the normal, composited and normalised by ops.mesh_colour_rays and ops.mesh_colour_integrate
(csrc/nf_mesh_colour.hip; DESIGN.md "Mesh colours"); write_mesh stores them per vertex in each of its three formats.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops
from .models import _point_query, density
from .ops import MeshColours


class Mesh(NamedTuple):
    vertices: torch.Tensor                       # (V, 3) float32
    faces: torch.Tensor                          # (F, 3) int32, counter-clockwise seen from outside (lower density)
    normals: Optional[torch.Tensor]              # (V, 3) float32 unit vectors towards lower density, or None


_resolution = ops._resolution


def grid_axes(lo, hi, resolution):
    """The coordinates of the grid points per axis, float32: lo + i * h with h = (hi - lo) / (n - 1), multiply then add -- the
    positions ops.isosurface gives the same grid points."""
    lo32, hi32 = ops._box(lo, hi, "density_grid")
    return [lo32[a] + np.arange(n, dtype=np.float32) * ((hi32[a] - lo32[a]) / np.float32(n - 1)) for a, n in enumerate(_resolution(resolution))]


def density_grid(model, expr, latent_code=None, *, lo, hi, resolution, chunk_points: int = 1 << 22):
    """Raw density (nz, ny, nx) of a fused model on the grid of `resolution` (one number or (nx, ny, nz)) points spanning the box
    [lo, hi], x fastest, for one expression (and latent code), in the arithmetic of nerf.set_mlp_precision.  Evaluated through
    nerf.density in slabs of whole z planes of at most `chunk_points` points (at least one plane), so it carries that function's
    guards and equals it bit for bit on the same points.  Runs under torch.no_grad()."""
    if not (torch.is_tensor(expr) and expr.is_cuda):
        raise RuntimeError("nerf (MI355X build): tensors must live on a ROCm device (`device='cuda'`); there is no CPU path in this package")
    nx, ny, nz = _resolution(resolution)
    dev = expr.device
    xs, ys, zs = (torch.from_numpy(a).to(dev) for a in grid_axes(lo, hi, (nx, ny, nz)))
    planes = max(1, int(chunk_points) // (nx * ny))
    out = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
    with torch.no_grad():
        for k0 in range(0, nz, planes):
            k1 = min(nz, k0 + planes)
            shape = (k1 - k0, ny, nx)
            pts = torch.stack([xs.view(1, 1, nx).expand(shape), ys.view(1, ny, 1).expand(shape), zs[k0:k1].view(-1, 1, 1).expand(shape)], dim=-1)
            out[k0:k1] = density(model, pts.reshape(-1, 3), expr, latent_code).view(shape)
    return out


def density_grid_sparse(model, expr, latent_code=None, *, lo, hi, resolution, level, brick: int = 8, margin: float = 0.0, dilate: int = 1,
                        chunk_points: int = 1 << 22):
    """density_grid evaluated only near the surface raw density == level: ops.sparse_grid with nerf.density of the model as its
    function, under torch.no_grad().  Returns (grid, SparseGridStats): on the coarse lattice (the corners of the bricks of `brick`
    cells) and in the active bricks the grid equals density_grid bit for bit, every other point holds +inf or -inf, the side of its
    bricks' corners.  A brick is evaluated when its 8 corners are not all above level + margin or all below level - margin, or when
    it lies within `dilate` bricks of such a brick: a feature thinner than a brick that passes between the corners is missed unless
    `margin` is raised (ops.sparse_grid has the guarantee and its limit)."""
    if not (torch.is_tensor(expr) and expr.is_cuda):
        raise RuntimeError("nerf (MI355X build): tensors must live on a ROCm device (`device='cuda'`); there is no CPU path in this package")
    with torch.no_grad():
        return ops.sparse_grid(lambda pts: density(model, pts, expr, latent_code), float(level), lo, hi, resolution, brick=brick, margin=margin,
                               dilate=dilate, chunk_points=chunk_points, device=expr.device)


def _mesh_fields(mesh, what: str):
    fields = tuple(mesh)
    if len(fields) not in (2, 3):
        raise ValueError(f"{what}: expected Mesh(vertices, faces, normals) or a (vertices, faces[, normals]) tuple")
    return (fields + (None,))[:3]


def mesh_components(mesh) -> ops.MeshComponents:
    """Connected components of a Mesh (or a (vertices, faces[, normals]) tuple) on the device: ops.mesh_components of its faces over
    its vertices -- MeshComponents(vertex_label, face_label, face_counts, vertex_counts), numbered by ascending smallest vertex id."""
    vertices, faces, _ = _mesh_fields(mesh, "mesh_components")
    if not torch.is_tensor(vertices) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("mesh_components: vertices must be a tensor of shape (V, 3)")
    return ops.mesh_components(faces, vertices.shape[0])


def filter_mesh(mesh, *, largest: bool = False, min_faces=None) -> Mesh:
    """The Mesh of the components one rule keeps (ops.filter_mesh): largest=True, the component with the most faces, or min_faces=N,
    every component with at least N faces -- a trained model's floaters are small components.  Order and bits of what is kept stay."""
    vertices, faces, normals = _mesh_fields(mesh, "filter_mesh")
    return Mesh(*ops.filter_mesh(vertices, faces, normals, largest=largest, min_faces=min_faces)[:3])


def smooth_mesh(mesh, *, iterations: int = 10, lam: float = 0.5, mu: float = -0.53, fix_boundary: bool = True) -> Mesh:
    """The Mesh (or (vertices, faces[, normals]) tuple) after `iterations` of Taubin's lambda | mu smoothing (ops.smooth_mesh): the
    marching-tetrahedra staircase and the wobble of a learned density go, the volume stays (mu < -lam; mu = 0 is plain Laplacian
    smoothing, which shrinks), the vertices on an open border stay where they are under fix_boundary.  Faces as given; normals, if
    the mesh has them, become vertex_normals of the smoothed positions.  iterations = 0 returns the mesh's own tensors."""
    vertices, faces, normals = _mesh_fields(mesh, "smooth_mesh")
    return Mesh(*ops.smooth_mesh(vertices, faces, normals, iterations=iterations, lam=lam, mu=mu, fix_boundary=fix_boundary)[:3])


def vertex_normals(mesh) -> torch.Tensor:
    """(V, 3) unit normals of a Mesh (or tuple) from its faces (ops.vertex_normals): area-weighted, towards lower density for the
    faces of extract_mesh, zero for a vertex no face uses."""
    vertices, faces, _ = _mesh_fields(mesh, "vertex_normals")
    return ops.vertex_normals(vertices, faces)


def decimate_mesh(mesh, *, cell, origin=(0.0, 0.0, 0.0)) -> Mesh:
    """The lighter Mesh (or (vertices, faces[, normals]) tuple) of vertex clustering (ops.decimate_mesh): the vertices inside one cell
    of the lattice origin + cell * (i, j, k) -- `cell` one number or three, in the mesh's units -- become one vertex at their mean,
    faces that lose a corner that way go, faces that end on one vertex set are welded into one; order and winding of what is kept
    stay.  Normals, if the mesh has them, become vertex_normals of the result.  ops.decimate_mesh also returns the map from old to
    new vertices and the statistics."""
    vertices, faces, normals = _mesh_fields(mesh, "decimate_mesh")
    return Mesh(*ops.decimate_mesh(vertices, faces, normals, cell=cell, origin=origin)[:3])


def _decimate_cells(decimate, what: str):
    """None, or K > 0 as a float: the edge of a decimation cell in grid cells."""
    if decimate is None:
        return None
    try:
        k = None if isinstance(decimate, (bool, str)) else float(decimate)
    except (TypeError, ValueError):
        k = None
    if k is None or not (0.0 < k < float("inf")):
        raise ValueError(f"{what}: decimate is None or a number of grid cells > 0, got {decimate!r}")
    return k


def decimation_lattice(lo, hi, resolution, k):
    """(cell, origin) of the lattice extract_mesh(decimate=k) clusters on: cells of k grid cells, k * (hi - lo) / (n - 1) per axis,
    from the box's corner `lo`."""
    return [float(k) * (float(h) - float(l)) / (int(n) - 1) for l, h, n in zip(lo, hi, _resolution(resolution))], [float(x) for x in lo]


def extract_mesh(model, expr, latent_code=None, *, lo, hi, resolution, level, normals: bool = True, chunk_points: int = 1 << 22, brick=None,
                 margin: float = 0.0, dilate: int = 1, largest: bool = False, min_faces=None, smooth: int = 0, smooth_lam: float = 0.5,
                 smooth_mu: float = -0.53, decimate=None) -> Mesh:
    """The surface raw density == level of a fused model inside the box [lo, hi] for one expression (and latent code): density_grid,
    then ops.isosurface.  `level` is in raw-density units (before the ReLU of the volume renderer) and has no default: what counts
    as surface depends on the scene's scale and on how the model was trained.  With `brick` (cells per brick, e.g. 8) the grid is
    density_grid_sparse's: the network runs only in the bricks near the surface, and the mesh is the dense one wherever no brick
    hides a feature between its corners (`margin`, `dilate`: ops.sparse_grid).  The normals reach one point past a brick, so they
    need dilate >= 1.  With largest=True or min_faces=N the mesh is filter_mesh's: its largest component, or those of at least N
    faces; with neither (the default) nothing more is launched.  With smooth=N the result is smooth_mesh's after N iterations with
    smooth_lam and smooth_mu, run after the component filter, so that floaters are not smoothed; at the default 0 nothing more is
    launched.  With decimate=K > 0 the result is decimate_mesh's on cells of K grid cells (cell = K h per axis, origin = lo), run
    after the filter and the smoothing: extract fine, then reduce; at the default None nothing more is launched."""
    decimate = _decimate_cells(decimate, "extract_mesh")
    try:
        whole = not isinstance(smooth, bool) and int(smooth) == smooth and int(smooth) >= 0
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole:
        raise ValueError(f"extract_mesh: smooth is a whole number of iterations, at least 0, got {smooth!r}")
    clean = largest or min_faces is not None
    if clean and (bool(largest) == (min_faces is not None) or (min_faces is not None and (isinstance(min_faces, bool) or int(min_faces) != min_faces
                                                                                          or int(min_faces) < 1))):
        raise ValueError("extract_mesh: exactly one rule applies, largest=True or min_faces=N with N >= 1")
    if brick is None:
        grid = density_grid(model, expr, latent_code, lo=lo, hi=hi, resolution=resolution, chunk_points=chunk_points)
    else:
        brick, margin, dilate = ops.check_sparse_grid_args(brick, margin, dilate, "extract_mesh")
        if normals and dilate == 0:
            raise ValueError("extract_mesh: normals=True needs dilate >= 1 (the central differences reach into the neighbouring brick)")
        grid, _ = density_grid_sparse(model, expr, latent_code, lo=lo, hi=hi, resolution=resolution, level=level, brick=brick, margin=margin,
                                      dilate=dilate, chunk_points=chunk_points)
    mesh = Mesh(*ops.isosurface(grid, float(level), lo, hi, normals=normals))
    if clean:
        mesh = filter_mesh(mesh, largest=largest, min_faces=min_faces)
    if int(smooth):
        mesh = smooth_mesh(mesh, iterations=int(smooth), lam=smooth_lam, mu=smooth_mu)
    if decimate is not None:
        cell, origin = decimation_lattice(lo, hi, resolution, decimate)
        mesh = decimate_mesh(mesh, cell=cell, origin=origin)
    return mesh


def vertex_colours(model, mesh, expr, latent_code=None, *, near, far, pose=None, view_z=None, samples: int = 8, depth, min_opacity: float = 1e-3,
                   chunk_points: int = 1 << 22) -> MeshColours:
    """The colour of every vertex of a Mesh (or a (vertices, faces[, normals]) tuple; without normals, vertex_normals(mesh) are used)
    under a fused model's radiance field, for one expression (and latent code): MeshColours(colours (V, 3) float32 in [0, 1],
    opacity (V,) float32).  Through every vertex runs a ray along the inward normal with `samples` samples spread over the shell
    [-depth, +depth] round the surface (ops.mesh_colour_rays); the model's full forward (model.hip_forward, the arithmetic of
    nerf.set_mlp_precision; never live_only) gives colour and density there, and ops.mesh_colour_integrate composites them from
    outside to inside as the renderer does and divides by the opacity gathered -- the colour a camera just outside the surface sees,
    without the background the camera-ray integrator ends on.  Where the shell absorbs less than `min_opacity` the colour is that
    of the sample at the vertex (samples // 2).

    `depth`, in world units, has no default: how far the true surface can lie from a vertex depends on the grid cell the mesh was
    extracted on and on how much it was smoothed (the length of a cell's diagonal is what launch/extract_mesh.py takes).  Under
    Quirk Q1 the network's direction input is PE4(view z, near, far): `near` and `far` are the config's, and the view direction is
    either that of the camera `pose` (camera-to-world, (3, 4) or (4, 4) on the device: every vertex gets the direction of the pixel
    that sees it, a vertex behind the camera the central ray) or (0, 0, view_z) -- exactly one of the two.

    Inference only, under torch.no_grad(); nerf.density's guards, one weight pack per call, the split-fp16 range check after it.  In
    slabs of max(1, chunk_points // samples) whole vertices; the same bits for any chunk_points.  No vertices: nothing is launched."""
    vertices, faces, normals = _mesh_fields(mesh, "vertex_colours")
    if not torch.is_tensor(vertices) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("vertex_colours: vertices must be a tensor of shape (V, 3)")
    samples, depth, _ = ops._check_colour_args(samples, depth, pose, view_z, "vertex_colours")
    with torch.no_grad():
        expr, latent = _point_query(model, vertices, expr, latent_code, "vertex_colours")
        if vertices.shape[0] == 0:
            return MeshColours(torch.empty((0, 3), dtype=torch.float32, device=vertices.device), torch.empty((0,), dtype=torch.float32, device=vertices.device))
        if normals is None:
            normals = ops.vertex_normals(vertices, faces)
        ops.bump_pack_epoch()          # as nerf.density: a weight image never outlives one call
        near, far = float(near), float(far)
        forward = lambda ro, rd, z, rd_view: model.hip_forward(ro, rd, z, rd_view, expr, latent, near, far, need_grad=False)[0]
        out = ops.vertex_colours(forward, vertices, normals, samples=samples, depth=depth, pose=pose, view_z=view_z, min_opacity=min_opacity,
                                 chunk_points=chunk_points)
        if ops.get_mlp_precision() in ops.F16_MODES:
            ops.check_f16_range(model)
    return out


def _host(mesh):
    v, f, n = (tuple(mesh) + (None,))[:3]
    to = lambda t, dt: None if t is None else np.ascontiguousarray((t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)), dtype=dt)
    v, f, n = to(v, "<f4"), to(f, "<i4"), to(n, "<f4")
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or (n is not None and n.shape != v.shape):
        raise ValueError("write_mesh: expected vertices (V, 3), faces (F, 3) and normals (V, 3) or None")
    return v, f, n


def quantise_colours(colours) -> np.ndarray:
    """(V, 3) uint8 of float colours by the rule the rendered frames are written with (cast_to_image): clip to [0, 1], times 255 in
    float32, truncate; a NaN becomes 0.  uint8 input is returned as it is."""
    c = np.asarray(colours)
    if c.dtype == np.uint8:
        return np.ascontiguousarray(c)
    c = np.nan_to_num(c.astype(np.float32), nan=0.0)
    return (np.clip(c, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)


def _host_colours(colours, n_vertices):
    """(floats (V, 3) float32 for the text formats, bytes (V, 3) uint8) of write_mesh's colours."""
    c = colours.detach().cpu().numpy() if torch.is_tensor(colours) else np.asarray(colours)
    if c.shape != (n_vertices, 3) or not (c.dtype == np.uint8 or np.issubdtype(c.dtype, np.floating)):
        raise ValueError(f"write_mesh: colours must be ({n_vertices}, 3), the vertices' shape, float in [0, 1] or uint8, got {c.dtype} {c.shape}")
    as_float = c.astype(np.float32) / np.float32(255) if c.dtype == np.uint8 else c.astype(np.float32)
    return as_float, quantise_colours(c)


def write_mesh(path: str, mesh, colours=None) -> None:
    """Write Mesh(vertices, faces, normals) -- or a (vertices, faces[, normals]) tuple -- in the format the extension names: .off
    (positions and faces; floats printed with 9 significant digits, which round-trips float32), .obj (`vn` lines and `f a//a`
    indices when there are normals) or .ply (binary little-endian: float x y z [nx ny nz], then uchar 3 + three int32 per face).

    colours: None, or (V, 3) per-vertex colours (nerf.vertex_colours), a tensor or an array, float in [0, 1] or uint8.  Floats are
    quantised by the rule the rendered frames are written with (cast_to_image): clip to [0, 1], multiply by 255 in float32,
    truncate.  .ply: `property uchar red / green / blue` behind the normals, if any; .obj: `v x y z r g b` with the floats as they
    are, 9 significant digits (uint8 divided by 255); .off: the header becomes COFF and a vertex line `x y z r g b 255` with the
    bytes.  Without colours every format is what it was, byte for byte."""
    v, f, n = _host(mesh)
    if colours is not None:
        c_float, c_byte = _host_colours(colours, len(v))
    ext = os.path.splitext(path)[1].lower()
    if ext == ".off":
        with open(path, "w") as fh:
            fh.write(f"{'OFF' if colours is None else 'COFF'}\n{len(v)} {len(f)} 0\n")
            if colours is None:
                fh.writelines("%.9g %.9g %.9g\n" % tuple(p) for p in v.tolist())
            else:
                fh.writelines("%.9g %.9g %.9g %d %d %d 255\n" % (*p, *c) for p, c in zip(v.tolist(), c_byte.tolist()))
            fh.writelines("3 %d %d %d\n" % tuple(t) for t in f.tolist())
    elif ext == ".obj":
        with open(path, "w") as fh:
            if colours is None:
                fh.writelines("v %.9g %.9g %.9g\n" % tuple(p) for p in v.tolist())
            else:
                fh.writelines("v %.9g %.9g %.9g %.9g %.9g %.9g\n" % (*p, *c) for p, c in zip(v.tolist(), c_float.tolist()))
            if n is not None:
                fh.writelines("vn %.9g %.9g %.9g\n" % tuple(p) for p in n.tolist())
                fh.writelines("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) for a, b, c in (f + 1).tolist())
            else:
                fh.writelines("f %d %d %d\n" % tuple(t) for t in (f + 1).tolist())
    elif ext == ".ply":
        props = ["x", "y", "z"] + (["nx", "ny", "nz"] if n is not None else [])
        header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {len(v)}\n" + "".join(f"property float {p}\n" for p in props) + \
                 ("" if colours is None else "".join(f"property uchar {p}\n" for p in ("red", "green", "blue"))) + \
                 f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n"
        rows = np.zeros(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
        rows["n"], rows["i"] = 3, f
        floats = (v if n is None else np.concatenate([v, n], axis=1)).astype("<f4")
        if colours is not None:
            packed = np.zeros(len(v), dtype=[("f", "<f4", (floats.shape[1],)), ("c", "u1", (3,))])
            packed["f"], packed["c"] = floats, c_byte
        with open(path, "wb") as fh:
            fh.write(header.encode("ascii"))
            fh.write(floats.tobytes() if colours is None else packed.tobytes())
            fh.write(rows.tobytes())
    else:
        raise ValueError(f"write_mesh: unknown extension {ext!r} (.off, .obj or .ply)")
