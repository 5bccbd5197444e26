"""NumPy restatement of the isosurface specification (DESIGN.md "Isosurface"): marching tetrahedra on the Kuhn triangulation of a
dense grid v[nz][ny][nx], every float operation in float32 and in the specified order.  The tests compare the library against it;
nothing in the product imports it.

    derive_table()                              -> (6, 16) uint32, the encoding of nf_isosurface_table
    isosurface(v, level, lo, hi, normals=False) -> verts (V,3) f32, faces (F,3) i32, normals (V,3) f32 or None
    mesh_report(verts, faces)                   -> closedness / orientation / Euler characteristic / signed volume
"""
import itertools
import struct

import numpy as np

PERMS = list(itertools.permutations((0, 1, 2)))          # lexicographic


def tet_corners(tet):
    p = PERMS[tet]
    return (0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7)


def _corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, c >> 2], dtype=np.float64)


def case_triangles(tet, mask):
    """Triangles of one tetrahedron for one inside mask (bit n = tet vertex n inside): a list of triangles, each three edges
    (m, n) of tet vertices with m < n, the flip already applied; and the flip bit."""
    inside = [v for v in range(4) if (mask >> v) & 1]
    outside = [v for v in range(4) if not (mask >> v) & 1]
    if len(inside) == 1:
        a, (b, c, d) = inside[0], outside
        tris, pair = [[(a, b), (a, c), (a, d)]], (a, b)
    elif len(inside) == 3:
        a, (b, c, d) = outside[0], inside
        tris, pair = [[(a, b), (a, c), (a, d)]], (b, a)
    elif len(inside) == 2:
        (a, b), (c, d) = inside, outside
        tris, pair = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]], (a, c)
    else:
        return [], False
    corners = tet_corners(tet)
    direction = _corner_xyz(corners[pair[1]]) - _corner_xyz(corners[pair[0]])          # inside -> outside
    flips = []
    for tri in tris:
        p = [0.5 * (_corner_xyz(corners[m]) + _corner_xyz(corners[n])) for m, n in tri]
        s = float(np.dot(np.cross(p[1] - p[0], p[2] - p[0]), direction))
        assert s != 0.0
        flips.append(s < 0.0)
    assert len(set(flips)) == 1, (tet, mask, flips)                                     # both triangles of a quad agree
    flip = flips[0]
    out = [[tuple(sorted(e)) for e in ((t[0], t[2], t[1]) if flip else t)] for t in tris]
    return out, flip


def derive_table():
    table = np.zeros((6, 16), dtype=np.uint32)
    for tet in range(6):
        for mask in range(16):
            tris, flip = case_triangles(tet, mask)
            e = len(tris) << 24 | (1 << 26 if flip else 0)
            for k, tri in enumerate(tris):
                for v, (m, n) in enumerate(tri):
                    e |= (m | n << 2) << (4 * (3 * k + v))
            table[tet, mask] = e
    return table


def _axis(lo, hi, n):
    h = (np.float32(hi) - np.float32(lo)) / np.float32(n - 1)
    return np.float32(lo) + np.arange(n, dtype=np.float32) * h, h


def _gradient(v, hs):
    """Central differences, one-sided at the box faces, divided by the spacing: (nz, ny, nx, 3) in x, y, z order."""
    g = np.zeros(v.shape + (3,), dtype=np.float32)
    for comp, axis in ((0, 2), (1, 1), (2, 0)):
        n = v.shape[axis]
        w = np.moveaxis(v, axis, 0)
        d = np.empty_like(w)
        two_h, h = np.float32(2.0) * hs[comp], hs[comp]
        d[1:-1] = (w[2:] - w[:-2]) / two_h
        d[0] = (w[1] - w[0]) / h
        d[n - 1] = (w[n - 1] - w[n - 2]) / h
        g[..., comp] = np.moveaxis(d, 0, axis)
    return g


def isosurface(v, level, lo, hi, normals=False):
    v = np.ascontiguousarray(v, dtype=np.float32)
    nz, ny, nx = v.shape
    assert min(nx, ny, nz) >= 2
    level = np.float32(level)
    with np.errstate(all="ignore"):
        inside = v > level                                                              # NaN and == level: outside
        xs, hx = _axis(lo[0], hi[0], nx)
        ys, hy = _axis(lo[1], hi[1], ny)
        zs, hz = _axis(lo[2], hi[2], nz)
        # ---- vertices: crossing edges in the order (k, j, i, e)
        cross = np.zeros((nz, ny, nx, 7), dtype=bool)
        for e in range(1, 8):
            dx, dy, dz = e & 1, (e >> 1) & 1, e >> 2
            a = inside[:nz - dz, :ny - dy, :nx - dx]
            b = inside[dz:, dy:, dx:]
            cross[:nz - dz, :ny - dy, :nx - dx, e - 1] = a != b
        flat = cross.reshape(-1)
        ids = np.cumsum(flat) - flat                                                    # exclusive count
        vid = np.where(flat, ids, -1).reshape(cross.shape)
        k_, j_, i_, e_ = np.nonzero(cross)                                              # already in (k, j, i, e) order
        e_ = e_ + 1
        dx, dy, dz = e_ & 1, (e_ >> 1) & 1, e_ >> 2
        va, vb = v[k_, j_, i_], v[k_ + dz, j_ + dy, i_ + dx]
        t = (level - va) / (vb - va)
        t = np.where((t >= 0) & (t <= 1), t, np.float32(0.5)).astype(np.float32)
        pa = np.stack([xs[i_], ys[j_], zs[k_]], axis=1)
        pb = np.stack([xs[i_ + dx], ys[j_ + dy], zs[k_ + dz]], axis=1)
        verts = (pa + t[:, None] * (pb - pa)).astype(np.float32)
        norm = None
        if normals:
            g = _gradient(v, (hx, hy, hz))
            ga, gb = g[k_, j_, i_], g[k_ + dz, j_ + dy, i_ + dx]
            gi = ga + t[:, None] * (gb - ga)
            length = np.sqrt((gi[:, 0] * gi[:, 0] + gi[:, 1] * gi[:, 1]) + gi[:, 2] * gi[:, 2])
            ok = (length > 0) & np.isfinite(length)
            norm = np.where(ok[:, None], -(gi / np.where(ok, length, np.float32(1.0))[:, None]), np.float32(0.0)).astype(np.float32)
    # ---- faces: (cell, tetrahedron, triangle); only cells with a mixed corner set can hold one
    cases = [[case_triangles(tet, mask)[0] for mask in range(16)] for tet in range(6)]
    corner_in = np.stack([inside[(c >> 2):nz - 1 + (c >> 2), ((c >> 1) & 1):ny - 1 + ((c >> 1) & 1), (c & 1):nx - 1 + (c & 1)] for c in range(8)])
    n_in = corner_in.sum(axis=0)
    faces = []
    for k, j, i in zip(*np.nonzero((n_in > 0) & (n_in < 8))):                           # np.nonzero: cell linear order
        for tet in range(6):
            corners = tet_corners(tet)
            mask = sum(int(corner_in[c, k, j, i]) << n for n, c in enumerate(corners))
            for tri in cases[tet][mask]:
                row = []
                for m, n in tri:
                    ca, cb = corners[m], corners[n]
                    e = ca ^ cb
                    assert ca & cb == ca and e
                    w = vid[k + (ca >> 2), j + ((ca >> 1) & 1), i + (ca & 1), e - 1]
                    assert w >= 0
                    row.append(w)
                faces.append(row)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    return verts, faces, norm


def mesh_report(verts, faces):
    """closed: every directed edge once and its reverse once; plus zero-area triangles, unreferenced vertices, chi, signed volume."""
    f = faces.astype(np.int64)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(verts.shape[0]) + 1
    key = directed[:, 0] * n + directed[:, 1]
    rev = directed[:, 1] * n + directed[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    closed = bool(np.all(counts == 1) and np.array_equal(uniq, np.unique(rev)))
    p = verts.astype(np.float64)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    area2 = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    undirected = np.unique(np.minimum(key, rev))
    return {"closed": closed, "zero_area": int(np.sum(area2 == 0.0)), "unreferenced": int(verts.shape[0] - np.unique(f).size),
            "chi": int(verts.shape[0] - undirected.size + f.shape[0]), "volume": float(np.sum(np.einsum("ij,ij->i", a, np.cross(b, c))) / 6.0)}


# ---- the fields of the tests (built in float32)
BOX_LO, BOX_HI, BOX_N = (-1.1, -0.9, -1.0), (1.2, 1.0, 1.1), (23, 19, 21)


def grid_points(lo, hi, n):
    """(nz, ny, nx) float32 coordinate arrays X, Y, Z of the grid points."""
    xs, ys, zs = (_axis(lo[a], hi[a], n[a])[0] for a in range(3))
    z, y, x = np.meshgrid(zs, ys, xs, indexing="ij")
    return x, y, z


def sphere(x, y, z, r=0.7, cx=0.0):
    return (np.float32(r * r) - ((x - np.float32(cx)) ** 2 + y ** 2 + z ** 2)).astype(np.float32)


def torus(x, y, z, big=0.55, small=0.22):
    q = np.sqrt(x ** 2 + y ** 2) - np.float32(big)
    return (np.float32(small * small) - (q ** 2 + z ** 2)).astype(np.float32)


def two_spheres(x, y, z, r=0.3, off=0.5):
    return np.maximum(sphere(x, y, z, r, -off), sphere(x, y, z, r, off))


def noise_field(seed=0, n=(10, 8, 9)):
    """(nz, ny, nx) seeded noise with a shell of outside values, so that every surface component is closed."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n[2], n[1], n[0])).astype(np.float32)
    v[0], v[-1], v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1] = -1, -1, -1, -1, -1, -1
    return v


def read_ply(path):
    """A binary little-endian .ply of float vertex properties and triangle faces -> (vertex rows, faces, property names, header, body)."""
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n_v = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    n_f = int([l for l in lines if l.startswith("element face")][0].split()[2])
    props = [l.split()[2] for l in lines if l.startswith("property float")]
    vert = np.frombuffer(body, dtype="<f4", count=n_v * len(props)).reshape(n_v, len(props))
    rest = body[n_v * len(props) * 4:]
    assert len(rest) == 13 * n_f
    faces = np.array([struct.unpack_from("<B3i", rest, 13 * i) for i in range(n_f)], dtype=np.int64).reshape(n_f, 4)
    assert (faces[:, 0] == 3).all()
    return vert, faces[:, 1:].astype(np.int32), props, head, body
