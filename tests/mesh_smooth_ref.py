"""NumPy restatement of the mesh-smoothing specification (DESIGN.md "Mesh smoothing"), the text csrc/nf_mesh_smooth.hip is held to
exactly: every float32 operation the specification fixes is one NumPy float32 operation here, in the same order, so every
comparison is array_equal on the bit patterns.

    adjacency(faces, n_vertices)      -> row_start (V+1,), neighbours (E,), multiplicity (E,) int32, boundary (V,) uint8
    one_pass(p, row_start, neighbours, factor, pinned=None) -> p' (V, 3) float32
    smooth(vertices, faces, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True) -> vertices' (V, 3) float32
    vertex_normals(vertices, faces)   -> (V, 3) float32
    smooth_mesh(vertices, faces, normals=None, ...) -> vertices', faces, normals' or None, stats (dict)

A face is valid iff its three indices lie in [0, V).  A valid face (a, b, c) has the sides ab, bc, ca; a side with equal ends is
dropped.  N(v) = the distinct w != v joined to v by a side, ascending; the multiplicity of {v, w} = the number of sides joining
them; v is on the boundary iff it ends an edge of multiplicity 1.
"""
import numpy as np


def valid_faces(faces, n_vertices):
    faces = np.asarray(faces).reshape(-1, 3)
    return ((faces >= 0) & (faces < n_vertices)).all(axis=1)


def _csr(rows, entries, n_vertices):
    """Rows of ascending entries from (row, entry) pairs: row_start (V+1,) int64, and the pairs sorted by (row, entry)."""
    order = np.lexsort((entries, rows))
    rows, entries = rows[order], entries[order]
    row_start = np.zeros(n_vertices + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_vertices), out=row_start[1:])
    return row_start, rows, entries


def adjacency(faces, n_vertices):
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    tri = faces[valid_faces(faces, n_vertices)]
    ends = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])            # the sides
    ends = ends[ends[:, 0] != ends[:, 1]]
    rows, cols = np.concatenate([ends[:, 0], ends[:, 1]]), np.concatenate([ends[:, 1], ends[:, 0]])
    key, multiplicity = np.unique(rows * (n_vertices + 1) + cols, return_counts=True)   # ascending: by row, then by neighbour
    rows, neighbours = key // (n_vertices + 1), key % (n_vertices + 1)
    row_start = np.zeros(n_vertices + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_vertices), out=row_start[1:])
    boundary = np.zeros(n_vertices, dtype=np.uint8)
    boundary[rows[multiplicity == 1]] = 1
    return row_start.astype(np.int32), neighbours.astype(np.int32), multiplicity.astype(np.int32), boundary


def _ordered_sum(row_start, entries, values):
    """(V, 3) float32: per row the sum of values[entries] from the row's first entry on, one float32 addition per further entry;
    zero for an empty row."""
    row_start = np.asarray(row_start, dtype=np.int64)
    n = len(row_start) - 1
    d = np.diff(row_start)
    s = np.zeros((n, 3), dtype=np.float32)
    some = np.flatnonzero(d > 0)
    s[some] = values[entries[row_start[some]]]
    for k in range(1, int(d.max()) if n else 0):
        more = np.flatnonzero(d > k)
        s[more] = s[more] + values[entries[row_start[more] + k]]                     # float32 + float32: rounded once
    return s, d


def one_pass(p, row_start, neighbours, factor, pinned=None):
    p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
    f = np.float32(factor)
    with np.errstate(all="ignore"):
        s, d = _ordered_sum(row_start, np.asarray(neighbours, dtype=np.int64), p)
        moves = d > 0
        if pinned is not None:
            moves &= np.asarray(pinned) == 0
        m = s[moves] / d[moves].astype(np.float32)[:, None]
        t = m - p[moves]
        u = f * t
        out = p.copy()
        out[moves] = p[moves] + u
    assert out.dtype == np.float32
    return out


def check_factors(iterations, lam, mu):
    lam, mu = np.float32(lam), np.float32(mu)
    if isinstance(iterations, bool) or int(iterations) != iterations or iterations < 0:
        raise ValueError("iterations is a whole number of at least 0")
    if not (0 < lam <= 1) or not (-1 <= mu <= 0):
        raise ValueError("0 < lam <= 1 and -1 <= mu <= 0")
    return int(iterations), lam, mu


def smooth(vertices, faces, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True):
    iterations, lam, mu = check_factors(iterations, lam, mu)
    p = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    row_start, neighbours, _, boundary = adjacency(faces, p.shape[0])
    pinned = boundary if fix_boundary else None
    for _ in range(iterations):
        p = one_pass(p, row_start, neighbours, lam, pinned)
        if mu != 0:
            p = one_pass(p, row_start, neighbours, mu, pinned)
    return p


def vertex_normals(vertices, faces):
    p = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n_vertices = p.shape[0]
    ids = np.flatnonzero(valid_faces(faces, n_vertices))
    tri = faces[ids]
    with np.errstate(all="ignore"):
        e1, e2 = p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]]
        cross = np.zeros((faces.shape[0], 3), dtype=np.float32)
        cross[ids] = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                               e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        # every face once per vertex it holds: the second and third index only where they differ from the earlier ones
        second, third = tri[:, 1] != tri[:, 0], (tri[:, 2] != tri[:, 0]) & (tri[:, 2] != tri[:, 1])
        rows = np.concatenate([tri[:, 0], tri[second, 1], tri[third, 2]])
        held = np.concatenate([ids, ids[second], ids[third]])
        row_start, _, held = _csr(rows, held, n_vertices)                            # ascending face id within a row
        s, _ = _ordered_sum(row_start, held, cross)
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        ok = (length > 0) & np.isfinite(length)
        out = np.where(ok[:, None], s / np.where(ok, length, np.float32(1.0))[:, None], np.float32(0.0)).astype(np.float32)
    assert s.dtype == np.float32 and length.dtype == np.float32
    return out


def smooth_mesh(vertices, faces, normals=None, iterations=10, lam=0.5, mu=-0.53, fix_boundary=True):
    iterations, lam, mu = check_factors(iterations, lam, mu)
    vertices, faces = np.asarray(vertices), np.asarray(faces)
    if iterations == 0:
        return vertices, faces, normals, dict(edges=0, boundary_vertices=0, pinned_vertices=0, passes=0)
    row_start, neighbours, _, boundary = adjacency(faces, vertices.shape[0])
    out = smooth(vertices, faces, iterations, lam, mu, fix_boundary)
    n_boundary = int(boundary.sum())
    stats = dict(edges=len(neighbours), boundary_vertices=n_boundary, pinned_vertices=n_boundary if fix_boundary else 0,
                 passes=iterations * (2 if mu != 0 else 1))
    return out, faces, None if normals is None else vertex_normals(out, faces), stats


# ---- the meshes of the tests
def fan(n_rim, hub="first", order="ascending", closed=False, seed=0):
    """(V, faces): a fan of triangles (hub, rim[i], rim[i + 1]) over n_rim rim vertices -- n_rim - 1 faces, or n_rim when closed --
    with the hub at id 0 or V - 1 and the rim ids along the fan ascending, descending or permuted (the faces shuffled as well)."""
    rng = np.random.default_rng(seed)
    n_vertices = n_rim + 1
    centre = 0 if hub == "first" else n_vertices - 1
    rim = np.arange(n_rim) + (1 if hub == "first" else 0)
    rim = {"ascending": rim, "descending": rim[::-1], "permuted": rng.permutation(rim)}[order]
    nxt = np.roll(rim, -1)
    n_faces = n_rim if closed else n_rim - 1
    faces = np.stack([np.full(n_faces, centre), rim[:n_faces], nxt[:n_faces]], axis=1).astype(np.int32)
    if order == "permuted":
        faces = faces[rng.permutation(n_faces)]
    return n_vertices, np.ascontiguousarray(faces)


def positions(n_vertices, seed=1):
    return np.random.default_rng(seed).standard_normal((n_vertices, 3)).astype(np.float32)


def radial_sphere(x, y, z, r=0.7):
    """r - |p|: the field of the property tests (its level set 0 is the sphere of radius r, and noise added to it moves the
    surface by about its own size)."""
    return (np.float32(r) - np.sqrt(x * x + y * y + z * z)).astype(np.float32)
