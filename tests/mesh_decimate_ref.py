"""NumPy restatement of the mesh-decimation specification (DESIGN.md "Mesh decimation"), the text csrc/nf_mesh_decimate.hip is held
to exactly: every float32 and float64 operation the specification names is one NumPy operation of that type here, so every
comparison is array_equal on the bit patterns.

    cells(vertices, origin, cell)       -> t (V, 3) float32, i (V, 3) int64, clustered (V,) bool, key (V,) int64
    representatives(vertices, origin, cell) -> rep (V,) int64, members (V,) int64 (of v's cluster), and the four above
    decimate(vertices, faces, cell, origin=(0, 0, 0), normals=None)
                                        -> vertices' (V', 3) float32, faces' (F', 3) int32, normals' or None, vertex_map (V,) int32, stats

stats is a dict with the fields of ops.MeshDecimateStats.  `cell` is one number or three.
"""
import numpy as np

from tests import mesh_smooth_ref as S

RANGE = 1 << 20                       # cell indices lie in [-2^20, 2^20)
SCALE = 1 << 30                       # the fixed point of a position inside its cell


def _three(x):
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    return np.repeat(x, 3) if x.size == 1 else x


def cells(vertices, origin, cell):
    p = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    o, c = _three(origin), _three(cell)
    assert o.shape == c.shape == (3,) and np.isfinite(o).all() and np.isfinite(c).all() and (c > 0).all()
    with np.errstate(all="ignore"):
        t = (p - o[None, :]) / c[None, :]                                            # float32 - float32, float32 / float32
        low = np.floor(t)
        clustered = (np.isfinite(t) & (low >= np.float32(-RANGE)) & (low < np.float32(RANGE))).all(axis=1)
    i = np.where(clustered[:, None], low, np.float32(0)).astype(np.int64)
    key = (i[:, 0] + RANGE) + (i[:, 1] + RANGE) * (1 << 21) + (i[:, 2] + RANGE) * (1 << 42)
    assert t.dtype == np.float32
    return t, i, clustered, np.where(clustered, key, -1)


def representatives(vertices, origin, cell):
    t, i, clustered, key = cells(vertices, origin, cell)
    n_vertices = len(key)
    rep, members = np.arange(n_vertices, dtype=np.int64), np.ones(n_vertices, dtype=np.int64)
    ids = np.flatnonzero(clustered)                                                    # ascending: a key's first occurrence is its smallest id
    if len(ids):
        _, first, inverse, counts = np.unique(key[ids], return_index=True, return_inverse=True, return_counts=True)
        rep[ids], members[ids] = ids[first[inverse]], counts[inverse]
    return rep, members, t, i, clustered, key


def _even(r, s):
    """r is an even permutation of the ascending triple s: one of its three rotations."""
    return (r == s).all(axis=1) | (r == s[:, [1, 2, 0]]).all(axis=1) | (r == s[:, [2, 0, 1]]).all(axis=1)


def decimate(vertices, faces, cell, origin=(0.0, 0.0, 0.0), normals=None):
    p = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    o, c = _three(origin), _three(cell)
    n_vertices, n_faces = p.shape[0], faces.shape[0]
    rep, members, t, i, clustered, _ = representatives(p, o, c)

    # faces
    valid = S.valid_faces(faces, n_vertices)
    ids = np.flatnonzero(valid)
    r = rep[faces[ids]]
    distinct = (r[:, 0] != r[:, 1]) & (r[:, 1] != r[:, 2]) & (r[:, 2] != r[:, 0])
    ids, r = ids[distinct], r[distinct]
    s = np.sort(r, axis=1)
    keep = np.zeros(len(ids), dtype=bool)
    if len(ids):
        even = _even(r, s)
        _, group = np.unique(s, axis=0, return_inverse=True)
        group = group.reshape(-1)
        n_groups = int(group.max()) + 1
        n_even, n_odd = np.bincount(group[even], minlength=n_groups), np.bincount(group[~even], minlength=n_groups)
        first_even, first_odd = np.full(n_groups, n_faces, dtype=np.int64), np.full(n_groups, n_faces, dtype=np.int64)
        np.minimum.at(first_even, group[even], ids[even])
        np.minimum.at(first_odd, group[~even], ids[~even])
        winner = np.where(n_even > n_odd, first_even, np.where(n_odd > n_even, first_odd, -1))
        keep = ids == winner[group]
    kept_ids, kept_r = ids[keep], r[keep]                                              # ascending face id, each its own r in its own order

    # vertices
    used = np.zeros(n_vertices, dtype=bool)
    used[kept_r.reshape(-1)] = True
    new_id = np.where(used, np.cumsum(used) - 1, -1)
    vertex_map = new_id[rep].astype(np.int32)
    out_faces = new_id[kept_r].astype(np.int32).reshape(-1, 3)

    reps = np.flatnonzero(used)
    out = p[reps].copy()                                                               # one member: its floats, bit for bit
    many = members[reps] > 1
    if many.any():
        inside = clustered & (members > 1)
        with np.errstate(all="ignore"):
            frac = t[inside] - i[inside].astype(np.float32)                            # one float32 subtraction
        q = (frac * np.float32(SCALE)).astype(np.int64)                                # exact scaling, truncation
        assert frac.dtype == np.float32 and q.min() >= 0 and q.max() <= SCALE
        total = np.zeros((n_vertices, 3), dtype=np.int64)
        np.add.at(total, rep[inside], q)                                               # exact, any order
        u = reps[many]
        m = total[u].astype(np.float64) / members[u].astype(np.float64)[:, None]
        x = o.astype(np.float64)[None, :] + c.astype(np.float64)[None, :] * (i[u].astype(np.float64) + m * np.float64(2.0 ** -30))
        out[many] = x.astype(np.float32)
    assert out.dtype == np.float32

    stats = dict(vertices=n_vertices, kept_vertices=len(reps), faces=n_faces, kept_faces=len(kept_ids), degenerate_faces=int((~distinct).sum()),
                 coincident_faces=int(len(ids) - len(kept_ids)), invalid_faces=int(n_faces - valid.sum()),
                 unclustered_vertices=int(n_vertices - clustered.sum()), largest_cluster=int(members.max()) if n_vertices else 0)
    out_normals = None if normals is None else S.vertex_normals(out, out_faces)
    return out, out_faces, out_normals, vertex_map, stats


# ---- the meshes of the tests
def random_mesh(rng, n_vertices, n_faces, cell=1.0, origin=(0.0, 0.0, 0.0), spread=1.5):
    """Seeded (vertices, faces): normal positions round the origin of the lattice (negative coordinates included), a few of them NaN,
    infinite, at and just inside either end of the cell range; tests/mesh_components_ref.py's faces (invalid and repeated indices
    among them), about one in four a copy of another face with its corners rotated or swapped."""
    from tests import mesh_components_ref as M
    o, c = _three(origin), _three(cell)
    p = (rng.standard_normal((n_vertices, 3)) * spread).astype(np.float32) * c + o
    edge = np.float32(RANGE) * c
    special = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), o[0] + edge[0], o[0] - edge[0], np.nextafter(o[0] + edge[0], np.float32(0)),
               np.nextafter(o[0] - edge[0], np.float32(-np.inf)), np.float32(3e38), np.float32(-3e38)]
    for k in range(min(n_vertices // 6, 2 * len(special))):
        p[rng.integers(0, n_vertices), rng.integers(0, 3)] = special[k % len(special)]
    faces = M.random_faces(rng, n_vertices, n_faces)
    orders = [(1, 2, 0), (2, 0, 1), (0, 2, 1), (1, 0, 2), (2, 1, 0), (0, 1, 2)]
    for k in range(n_faces // 4):
        a, b = rng.integers(0, n_faces, size=2)
        faces[a] = faces[b][list(orders[k % 6])]
    return p.astype(np.float32), np.ascontiguousarray(faces, dtype=np.int32)


def cell_boxes(vertices, origin, cell):
    """(lo, hi) float64 (V, 3): the box of every vertex's cell, o + c i and o + c (i + 1) in float64 (meaningful for clustered ones)."""
    _, i, _, _ = cells(vertices, origin, cell)
    o, c = _three(origin).astype(np.float64), _three(cell).astype(np.float64)
    return o + c * i, o + c * (i + 1)
