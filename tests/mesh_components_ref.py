"""NumPy restatement of the mesh-components specification (DESIGN.md "Mesh components"), the text csrc/nf_mesh_components.hip is held
to exactly -- every output is an integer or a copied float, so every comparison is array_equal.

    mesh_components(faces, n_vertices) -> vertex_label (V,), face_label (F,), face_counts (C,), vertex_counts (C,), all int32
    kept_components(face_counts, largest=, min_faces=) -> (C,) bool
    filter_mesh(vertices, faces, normals=None, largest=, min_faces=) -> vertices, faces, normals or None, stats (dict)

A face is valid iff its three indices lie in [0, V); vertices are connected through valid faces (a shared vertex is enough); the
components are numbered by ascending smallest vertex id; a face carries the label of its first vertex, an invalid face -1.
"""
import numpy as np


def valid_faces(faces, n_vertices):
    faces = np.asarray(faces).reshape(-1, 3)
    return ((faces >= 0) & (faces < n_vertices)).all(axis=1)


def smallest_vertex(faces, n_vertices):
    """(V,) int64: for every vertex the smallest vertex id of its component.  Every valid face hands the smallest value among its
    three vertices to all three, then every vertex jumps to the value of its value; repeated until nothing changes."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    low = np.arange(n_vertices, dtype=np.int64)
    tri = faces[valid_faces(faces, n_vertices)]
    while tri.size:
        new = low.copy()
        np.minimum.at(new, tri.reshape(-1), np.repeat(low[tri].min(axis=1), 3))
        while True:
            jump = new[new]
            if np.array_equal(jump, new):
                break
            new = jump
        if np.array_equal(new, low):
            break
        low = new
    return low


def mesh_components(faces, n_vertices):
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    low = smallest_vertex(faces, n_vertices)
    is_root = low == np.arange(n_vertices)
    rank = np.cumsum(is_root) - 1                                          # the numbering rule: ascending smallest vertex
    n_components = int(is_root.sum())
    vertex_label = rank[low].astype(np.int32)
    valid = valid_faces(faces, n_vertices)
    face_label = np.full(faces.shape[0], -1, dtype=np.int32)
    face_label[valid] = vertex_label[faces[valid, 0]]
    face_counts = np.bincount(face_label[valid], minlength=n_components).astype(np.int32)
    vertex_counts = np.bincount(vertex_label, minlength=n_components).astype(np.int32)
    return vertex_label, face_label, face_counts, vertex_counts


def kept_components(face_counts, largest=False, min_faces=None):
    if bool(largest) == (min_faces is not None):
        raise ValueError("exactly one rule applies")
    keep = np.zeros(len(face_counts), dtype=bool)
    if largest:
        if len(face_counts) and face_counts.max() > 0:
            keep[int(np.argmax(face_counts))] = True                      # argmax: the first of equal counts, i.e. the lower label
    else:
        if min_faces < 1:
            raise ValueError("min_faces >= 1")
        keep = face_counts >= min_faces
    return keep


def random_faces(rng, n_vertices, n_faces):
    """Seeded faces over n_vertices vertices: about one in six with an index outside [0, V) (-1, V, far outside), about one in five
    with a repeated index."""
    faces = rng.integers(0, n_vertices, size=(n_faces, 3)).astype(np.int32)
    for f in range(n_faces):
        roll = rng.integers(0, 30)
        if roll < 5:
            faces[f, rng.integers(0, 3)] = (-1, n_vertices, -2 ** 31, 2 ** 31 - 1, n_vertices + 7)[roll]
        elif roll < 11:
            faces[f, (roll + 1) % 3] = faces[f, roll % 3]
    return faces


# the field of the end-to-end test: a sphere A and two smaller ones, each written only inside a box round its centre
E2E_N, E2E_LO, E2E_HI = (33, 29, 25), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
E2E_A = (0.45, (-0.3, 0.0, 0.0))
E2E_SMALL = [(0.2, (0.6, 0.3, 0.1), 0.3), (0.12, (0.55, -0.6, -0.5), 0.22)]          # radius, centre, half-width of the box


def e2e_fields(x, y, z):
    """(A alone, A with the two small spheres) on the float32 coordinate arrays x, y, z: r^2 - |p - c|^2 each; outside the boxes the
    second field IS the first, so the surface of A and its normals (central differences) are the same in both."""
    ball = lambda r, c: (np.float32(r * r) - ((x - np.float32(c[0])) ** 2 + (y - np.float32(c[1])) ** 2 + (z - np.float32(c[2])) ** 2)).astype(np.float32)
    alone = ball(*E2E_A)
    both = alone.copy()
    for r, c, half in E2E_SMALL:
        box = (np.abs(x - np.float32(c[0])) <= half) & (np.abs(y - np.float32(c[1])) <= half) & (np.abs(z - np.float32(c[2])) <= half)
        both[box] = ball(r, c)[box]
    return alone, both


def filter_mesh(vertices, faces, normals=None, largest=False, min_faces=None):
    vertices, faces = np.asarray(vertices), np.asarray(faces).reshape(-1, 3)
    n_vertices = vertices.shape[0]
    vertex_label, face_label, face_counts, _ = mesh_components(faces, n_vertices)
    keep = kept_components(face_counts, largest, min_faces)
    keep_v = keep[vertex_label] if n_vertices else np.zeros(0, dtype=bool)
    keep_f = (face_label >= 0) & np.append(keep, False)[face_label]        # label -1 reads the appended False
    new_id = np.cumsum(keep_v) - 1
    out_f = new_id[faces[keep_f].astype(np.int64)].astype(np.int32).reshape(-1, 3)
    stats = dict(components=len(face_counts), kept_components=int(keep.sum()), vertices=n_vertices, kept_vertices=int(keep_v.sum()),
                 faces=faces.shape[0], kept_faces=int(keep_f.sum()))
    return vertices[keep_v].reshape(-1, 3), out_f, None if normals is None else np.asarray(normals)[keep_v].reshape(-1, 3), stats
