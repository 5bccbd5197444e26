"""NumPy restatement of the mesh colour pass (DESIGN.md "Mesh colours"; csrc/nf_mesh_colour.hip): the rays with one float32 NumPy
operation per kernel operation, in the kernel's order, so that the bits agree; the composite in float64 (the reference of the GPU
tests) and in float32 (the kernel's order of operations, to show that the gates are reachable); the quantisation of write_mesh; and a
reader of the three coloured file formats."""
import struct

import numpy as np

F = np.float32
MAX_SAMPLES = 64


def depths(n_samples, depth):
    """z[k] = float(2 k - K + 1) * (depth / float(K)), float32."""
    half = F(depth) / F(n_samples)
    return (2 * np.arange(n_samples, dtype=np.int64) - n_samples + 1).astype(F) * half


def rays(vertices, normals, view, n_samples, depth):
    """(rd (V, 3), rd_view (V, 3), z (V, K)), float32.  view: a camera-to-world matrix (3, 4) or (4, 4), or the number view_z."""
    v = np.ascontiguousarray(vertices, dtype=F).reshape(-1, 3)
    n = np.ascontiguousarray(normals, dtype=F).reshape(-1, 3)
    assert 1 <= n_samples <= MAX_SAMPLES and F(depth) >= 0
    rd = -n
    z = np.broadcast_to(depths(n_samples, depth), (len(v), n_samples)).copy()
    if np.ndim(view) == 0:
        rd_view = np.zeros_like(v)
        rd_view[:, 2] = F(view)
        return rd, rd_view, z
    c2w = np.asarray(view, dtype=F)
    r02, r12, r22 = c2w[0, 2], c2w[1, 2], c2w[2, 2]
    with np.errstate(all="ignore"):
        t0, t1, t2 = v[:, 0] - c2w[0, 3], v[:, 1] - c2w[1, 3], v[:, 2] - c2w[2, 3]
        d = -((t0 * r02 + t1 * r12) + t2 * r22)
        front = d > 0                                                       # False for a NaN
        safe = np.where(front, d, F(1))
        rd_view = np.stack([np.where(front, t0 / safe, -r02), np.where(front, t1 / safe, -r12), np.where(front, t2 / safe, -r22)], axis=1).astype(F)
    return rd, rd_view, z


def _sigmoid(x):
    one = x.dtype.type(1)
    with np.errstate(over="ignore"):
        return one / (one + np.exp(-x))


def integrate(raw, step, min_opacity, dtype=np.float64):
    """(colour (V, 3), opacity (V,)) in `dtype`, the sums over k ascending.  float64: the reference; float32: the kernel's operations
    (its exp is the device's, so the bits need not agree)."""
    raw = np.asarray(raw, dtype=F).astype(dtype)
    n_vertices, n_samples, _ = raw.shape
    step, one = dtype(F(step)), dtype(1)
    trans, acc, col = np.ones(n_vertices, dtype), np.zeros(n_vertices, dtype), np.zeros((n_vertices, 3), dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(n_samples):
            sigma = np.where(raw[:, k, 3] < 0, dtype(0), raw[:, k, 3])      # a NaN stays
            alpha = one - np.exp(-(sigma * step))
            w = alpha * trans
            acc = acc + w
            col = col + w[:, None] * _sigmoid(raw[:, k, :3])
            trans = trans * (one - alpha)
        seen = acc >= dtype(F(min_opacity))
        colour = np.where(seen[:, None], col / np.where(seen, acc, one)[:, None], _sigmoid(raw[:, n_samples // 2, :3]))
    return colour, acc


def quantise(colours):
    """write_mesh's bytes of float colours: clip to [0, 1], times 255 in float32, truncate (cast_to_image); a NaN is 0."""
    c = np.asarray(colours)
    if c.dtype == np.uint8:
        return c
    c = np.where(np.isnan(c), 0, c).astype(F)
    return (np.minimum(np.maximum(c, F(0)), F(1)) * F(255)).astype(np.uint8)


def ply_bytes(vertices, faces, normals=None, colours_u8=None):
    """The .ply file write_mesh writes, built on its own."""
    v, f = np.asarray(vertices, dtype="<f4"), np.asarray(faces, dtype="<i4")
    names = ["x", "y", "z"] + ([] if normals is None else ["nx", "ny", "nz"])
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"] + [f"property float {p}" for p in names]
    if colours_u8 is not None:
        head += [f"property uchar {p}" for p in ("red", "green", "blue")]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    out = ("\n".join(head) + "\n").encode("ascii")
    for i in range(len(v)):
        out += struct.pack("<3f", *v[i].tolist())
        if normals is not None:
            out += struct.pack("<3f", *np.asarray(normals, dtype="<f4")[i].tolist())
        if colours_u8 is not None:
            out += struct.pack("<3B", *np.asarray(colours_u8)[i].tolist())
    for t in f.tolist():
        out += struct.pack("<B3i", 3, *t)
    return out


def read_ply(path):
    """A binary little-endian .ply of float (and, behind them, uchar) vertex properties and triangle faces -> (float rows (V, n) float32,
    faces (F, 3) int32, colours (V, 3) uint8 or None, the property names in file order)."""
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n_v = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    n_f = int([l for l in lines if l.startswith("element face")][0].split()[2])
    props = [l.split()[1:] for l in lines if l.startswith("property ") and not l.startswith("property list")]
    floats = [name for kind, name in props if kind == "float"]
    chars = [name for kind, name in props if kind == "uchar"]
    assert [name for _, name in props] == floats + chars and chars in ([], ["red", "green", "blue"])
    row = np.dtype([("f", "<f4", (len(floats),))] + ([("c", "u1", (3,))] if chars else []))
    vert = np.frombuffer(body, dtype=row, count=n_v)
    rest = body[n_v * row.itemsize:]
    assert len(rest) == 13 * n_f
    faces = np.frombuffer(rest, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]), count=n_f)
    assert (faces["n"] == 3).all()
    return vert["f"].copy(), faces["i"].astype(np.int32), vert["c"].copy() if chars else None, floats + chars


def read_obj(path):
    """-> (vertices (V, 3) float32, colours (V, 3) float32 or None, normals (V, 3) float32 or None, faces (F, 3) int32, 0-based)."""
    v, n, f = [], [], []
    for line in open(path).read().splitlines():
        tag, *rest = line.split()
        if tag == "v":
            v.append([float(x) for x in rest])
        elif tag == "vn":
            n.append([float(x) for x in rest])
        elif tag == "f":
            f.append([int(x.split("/")[0]) - 1 for x in rest])
    v = np.asarray(v, dtype=np.float64).reshape(len(v), -1)
    assert v.shape[1] in (3, 6)
    return (v[:, :3].astype(F), v[:, 3:].astype(F) if v.shape[1] == 6 else None, np.asarray(n, dtype=F).reshape(-1, 3) if n else None,
            np.asarray(f, dtype=np.int32).reshape(-1, 3))


def read_off(path):
    """-> (vertices (V, 3) float32, colours (V, 4) uint8 rgba or None, faces (F, 3) int32)."""
    lines = open(path).read().splitlines()
    assert lines[0] in ("OFF", "COFF")
    n_v, n_f, _ = (int(x) for x in lines[1].split())
    rows = [l.split() for l in lines[2:2 + n_v]]
    assert all(len(r) == (7 if lines[0] == "COFF" else 3) for r in rows)
    v = np.asarray([[float(x) for x in r[:3]] for r in rows], dtype=F).reshape(-1, 3)
    c = np.asarray([[int(x) for x in r[3:]] for r in rows], dtype=np.uint8).reshape(-1, 4) if lines[0] == "COFF" else None
    faces = np.asarray([[int(x) for x in l.split()] for l in lines[2 + n_v:2 + n_v + n_f]], dtype=np.int32).reshape(-1, 4)
    assert (faces[:, 0] == 3).all() and len(lines) == 2 + n_v + n_f
    return v, c, faces[:, 1:]
