"""CPU: the mesh-decimation specification as tests/mesh_decimate_ref.py restates it -- against a second, deliberately naive
implementation (Python dicts, Python integers for the fixed-point sums), on the isosurface cases DESIGN.md "Mesh decimation" lists;
the workspace plan and the refusals of the entry points, which need no device; the new symbols in the header, the binding and the
library; the argument checks of the Python layers, which hold before a device is asked for."""
import math
import os
import re

import numpy as np
import pytest

from tests import isosurface_ref as R
from tests import mesh_decimate_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["nf_mesh_decimate_workspace_bytes", "nf_mesh_decimate_count", "nf_mesh_decimate_emit"]
ISO_N, ISO_LO, ISO_HI, ISO_ORIGIN, ISO_H = (33, 33, 33), (-1, -1, -1), (1, 1, 1), (-1.03, -1.01, -1.02), 2.0 / 32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the restatement against a naive implementation
def _naive(vertices, faces, cell, origin):
    """The specification once more, vertex by vertex and face by face: dicts for the cells and the vertex sets, Python integers for S,
    Python floats (IEEE double, every operation rounded on its own) for the position."""
    p = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    o, c = D._three(origin), D._three(cell)
    n_vertices = len(p)
    t, i, cluster = {}, {}, {}
    with np.errstate(all="ignore"):
        for v in range(n_vertices):
            ts = [np.float32(np.float32(p[v, a] - o[a]) / c[a]) for a in range(3)]
            if all(math.isfinite(float(x)) and -2 ** 20 <= math.floor(float(x)) < 2 ** 20 for x in ts):
                t[v], i[v] = ts, [math.floor(float(x)) for x in ts]
                cluster.setdefault(tuple(i[v]), []).append(v)
    rep, members = list(range(n_vertices)), [1] * n_vertices
    for group in cluster.values():
        for v in group:
            rep[v], members[v] = min(group), len(group)
    invalid = degenerate = 0
    sets = {}
    for f, (a, b, cc) in enumerate(np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist()):
        if not all(0 <= x < n_vertices for x in (a, b, cc)):
            invalid += 1
            continue
        r = (rep[a], rep[b], rep[cc])
        if len(set(r)) < 3:
            degenerate += 1
            continue
        inversions = (r[0] > r[1]) + (r[0] > r[2]) + (r[1] > r[2])
        sets.setdefault(frozenset(r), ([], []))[inversions % 2].append((f, r))
    kept = []
    for even, odd in sets.values():
        if len(even) != len(odd):
            kept.append(min(even if len(even) > len(odd) else odd))
    kept.sort()
    used = sorted({u for _, r in kept for u in r})
    new_id = {u: k for k, u in enumerate(used)}
    out = np.zeros((len(used), 3), dtype=np.float32)
    for k, u in enumerate(used):
        out[k] = p[u]
        if members[u] > 1:
            group = cluster[tuple(i[u])]
            for a in range(3):
                total = 0
                for v in group:
                    frac = np.float32(t[v][a] - np.float32(i[v][a]))
                    total += int(float(frac) * 2.0 ** 30)
                m = float(total) / float(len(group))
                out[k, a] = np.float32(float(o[a]) + float(c[a]) * (float(i[u][a]) + m * 2.0 ** -30))
    vertex_map = np.array([new_id.get(rep[v], -1) for v in range(n_vertices)], dtype=np.int32)
    out_faces = np.array([[new_id[u] for u in r] for _, r in kept], dtype=np.int32).reshape(-1, 3)
    stats = dict(vertices=n_vertices, kept_vertices=len(used), faces=len(faces), kept_faces=len(kept), degenerate_faces=degenerate,
                 coincident_faces=sum(len(e) + len(od) for e, od in sets.values()) - len(kept), invalid_faces=invalid,
                 unclustered_vertices=n_vertices - len(t), largest_cluster=max(members) if members else 0)
    return out, out_faces, vertex_map, stats


@pytest.mark.parametrize("n_vertices", [1, 7, 300])
def test_the_restatement_equals_the_naive_implementation(n_vertices):
    """Seeded meshes of 0 .. 2V faces with invalid and repeated indices, NaN and infinite vertices, coordinates at and past either end
    of the cell range, negative coordinates with the default origin, faces listed again rotated and swapped; three lattices."""
    rng = np.random.default_rng(400 + n_vertices)
    seen = dict(invalid=False, degenerate=False, coincident=False, unclustered=False, merged=False, dropped=False, negative=False)
    for n_faces in sorted({0, 1, 2, n_vertices // 2, n_vertices, 2 * n_vertices}):
        for cell, origin in ((1.0, (0.0, 0.0, 0.0)), ((0.75, 1.5, 0.4), (0.0, 0.0, 0.0)), (0.5, (-0.3, 0.2, 1.1))):
            v, f = D.random_mesh(rng, n_vertices, n_faces, cell=cell, origin=origin)
            got = D.decimate(v, f, cell, origin)
            want = _naive(v, f, cell, origin)
            assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[3].dtype == np.int32 and got[2] is None
            assert got[0].shape == want[0].shape and np.array_equal(_bits(got[0]), _bits(want[0])), (n_faces, cell)
            assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1]), (n_faces, cell)
            assert np.array_equal(got[3], want[2]) and got[4] == want[3], (n_faces, cell, got[4], want[3])
            st = got[4]
            seen["invalid"] |= st["invalid_faces"] > 0
            seen["degenerate"] |= st["degenerate_faces"] > 0
            seen["coincident"] |= st["coincident_faces"] > 0
            seen["unclustered"] |= st["unclustered_vertices"] > 0
            seen["merged"] |= st["largest_cluster"] > 2 and st["kept_vertices"] > 0
            seen["dropped"] |= bool((got[3] == -1).any()) and st["kept_vertices"] > 0
            seen["negative"] |= bool((v[np.isfinite(v).all(axis=1)] < 0).any()) and origin == (0.0, 0.0, 0.0)
            assert st["kept_faces"] + st["coincident_faces"] + st["degenerate_faces"] + st["invalid_faces"] == n_faces
    assert n_vertices < 300 or all(seen.values()), seen


def test_the_coincidence_rule_by_hand():
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5], [0.6, 0.6, 0.6]], dtype=np.float32)
    run = lambda faces: D.decimate(v, np.array(faces, dtype=np.int32).reshape(-1, 3), 1.0)
    assert run([(0, 1, 2), (0, 2, 1)])[1].shape == (0, 3) and run([(0, 1, 2), (0, 2, 1)])[4]["coincident_faces"] == 2
    assert run([(1, 2, 0), (0, 1, 2)])[1].tolist() == [[1, 2, 0]] and run([(1, 2, 0), (0, 1, 2)])[4]["coincident_faces"] == 1
    out = run([(0, 2, 1), (1, 2, 4), (2, 0, 1)])                     # odd, even (4 is in 0's cell), even: the smaller even id stays, with its own order
    assert out[1].tolist() == [[1, 2, 0]] and out[3].tolist() == [0, 1, 2, -1, 0] and out[4]["largest_cluster"] == 2
    assert np.array_equal(_bits(out[0][1:]), _bits(v[1:3])) and out[0][0].tolist() == pytest.approx([0.55, 0.55, 0.55], abs=1e-6)
    assert run([(0, 4, 1)])[4] == dict(vertices=5, kept_vertices=0, faces=1, kept_faces=0, degenerate_faces=1, coincident_faces=0, invalid_faces=0,
                                       unclustered_vertices=0, largest_cluster=2)
    assert run([(0, 4, 1)])[3].tolist() == [-1] * 5


# ---- 2. the isosurface cases of the specification
SIZES = {"sphere": ((7118, 14232), {1: (1753, 3504), 2: (515, 1026), 3.7: (164, 324), 8: (38, 72), 100: (0, 0)}, {1: 11, 2: 36, 3.7: 116, 8: 401}),
         "torus": ((5436, 10872), {1: (1355, 2710), 100: (0, 0)}, {}),
         "two_spheres": (None, {100: (0, 0)}, {})}


@pytest.mark.parametrize("field", list(SIZES))
def test_the_isosurface_cases_of_the_specification(field):
    """33^3 over [-1, 1]^3, origin (-1.03, -1.01, -1.02), cell = k h: the sizes DESIGN.md lists, the Euler characteristic of the input
    in every case, every output vertex inside its cell's box within 4 float32 ulps of the coordinate."""
    v, f, _ = R.isosurface(getattr(R, field)(*R.grid_points(ISO_LO, ISO_HI, ISO_N)), 0.0, ISO_LO, ISO_HI)
    size, kept, largest = SIZES[field]
    before = R.mesh_report(v, f)
    assert before["closed"] and (size is None or (len(v), len(f)) == size)
    for k in (1, 2, 3.7, 8, 100):
        cell = k * ISO_H
        out_v, out_f, _, vertex_map, stats = D.decimate(v, f, cell, ISO_ORIGIN)
        assert stats["invalid_faces"] == 0 and stats["unclustered_vertices"] == 0
        if k in kept:
            assert (len(out_v), len(out_f)) == kept[k], (field, k)
        if k in largest:
            assert stats["largest_cluster"] == largest[k], (field, k)
        if k == 100:
            assert stats["largest_cluster"] == len(v) and (vertex_map == -1).all()
            continue
        after = R.mesh_report(out_v, out_f)
        assert after["chi"] == before["chi"] and after["unreferenced"] == 0, (field, k, after)
        members = np.flatnonzero(vertex_map >= 0)
        first = np.full(len(out_v), len(v), dtype=np.int64)
        np.minimum.at(first, vertex_map[members], members)             # a member of every kept cluster: its cell is the cluster's
        lo, hi = D.cell_boxes(v[first], ISO_ORIGIN, cell)
        slack = 4 * np.spacing(np.abs(out_v)).astype(np.float64)
        assert (out_v >= lo - slack).all() and (out_v <= hi + slack).all(), (field, k)


# ---- 3. the Python layers refuse before a device is asked for
def test_argument_errors_are_raised_before_anything_touches_the_device(monkeypatch):
    import torch
    import nerf
    from nerf import _hip, ops
    monkeypatch.setattr(_hip, "lib", lambda: pytest.fail("the library must not be asked for"))
    v, f, n = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    nan, inf = float("nan"), float("inf")
    bad = [((v, f, n), dict(cell=0.0)), ((v, f, n), dict(cell=-1.0)), ((v, f, n), dict(cell=nan)), ((v, f, n), dict(cell=inf)), ((v, f, n), dict(cell=(1.0, 2.0))),
           ((v, f, n), dict(cell=(1.0, 0.0, 1.0))), ((v, f, n), dict(cell="1")), ((v, f, n), dict(cell=True)), ((v, f, n), dict(cell=None)),
           ((v, f, n), dict(cell=1e-50)), ((v, f, n), dict(cell=1.0, origin=(0.0, nan, 0.0))), ((v, f, n), dict(cell=1.0, origin=(0.0, inf, 0.0))),
           ((v, f, n), dict(cell=1.0, origin=0.0)), ((v, f, n), dict(cell=1.0, origin=(0.0, 0.0))), ((v, f.long(), n), dict(cell=1.0)),
           ((v.double(), f, None), dict(cell=1.0)), ((v, f.view(3, 2), n), dict(cell=1.0)), ((v.view(3, 4), f, None), dict(cell=1.0)),
           ((v, f, torch.zeros(5, 3)), dict(cell=1.0)), ((v, f, n.double()), dict(cell=1.0)), ((v.numpy(), f, n), dict(cell=1.0))]
    for args, kw in bad:
        with pytest.raises(ValueError):
            ops.decimate_mesh(*args, **kw)
        with pytest.raises(ValueError):
            nerf.decimate_mesh(nerf.Mesh(*args), **kw)
    with pytest.raises(TypeError):
        ops.decimate_mesh(v, f, n)                                   # cell has no default
    with pytest.raises(ValueError):
        nerf.decimate_mesh((v,), cell=1.0)
    m = nerf.models.ConditionalBlendshapePaperNeRFModel(num_encoding_fn_xyz=10, num_encoding_fn_dir=4, include_input_dir=False)
    box = dict(lo=(-1, -1, -1), hi=(1, 1, 1), resolution=4, level=0.0)
    for k in (0, -1, nan, inf, True, "2"):
        with pytest.raises(ValueError, match="decimate"):
            nerf.extract_mesh(m, torch.zeros(76), torch.zeros(32), **box, decimate=k)
    for call in (lambda: ops.decimate_mesh(v, f, n, cell=1.0), lambda: ops.decimate_mesh(v, f, cell=(1.0, 2.0, 3.0), origin=(-1.0, 0.0, 1.0)),
                 lambda: nerf.decimate_mesh(nerf.Mesh(v, f, None), cell=0.5), lambda: nerf.decimate_mesh((v, f), cell=0.5)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    assert ops.MeshDecimateStats._fields == ("vertices", "kept_vertices", "faces", "kept_faces", "degenerate_faces", "coincident_faces", "invalid_faces",
                                             "unclustered_vertices", "largest_cluster")
    assert "decimate_mesh(mesh" in nerf.mesh.__doc__ and nerf.decimate_mesh is nerf.mesh.decimate_mesh
    assert nerf.mesh.decimation_lattice((-1, 0, 1), (1, 4, 2), (5, 9, 3), 2.5) == ([1.25, 1.25, 1.25], [-1.0, 0.0, 1.0])


def test_the_launcher_refuses_bad_decimation_arguments(capsys):
    from launch import extract_mesh
    base = ["--config", "c.yml", "--checkpoint", "ck", "--frame", "0", "--level", "1", "--resolution", "8", "--out", "m.ply"]
    for extra in (["--decimate", "0"], ["--decimate", "-2"], ["--decimate", "nan"], ["--decimate", "inf"], ["--decimate", "x"]):
        with pytest.raises(SystemExit) as e:
            extract_mesh.main(base + extra)
        assert e.value.code == 2
    capsys.readouterr()
    with pytest.raises(SystemExit):
        extract_mesh.main(["--help"])
    text = capsys.readouterr().out
    assert "--decimate K" in text and "how far the true surface can lie from a clustered vertex" in " ".join(text.split())


# ---- 4. the library: symbols, the plan, the refusals
def test_new_entry_points_are_declared_prototyped_and_exported(hip_lib):
    import ctypes as C
    from nerf import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerface_hip.h")).read(), flags=re.S)
    declared = dict(re.findall(r"^(?:int|size_t)\s+(nf_mesh_decimate_\w+)\(([^;]*)\);", header, re.M))
    assert sorted(declared) == sorted(ENTRY_POINTS)
    ctype = lambda arg: C.c_void_p if "*" in arg or "nf_stream_t" in arg else {"int64_t": C.c_int64, "size_t": C.c_size_t, "int": C.c_int,
                                                                                "float": C.c_float}[arg.split()[0]]
    for name, args in declared.items():
        assert name in _hip._PROTOTYPES and name not in _hip._OPTIONAL and hasattr(hip_lib, name), name
        res, argtypes = _hip._PROTOTYPES[name]
        assert argtypes == [ctype(a.strip()) for a in args.split(",")], name
        assert res is (C.c_size_t if name.endswith("workspace_bytes") else C.c_int)
    assert _hip.ABI_VERSION == 5 and hip_lib.nf_abi_version() == 5
    assert "nf_mesh_decimate.hip" in open(os.path.join(ROOT, "4d-facial-avatars_amd", "build.py")).read()
    text = open(os.path.join(ROOT, "include", "nerface_hip.h")).read()
    assert 'DESIGN.md "Mesh decimation"' in text and "### Mesh decimation" in open(os.path.join(ROOT, "DESIGN.md")).read()


def _capacity(n):
    cap = 1
    while cap < 2 * max(n, 128):
        cap *= 2
    return cap


def _layout_bytes(n_vertices, n_faces):
    """The workspace layout of DESIGN.md "Mesh decimation": a header of 256 bytes, then parts of whole 256 bytes."""
    up = lambda b: (b + 255) // 256 * 256
    blocks = lambda n: (n + 255) // 256
    cv, cf = _capacity(n_vertices), _capacity(n_faces)
    parts = [8 * n_vertices, 4 * n_vertices, 4 * n_vertices, 24 * n_vertices, 4 * n_vertices, 4 * n_vertices, 4 * blocks(n_vertices), 4 * cv, 4 * cv, 4 * cv,
             12 * n_faces, 4 * n_faces, 4 * n_faces, 4 * blocks(n_faces), 4 * cf, 8 * cf, 8 * cf]
    return 256 + sum(up(b) for b in parts)


def test_the_workspace_plan(hip_lib):
    """At least the header; monotone in V and in F; 0 past 2^30 and below 0; both tables hold the smallest power of two >= 2 max(n, 128)
    slots, which the layout's byte count pins (a vertex slot takes 12 bytes, a face slot 20)."""
    ws_bytes = hip_lib.nf_mesh_decimate_workspace_bytes
    assert [_capacity(n) for n in (0, 1, 128, 129, 256, 257, 4096, 65536, 2 ** 20 + 257, 2 ** 30)] == [256, 256, 256, 512, 512, 1024, 8192, 131072, 2 ** 22, 2 ** 31]
    assert ws_bytes(0, 0) == _layout_bytes(0, 0) >= 256 and ws_bytes(0, 0) % 256 == 0
    assert ws_bytes(-1, 4) == 0 and ws_bytes(4, -1) == 0 and ws_bytes(2 ** 30 + 1, 4) == 0 and ws_bytes(4, 2 ** 30 + 1) == 0 and ws_bytes(2 ** 31, 2 ** 31) == 0
    assert ws_bytes(2 ** 30, 2 ** 30) == _layout_bytes(2 ** 30, 2 ** 30)
    sizes = [0, 1, 5, 127, 128, 129, 255, 256, 257, 1000, 4096, 4097, 65536, 65537, 2 ** 20 + 257, 2 ** 24]
    for n_vertices in sizes:
        row = [ws_bytes(n_vertices, n_faces) for n_faces in sizes]
        assert row == [_layout_bytes(n_vertices, n_faces) for n_faces in sizes], n_vertices
        assert all(a <= b for a, b in zip(row, row[1:])) and all(ws_bytes(n_vertices, n) >= ws_bytes(m, n) for m in sizes if m <= n_vertices for n in (0, 1000))
    assert ws_bytes(129, 0) - ws_bytes(128, 0) >= 12 * 256 and ws_bytes(0, 129) - ws_bytes(0, 128) >= 20 * 256       # the tables double there


def test_entry_points_refuse_before_touching_the_device(hip_lib):
    """NF_EINVAL (-22) for NULL pointers where a size needs the buffer, an unserved size, a workspace that is too small, a cell that is
    NaN, infinite, zero or negative, an origin that is NaN or infinite, output sizes no count can have found.  The device pointers
    handed over are never dereferenced on these paths, so a small integer stands in for device memory."""
    import ctypes as C
    n = hip_lib.nf_mesh_decimate_workspace_bytes(1000, 3000)
    P = 4096
    nan, inf = float("nan"), float("inf")
    three = lambda *x: C.addressof(three.keep.setdefault(x, (C.c_float * 3)(*x)))
    three.keep = {}
    origin, cell = three(0.0, 0.0, 0.0), three(0.5, 0.5, 0.5)
    bad_cells = [three(*x) for x in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, nan), (inf, 1.0, 1.0), (1.0, -inf, 1.0), (-0.0, 1.0, 1.0))]
    bad_origins = [three(*x) for x in ((nan, 0.0, 0.0), (0.0, inf, 0.0), (0.0, 0.0, -inf))]
    count, emit = hip_lib.nf_mesh_decimate_count, hip_lib.nf_mesh_decimate_emit
    ok = dict(vertices=P, faces=P, n_vertices=1000, n_faces=3000, origin=origin, cell=cell, ws=P, ws_bytes=n, counts=P, stream=None)
    changes = [dict(vertices=None), dict(faces=None), dict(origin=None), dict(cell=None), dict(ws=None), dict(counts=None), dict(ws_bytes=n - 1),
               dict(ws_bytes=0), dict(n_vertices=-1), dict(n_faces=-1), dict(n_vertices=2 ** 30 + 1, ws_bytes=1 << 50), dict(n_faces=2 ** 30 + 1, ws_bytes=1 << 50)]
    changes += [dict(cell=c) for c in bad_cells] + [dict(origin=o) for o in bad_origins]
    for change in changes:
        assert count(*{**ok, **change}.values()) == -22, change
    ok = dict(vertices=P, faces=P, n_vertices=1000, n_faces=3000, origin=origin, cell=cell, ws=P, ws_bytes=n, out_vertices=P, n_out_vertices=10, out_faces=P,
              n_out_faces=12, vertex_map=P, stream=None)
    changes = [dict(vertices=None), dict(faces=None), dict(origin=None), dict(cell=None), dict(ws=None), dict(out_vertices=None), dict(out_faces=None),
               dict(vertex_map=None), dict(ws_bytes=n - 1), dict(n_vertices=-1), dict(n_faces=-1), dict(n_vertices=2 ** 30 + 1, ws_bytes=1 << 50),
               dict(n_out_vertices=-1), dict(n_out_faces=-1), dict(n_out_vertices=1001), dict(n_out_faces=3001)]
    changes += [dict(cell=c) for c in bad_cells] + [dict(origin=o) for o in bad_origins]
    for change in changes:
        assert emit(*{**ok, **change}.values()) == -22, change
    # no vertices: nothing can be kept, and nothing is launched or read
    empty = dict(vertices=None, faces=P, n_vertices=0, n_faces=3, origin=origin, cell=cell, ws=P, ws_bytes=hip_lib.nf_mesh_decimate_workspace_bytes(0, 3),
                 out_vertices=None, n_out_vertices=0, out_faces=None, n_out_faces=0, vertex_map=None, stream=None)
    assert emit(*empty.values()) == 0 and emit(*{**empty, "n_out_faces": 1, "out_faces": P}.values()) == -22
