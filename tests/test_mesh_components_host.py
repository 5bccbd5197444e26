"""CPU: the mesh-components specification as tests/mesh_components_ref.py restates it, against scipy's connected components; the
argument checks of the Python layer, which hold before a device is asked for; the new entry points in the header, the binding and
the library."""
import os
import re

import numpy as np
import pytest

from tests import mesh_components_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["nf_mesh_components_workspace_bytes", "nf_mesh_components_label", "nf_mesh_components_select", "nf_mesh_components_emit"]


random_faces = M.random_faces


def test_the_end_to_end_field_has_three_components_and_its_largest_is_the_sphere_alone():
    """The field of the GPU end-to-end test through tests/isosurface_ref.py: three components of 308 / 4,504 / 880 faces, and the
    largest one equals the extraction of the big sphere alone -- vertices and normals bit for bit, faces exactly (extraction is local
    and ids are ordered; the small spheres live in boxes that do not reach the big one's cells or their neighbours)."""
    from tests import isosurface_ref as R
    alone, both = M.e2e_fields(*R.grid_points(M.E2E_LO, M.E2E_HI, M.E2E_N))
    mesh = R.isosurface(both, 0.0, M.E2E_LO, M.E2E_HI, normals=True)
    want = R.isosurface(alone, 0.0, M.E2E_LO, M.E2E_HI, normals=True)
    assert M.mesh_components(mesh[1], mesh[0].shape[0])[2].tolist() == [308, 4504, 880]
    v, f, n, stats = M.filter_mesh(*mesh, largest=True)
    assert np.array_equal(v.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(n.view(np.uint32), want[2].view(np.uint32))
    assert np.array_equal(f, want[1]) and stats["kept_components"] == 1 and stats["components"] == 3
    assert M.filter_mesh(*mesh, min_faces=309)[3]["kept_components"] == 2 and M.filter_mesh(*mesh, min_faces=5000)[1].shape == (0, 3)


@pytest.mark.parametrize("n_vertices", [1, 7, 300])
def test_the_restatements_partition_is_scipys(n_vertices):
    """On seeded face lists of 0 .. 2V faces, some invalid and some with repeated indices: the partition equals
    scipy.sparse.csgraph.connected_components of the graph whose edges are the sides of the valid faces; the components are
    numbered by ascending smallest vertex; the counts are the numbers of valid faces and of vertices per label."""
    sparse = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    rng = np.random.default_rng(100 + n_vertices)
    some_invalid = some_repeated = False
    for n_faces in sorted({0, 1, 2, n_vertices // 2, n_vertices, 2 * n_vertices}):
        faces = random_faces(rng, n_vertices, n_faces)
        valid = M.valid_faces(faces, n_vertices)
        some_invalid |= bool((~valid).any())
        some_repeated |= bool((valid & ((faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]))).any())
        vertex_label, face_label, face_counts, vertex_counts = M.mesh_components(faces, n_vertices)
        tri = faces[valid].astype(np.int64)
        rows, cols = np.concatenate([tri[:, 0], tri[:, 0]]), np.concatenate([tri[:, 1], tri[:, 2]])
        graph = sparse.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n_vertices, n_vertices))
        n_components, want = csgraph.connected_components(graph, directed=False)
        assert len(face_counts) == len(vertex_counts) == n_components
        # the same partition: the pairs (ours, scipy's) are a bijection
        pairs = set(zip(vertex_label.tolist(), want.tolist()))
        assert len(pairs) == n_components and len({a for a, _ in pairs}) == n_components and len({b for _, b in pairs}) == n_components
        # numbering: label c's smallest vertex is the c-th of the ascending smallest vertices
        firsts = [int(np.flatnonzero(vertex_label == c)[0]) for c in range(n_components)]
        assert firsts == sorted(firsts) and vertex_label.dtype == face_label.dtype == face_counts.dtype == np.int32
        assert np.array_equal(face_label[valid], vertex_label[tri[:, 0]]) and (face_label[~valid] == -1).all()
        assert np.array_equal(face_counts, np.bincount(face_label[valid], minlength=n_components))
        assert np.array_equal(vertex_counts, np.bincount(vertex_label, minlength=n_components)) and vertex_counts.sum() == n_vertices
    assert n_vertices == 1 or (some_invalid and some_repeated)


def test_selection_and_compaction_of_the_restatement():
    """Two triangles sharing one vertex are one component; ties go to the lower label; all counts zero keeps nothing; the filtered
    mesh keeps order and bits and renumbers the indices."""
    faces = np.array([[5, 6, 7], [0, 1, 2], [2, 3, 4], [9, 9, 8], [1, -1, 2], [0, 1, 10]], dtype=np.int32)
    vertex_label, face_label, face_counts, vertex_counts = M.mesh_components(faces, 10)
    assert vertex_label.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 2, 2] and face_label.tolist() == [1, 0, 0, 2, -1, -1]
    assert face_counts.tolist() == [2, 1, 1] and vertex_counts.tolist() == [5, 3, 2]
    assert M.kept_components(np.array([3, 7, 7, 1]), largest=True).tolist() == [False, True, False, False]
    assert not M.kept_components(np.array([0, 0]), largest=True).any() and not M.kept_components(np.zeros(0, dtype=np.int32), largest=True).any()
    assert M.kept_components(np.array([3, 7, 0]), min_faces=3).tolist() == [True, True, False]
    vertices = np.arange(30, dtype=np.float32).reshape(10, 3)
    v, f, n, stats = M.filter_mesh(vertices, faces, vertices + 0.5, min_faces=1)
    assert np.array_equal(v, vertices) and np.array_equal(n, vertices + 0.5) and np.array_equal(f, faces[:4])
    v, f, n, stats = M.filter_mesh(vertices, faces[[0, 3]], None, min_faces=1)
    assert np.array_equal(v, vertices[5:]) and n is None and f.tolist() == [[0, 1, 2], [4, 4, 3]]
    assert stats == dict(components=7, kept_components=2, vertices=10, kept_vertices=5, faces=2, kept_faces=2)
    v, f, n, stats = M.filter_mesh(vertices, faces, None, min_faces=3)
    assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == np.int32 and stats["kept_components"] == 0


def test_argument_errors_are_raised_before_anything_touches_the_device(monkeypatch):
    """Both rules or neither, min_faces < 1, a wrong dtype or shape and normals of another shape are ValueErrors on CPU tensors, with
    the library never asked for (nothing is packed or launched); well-formed CPU tensors then meet the no-CPU-path guard."""
    import torch
    import nerf
    from nerf import _hip, ops
    monkeypatch.setattr(_hip, "lib", lambda: pytest.fail("the library must not be asked for"))
    v, f, n = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    bad = [((v, f, n), dict()), ((v, f, n), dict(largest=True, min_faces=2)), ((v, f, n), dict(min_faces=0)), ((v, f, n), dict(min_faces=-3)),
           ((v, f, n), dict(min_faces=1.5)), ((v, f.long(), n), dict(largest=True)), ((v.double(), f, None), dict(largest=True)),
           ((v, f.view(3, 2), n), dict(largest=True)), ((v.view(3, 4), f, None), dict(largest=True)), ((v, f, torch.zeros(5, 3)), dict(largest=True)),
           ((v, f, n.double()), dict(largest=True)), ((v.numpy(), f, n), dict(largest=True)), ((v, f, n), dict(largest=False))]
    for args, rule in bad:
        with pytest.raises(ValueError):
            ops.filter_mesh(*args, **rule)
        with pytest.raises(ValueError):
            nerf.filter_mesh(nerf.Mesh(*args), **rule)
    for faces, n_vertices in ((f.long(), 4), (f.view(-1), 4), (f, -1), (f, 2 ** 31), (f.numpy(), 4)):
        with pytest.raises(ValueError):
            ops.mesh_components(faces, n_vertices)
    with pytest.raises(ValueError):
        nerf.mesh_components((v.view(-1), f))
    with pytest.raises(ValueError):
        nerf.filter_mesh((v,), largest=True)
    m = nerf.models.ConditionalBlendshapePaperNeRFModel(num_encoding_fn_xyz=10, num_encoding_fn_dir=4, include_input_dir=False)
    box = dict(lo=(-1, -1, -1), hi=(1, 1, 1), resolution=4, level=0.0)
    for rule in (dict(largest=True, min_faces=2), dict(min_faces=0), dict(min_faces=2.5)):
        with pytest.raises(ValueError, match="rule"):
            nerf.extract_mesh(m, torch.zeros(76), torch.zeros(32), **box, **rule)
    for call in (lambda: ops.filter_mesh(v, f, n, largest=True), lambda: ops.mesh_components(f, 4), lambda: nerf.filter_mesh(nerf.Mesh(v, f, None), min_faces=1),
                 lambda: nerf.mesh_components(nerf.Mesh(v, f, n))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    assert ops.MeshComponents._fields == ("vertex_label", "face_label", "face_counts", "vertex_counts")
    assert ops.MeshFilterStats._fields == ("components", "kept_components", "vertices", "kept_vertices", "faces", "kept_faces")
    assert nerf.Mesh._fields == ("vertices", "faces", "normals")


def test_the_launcher_takes_one_rule_at_most(capsys):
    from launch import extract_mesh
    base = ["--config", "c.yml", "--checkpoint", "ck", "--frame", "0", "--level", "1", "--resolution", "8", "--out", "m.ply"]
    for extra in (["--largest", "--min-faces", "3"], ["--min-faces", "0"], ["--min-faces", "-2"]):
        with pytest.raises(SystemExit) as e:
            extract_mesh.main(base + extra)
        assert e.value.code == 2
    capsys.readouterr()


def test_new_entry_points_are_declared_prototyped_and_exported(hip_lib):
    """The nf_mesh_components_* family of include/nerface_hip.h is the one the binding has prototypes for, argument for argument, and
    the library exports it; the ABI revision is still 5."""
    import ctypes as C
    from nerf import _hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerface_hip.h")).read(), flags=re.S)
    declared = dict(re.findall(r"^(?:int|size_t)\s+(nf_mesh_components_\w+)\(([^;]*)\);", header, re.M))
    assert sorted(declared) == sorted(ENTRY_POINTS)
    ctype = lambda arg: C.c_void_p if "*" in arg or "nf_stream_t" in arg else {"int64_t": C.c_int64, "size_t": C.c_size_t, "int": C.c_int}[arg.split()[0]]
    for name, args in declared.items():
        assert name in _hip._PROTOTYPES and name not in _hip._OPTIONAL and hasattr(hip_lib, name), name
        res, argtypes = _hip._PROTOTYPES[name]
        assert argtypes == [ctype(a.strip()) for a in args.split(",")], name
        assert res is (C.c_size_t if name.endswith("workspace_bytes") else C.c_int)
    assert _hip.ABI_VERSION == 5 and hip_lib.nf_abi_version() == 5
    assert "nf_mesh_components.hip" in open(os.path.join(ROOT, "4d-facial-avatars_amd", "build.py")).read()


def test_entry_points_refuse_before_touching_the_device(hip_lib):
    """The size query answers 0 outside [0, 2^31) and grows with V and F; NF_EINVAL (-22) for NULL pointers, an unserved size, a
    workspace that is too small, both rules or neither, negative min_faces or capacities, normals on one side only.  The pointers
    handed over are never dereferenced on these paths, so a small integer stands in for device memory."""
    ws_bytes = hip_lib.nf_mesh_components_workspace_bytes
    assert ws_bytes(-1, 4) == 0 and ws_bytes(4, -1) == 0 and ws_bytes(2 ** 31, 4) == 0 and ws_bytes(4, 2 ** 31) == 0
    assert ws_bytes(0, 0) >= 256 and ws_bytes(2 ** 31 - 1, 2 ** 31 - 1) >= 8 * (2 ** 31 - 1)
    n = ws_bytes(1000, 3000)
    assert n % 256 == 0 and 256 + 8 * 1000 <= n <= 256 + 8 * 1000 + 6 * 256
    P = 4096
    label, select, emit = hip_lib.nf_mesh_components_label, hip_lib.nf_mesh_components_select, hip_lib.nf_mesh_components_emit
    ok = dict(faces=P, n_vertices=1000, n_faces=3000, ws=P, ws_bytes=n, vertex_label=P, face_label=P, face_counts=P, vertex_counts=P, counts=P, stream=None)
    for change in (dict(faces=None), dict(ws=None), dict(vertex_label=None), dict(face_label=None), dict(face_counts=None), dict(vertex_counts=None),
                   dict(counts=None), dict(ws_bytes=n - 1), dict(n_vertices=-1), dict(n_faces=-1), dict(n_vertices=2 ** 31, ws_bytes=1 << 40)):
        assert label(*{**ok, **change}.values()) == -22, change
    ok = dict(vertex_label=P, face_label=P, face_counts=P, n_vertices=1000, n_faces=3000, largest=1, min_faces=0, ws=P, ws_bytes=n, counts=P, stream=None)
    for change in (dict(vertex_label=None), dict(face_label=None), dict(face_counts=None), dict(ws=None), dict(counts=None), dict(ws_bytes=n - 1),
                   dict(largest=0), dict(min_faces=5), dict(largest=0, min_faces=-1), dict(n_faces=2 ** 31, ws_bytes=1 << 40)):
        assert select(*{**ok, **change}.values()) == -22, change
    ok = dict(vertices=P, faces=P, normals=P, vertex_label=P, face_label=P, face_counts=P, n_vertices=1000, n_faces=3000, ws=P, ws_bytes=n, out_v=P,
              cap_v=10, out_f=P, cap_f=10, out_n=P, stream=None)
    for change in (dict(vertices=None), dict(faces=None), dict(vertex_label=None), dict(face_label=None), dict(face_counts=None), dict(ws=None),
                   dict(ws_bytes=n - 1), dict(out_v=None), dict(out_f=None), dict(normals=None), dict(out_n=None), dict(cap_v=-1), dict(cap_f=-1),
                   dict(cap_v=2 ** 31), dict(n_vertices=-5)):
        assert emit(*{**ok, **change}.values()) == -22, change
