"""Connected components and mesh filtering on the GPU: ops.mesh_components / ops.filter_mesh and the C entry points against
tests/mesh_components_ref.py -- integers and copied floats only, so every comparison is array_equal -- on hand meshes, deep and
contended union-find inputs, many components across workgroup and scan-round boundaries, ties, the isosurface of a known field,
poisoned buffers, and the model-level functions (nerf.filter_mesh, nerf.extract_mesh, launch.extract_mesh).  GPU only."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from oracle import cases as C
from tests import isosurface_ref as R
from tests import mesh_components_ref as M
from tests import util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 256                    # nfc::THREADS: vertices or faces per workgroup, one block sum each
SCAN_ROUND = 4 * 1024          # k_mc_scan: block sums per round of its one workgroup (SCAN_PER_THREAD * SCAN_THREADS)
SCAN_CAPACITY = SCAN_ROUND * BLOCK     # vertices (or faces) whose block sums one round takes: 2^20


def test_the_constants_above_are_the_kernels_own():
    shared, unit = (open(os.path.join(ROOT, "4d-facial-avatars_amd", "csrc", f)).read() for f in ("nf_scan_dev.h", "nf_mesh_components.hip"))
    assert "constexpr int THREADS = 256;" in shared and "constexpr int SCAN_THREADS = 1024;" in shared and "constexpr int SCAN_PER_THREAD = 4;" in unit
    assert SCAN_CAPACITY == 1 << 20


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _vertices(n_vertices, seed=1):
    """Seeded float32 rows with a few special bit patterns (NaN payloads, -0, inf, denormals): rows are copied, never computed on."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n_vertices, 3)).astype(np.float32)
    special = np.array([0x7FC0BEEF, 0x80000000, 0x7F800000, 0x00000001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    if n_vertices:
        v.reshape(-1)[:: 7] = np.resize(special, v.reshape(-1)[:: 7].shape)
    return v


def _check_components(gpu, faces, n_vertices, what):
    """ops.mesh_components == the restatement, all four arrays; returns the restatement's."""
    from nerf import ops
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    got = ops.mesh_components(torch.from_numpy(faces).to(gpu), n_vertices)
    want = M.mesh_components(faces, n_vertices)
    assert isinstance(got, ops.MeshComponents)
    for name, g, w in zip(got._fields, got, want):
        assert g.dtype == torch.int32 and g.is_cuda and g.dim() == 1, (what, name)
        assert g.shape == w.shape and np.array_equal(g.cpu().numpy(), w), (what, name)
    return want


def _check_filter(gpu, vertices, faces, normals, what, **rule):
    """ops.filter_mesh == the restatement: vertex and normal rows bit for bit, faces and stats exactly; returns the device result."""
    from nerf import ops
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    got = ops.filter_mesh(dev(vertices), dev(faces), dev(normals), **rule)
    want = M.filter_mesh(vertices, faces, normals, **rule)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[0].is_cuda and got[1].is_cuda
    assert tuple(got[0].shape) == want[0].shape and tuple(got[1].shape) == want[1].shape and got[0].shape[1] == 3 and got[1].shape[1] == 3, (what, rule)
    assert np.array_equal(_bits(got[0].cpu().numpy()), _bits(want[0])), (what, rule)
    assert np.array_equal(got[1].cpu().numpy(), want[1]), (what, rule)
    if normals is None:
        assert got[2] is None and want[2] is None
    else:
        assert got[2].shape == got[0].shape and np.array_equal(_bits(got[2].cpu().numpy()), _bits(want[2])), (what, rule)
    assert isinstance(got[3], ops.MeshFilterStats) and got[3]._asdict() == want[3], (what, rule, got[3], want[3])
    return got


def _check_all(gpu, faces, n_vertices, what, rules=(dict(largest=True), dict(min_faces=1), dict(min_faces=2))):
    want = _check_components(gpu, faces, n_vertices, what)
    v = _vertices(n_vertices)
    for k, rule in enumerate(rules):
        _check_filter(gpu, v, faces, None if k == 1 else -v, what, **rule)
    return want


# ---- 1. hand meshes
HAND = {
    "nothing": (0, []),
    "five vertices, no face": (5, []),
    "faces over no vertex": (0, [(0, 0, 0), (0, 1, 2)]),
    "one triangle": (3, [(2, 0, 1)]),
    "two triangles sharing one vertex": (5, [(3, 4, 2), (0, 1, 2)]),
    "two disjoint triangles, unused vertices between": (10, [(7, 8, 9), (0, 1, 2)]),
    "a repeated index": (4, [(1, 1, 3)]),
    "all three the same": (3, [(2, 2, 2)]),
    "faces holding -1 and V": (6, [(0, 1, 2), (2, -1, 3), (3, 4, 6), (4, 5, 4), (6, 6, 6), (-1, -1, -1)]),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_meshes(hip_lib, gpu, name):
    n_vertices, faces = HAND[name]
    vertex_label, face_label, face_counts, vertex_counts = _check_all(gpu, faces, n_vertices, name)
    expect = {"nothing": ([], []), "five vertices, no face": ([0, 1, 2, 3, 4], []), "faces over no vertex": ([], [-1, -1]),
              "one triangle": ([0, 0, 0], [0]), "two triangles sharing one vertex": ([0] * 5, [0, 0]),
              "two disjoint triangles, unused vertices between": ([0, 0, 0, 1, 2, 3, 4, 5, 5, 5], [5, 0]),
              "a repeated index": ([0, 1, 2, 1], [1]), "all three the same": ([0, 1, 2], [2]),
              "faces holding -1 and V": ([0, 0, 0, 1, 2, 2], [0, -1, -1, 2, -1, -1])}[name]
    assert vertex_label.tolist() == expect[0] and face_label.tolist() == expect[1]


def test_invalid_faces_leave_their_neighbours_components_alone(hip_lib, gpu):
    """The mesh with faces holding -1 and V labels its vertices as the mesh without them; the invalid faces are never kept."""
    from nerf import ops
    n_vertices, faces = HAND["faces holding -1 and V"]
    faces = np.array(faces, dtype=np.int32)
    valid = M.valid_faces(faces, n_vertices)
    assert valid.tolist() == [True, False, False, True, False, False]
    with_invalid = ops.mesh_components(torch.from_numpy(faces).to(gpu), n_vertices)
    without = ops.mesh_components(torch.from_numpy(faces[valid]).to(gpu), n_vertices)
    assert torch.equal(with_invalid.vertex_label, without.vertex_label) and torch.equal(with_invalid.face_counts, without.face_counts)
    assert with_invalid.face_counts.tolist() == [1, 0, 1]
    _, kept, _, stats = ops.filter_mesh(torch.from_numpy(_vertices(n_vertices)).to(gpu), torch.from_numpy(faces).to(gpu), min_faces=1)
    assert kept.cpu().tolist() == [[0, 1, 2], [3, 4, 3]] and stats.kept_faces == 2 and stats.kept_vertices == 5 and stats.components == 3


# ---- 2. depth, 3. contention
STRIP_V = 4099


@pytest.mark.parametrize("order", ["ascending", "descending", "permuted"])
def test_a_long_strip_is_one_component(hip_lib, gpu, order):
    """A triangle strip over 4,099 vertices (17 workgroups): ids ascending along the strip, descending (the longest find paths when the
    larger root goes under the smaller) and under a seeded permutation; the faces are shuffled too."""
    rng = np.random.default_rng(17)
    ids = {"ascending": np.arange(STRIP_V), "descending": np.arange(STRIP_V)[::-1], "permuted": rng.permutation(STRIP_V)}[order]
    at = np.arange(STRIP_V - 2)
    faces = np.stack([ids[at], ids[at + 1], ids[at + 2]], axis=1).astype(np.int32)
    if order == "permuted":
        faces = faces[rng.permutation(len(faces))]
    vertex_label, face_label, face_counts, vertex_counts = _check_all(gpu, faces, STRIP_V, f"strip {order}", rules=(dict(largest=True),))
    assert not vertex_label.any() and not face_label.any() and face_counts.tolist() == [STRIP_V - 2] and vertex_counts.tolist() == [STRIP_V]


@pytest.mark.parametrize("hub", ["first", "last"])
def test_a_fan_round_one_hub(hip_lib, gpu, hub):
    """3,000 faces that all hold one hub vertex: every union meets at the hub's parent word.  Hub id 0, then V - 1."""
    n_faces = 3000
    n_vertices = n_faces + 2
    ring = np.arange(n_faces + 1) + (1 if hub == "first" else 0)
    centre = 0 if hub == "first" else n_vertices - 1
    faces = np.stack([np.full(n_faces, centre), ring[:-1], ring[1:]], axis=1).astype(np.int32)
    vertex_label, face_label, face_counts, vertex_counts = _check_all(gpu, faces, n_vertices, f"fan, hub {hub}", rules=(dict(largest=True),))
    assert not vertex_label.any() and face_counts.tolist() == [n_faces] and vertex_counts.tolist() == [n_vertices]


# ---- 4. many components across workgroup and scan-round boundaries
def test_many_components_across_block_and_scan_round_boundaries(hip_lib, gpu):
    """1,025 disjoint triangles, one every 1,024 vertices, on the vertices 254, 255, 256 of their stretch (so each straddles a workgroup
    boundary), every other vertex isolated: V = 2^20 + 300 is past what one round of k_mc_scan takes, and the last triangle's
    root is a vertex of the second round's first workgroup.  min_faces=1 drops exactly the isolated vertices."""
    n_tri, stride = 1025, 1024
    base = np.arange(n_tri, dtype=np.int64) * stride + 254
    n_vertices = int(base[-1]) + 46
    assert n_vertices == SCAN_CAPACITY + 300 and base[-1] + 2 == SCAN_CAPACITY + BLOCK and n_vertices > 1024 > BLOCK
    faces = np.stack([base + 2, base, base + 1], axis=1).astype(np.int32)[::-1].copy()
    vertex_label, face_label, face_counts, vertex_counts = _check_components(gpu, faces, n_vertices, "1025 triangles")
    n_components = n_vertices - 2 * n_tri
    assert len(face_counts) == n_components and int(face_counts.sum()) == n_tri and int((face_counts == 1).sum()) == n_tri
    assert vertex_label[-1] == n_components - 1 and vertex_label[base[-1]] == vertex_label[base[-1] + 2] == base[-1] - 2 * (n_tri - 1)
    v = _vertices(n_vertices)
    got = _check_filter(gpu, v, faces, None, "1025 triangles", min_faces=1)
    assert got[3] == (n_components, n_tri, n_vertices, 3 * n_tri, n_tri, n_tri)
    assert np.array_equal(got[1].cpu().numpy(), (np.arange(3 * n_tri).reshape(n_tri, 3)[:, [2, 0, 1]])[::-1])
    got = _check_filter(gpu, v, faces, v, "1025 triangles", largest=True)                 # a tie of 1,025: the lowest label
    assert got[3].kept_vertices == 3 and got[1].cpu().tolist() == [[2, 0, 1]] and np.array_equal(_bits(got[0].cpu().numpy()), _bits(v[254:257]))


# ---- 5. ties
def test_ties_go_to_the_lower_label_and_no_faces_keep_nothing(hip_lib, gpu):
    from nerf import ops
    faces = [(8, 9, 10), (8, 10, 11), (5, 6, 7), (1, 2, 3), (1, 3, 4), (5, 5, 6)]         # components {1..4}: 2 faces, {5, 6, 7}: 2, {8..11}: 2
    want = _check_all(gpu, faces, 12, "tie")
    assert want[2].tolist() == [0, 2, 2, 2]
    got = _check_filter(gpu, _vertices(12), faces, None, "tie", largest=True)
    assert got[1].cpu().tolist() == [[0, 1, 2], [0, 2, 3]] and got[3].kept_vertices == 4
    for n_vertices, empty in ((5, []), (5, [(0, 1, 5), (-1, 2, 3)]), (0, [])):
        for rule in (dict(largest=True), dict(min_faces=1)):
            v, f, n, stats = _check_filter(gpu, _vertices(n_vertices), empty, _vertices(n_vertices, 2), "no valid face", **rule)
            assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3) and stats.kept_components == 0 and stats.components == n_vertices


# ---- 6. end to end on the isosurface
def test_largest_component_of_an_isosurface_is_the_extraction_of_the_big_sphere_alone(hip_lib, gpu):
    """33 x 29 x 25 grid on [-1, 1]^3: a sphere A of r 0.45 and two smaller ones written only inside boxes round their centres
    (tests/mesh_components_ref.py: e2e_fields).  ops.isosurface gives three components of 308 / 4,504 / 880 faces;
    filter_mesh(largest=True) equals ops.isosurface of A alone, vertices and normals bit for bit, faces exactly."""
    from nerf import ops
    alone, both = (torch.from_numpy(a).to(gpu) for a in M.e2e_fields(*R.grid_points(M.E2E_LO, M.E2E_HI, M.E2E_N)))
    mesh = ops.isosurface(both, 0.0, M.E2E_LO, M.E2E_HI, normals=True)
    want = ops.isosurface(alone, 0.0, M.E2E_LO, M.E2E_HI, normals=True)
    host = [t.cpu().numpy() for t in mesh]
    assert _check_components(gpu, host[1], host[0].shape[0], "three spheres")[2].tolist() == [308, 4504, 880]
    got = _check_filter(gpu, *host, "three spheres", largest=True)
    assert all(torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(got[:3], want)) and want[1].shape[0] == 4504
    assert got[3].components == 3 and got[3].kept_components == 1
    two = _check_filter(gpu, *host, "three spheres", min_faces=309)
    assert two[3].kept_components == 2 and two[3].kept_faces == 4504 + 880
    none = _check_filter(gpu, *host, "three spheres", min_faces=5000)
    assert none[0].shape == (0, 3) and none[1].shape == (0, 3) and none[2].shape == (0, 3)


# ---- 7. the entry points on poisoned buffers
PAD = 40                       # entries (rows) every output is longer than it needs to be


def _entry_points(gpu, vertices, faces, normals, rule, cut_v=0, cut_f=0):
    """label, select and emit through the C ABI: workspace and outputs filled with 0xFF, every output PAD entries (rows) longer than
    needed, capacities cut_v / cut_f rows below the counts.  Returns the counts and the host copies of the seven output buffers."""
    from nerf import _hip as H
    lib = H.lib()
    n_vertices, n_faces = vertices.shape[0], faces.shape[0]
    poison = lambda n, dtype=torch.int32: torch.full((n,), -1, dtype=dtype, device=gpu)       # -1: every byte 0xFF
    ws_bytes = lib.nf_mesh_components_workspace_bytes(n_vertices, n_faces)
    ws = torch.full((ws_bytes + 512,), 0xFF, dtype=torch.uint8, device=gpu)
    assert ws.data_ptr() % 256 == 0
    d_v, d_f = torch.from_numpy(vertices).to(gpu), torch.from_numpy(faces).to(gpu)
    d_n = None if normals is None else torch.from_numpy(normals).to(gpu)
    vertex_label, face_label, face_counts, vertex_counts = poison(n_vertices + PAD), poison(n_faces + PAD), poison(n_vertices + PAD), poison(n_vertices + PAD)
    counts = poison(4 + 2, torch.int64)
    stream = H.stream_ptr(gpu)
    H.check(lib.nf_mesh_components_label(H.ptr(d_f), n_vertices, n_faces, ws.data_ptr() + 256, ws_bytes, H.ptr(vertex_label), H.ptr(face_label),
                                         H.ptr(face_counts), H.ptr(vertex_counts), counts.data_ptr() + 8, stream), "label")
    H.check(lib.nf_mesh_components_select(H.ptr(vertex_label), H.ptr(face_label), H.ptr(face_counts), n_vertices, n_faces, int(bool(rule.get("largest"))),
                                          rule.get("min_faces") or 0, ws.data_ptr() + 256, ws_bytes, counts.data_ptr() + 8, stream), "select")
    assert counts[0].item() == -1 and counts[5].item() == -1
    n_components, kept_v, kept_f, kept_c = counts[1:5].tolist()
    out_v, out_f, out_n = poison(3 * (kept_v + PAD)), poison(3 * (kept_f + PAD)), poison(3 * (kept_v + PAD))
    H.check(lib.nf_mesh_components_emit(H.ptr(d_v), H.ptr(d_f), H.ptr(d_n), H.ptr(vertex_label), H.ptr(face_label), H.ptr(face_counts), n_vertices, n_faces,
                                        ws.data_ptr() + 256, ws_bytes, H.ptr(out_v), kept_v - cut_v, H.ptr(out_f), kept_f - cut_f,
                                        None if normals is None else H.ptr(out_n), stream), "emit")
    torch.cuda.synchronize()
    assert bool((ws[:256] == 0xFF).all()) and bool((ws[256 + ws_bytes:] == 0xFF).all())
    return (n_components, kept_v, kept_f, kept_c), [t.cpu().numpy() for t in (vertex_label, face_label, face_counts, vertex_counts, out_v, out_f, out_n)]


@pytest.mark.parametrize("rule", [dict(largest=True), dict(min_faces=2)], ids=["largest", "min_faces"])
def test_entry_points_keep_inside_their_buffers_and_repeat_bit_for_bit(hip_lib, gpu, rule):
    """Seeded faces (some invalid, some with repeated indices) over 1,500 vertices: everything up to the counts equals the
    restatement, nothing past the counts is written -- labels past V and F, counts past C, rows past V' and F' -- nor at or past a
    capacity below the counts; the bytes round the workspace stay; a second run gives the same bits; normals = NULL works."""
    n_vertices, n_faces = 1500, 700
    faces = M.random_faces(np.random.default_rng(5), n_vertices, n_faces)
    vertices, normals = _vertices(n_vertices, 3), _vertices(n_vertices, 4)
    labels = M.mesh_components(faces, n_vertices)
    want = M.filter_mesh(vertices, faces, normals, **rule)
    counts, bufs = _entry_points(gpu, vertices, faces, normals, rule)
    n_components, kept_v, kept_f, kept_c = counts
    assert counts == (len(labels[2]), want[3]["kept_vertices"], want[3]["kept_faces"], want[3]["kept_components"])
    assert 20 < n_components < n_vertices and 10 < kept_v < n_vertices and 8 < kept_f < n_faces
    for buf, ref, n in zip(bufs, labels + (want[0].view(np.int32).reshape(-1), want[1].reshape(-1), want[2].view(np.int32).reshape(-1)),
                           (n_vertices, n_faces, n_components, n_components, 3 * kept_v, 3 * kept_f, 3 * kept_v)):
        assert buf.dtype == np.int32 and np.array_equal(buf[:n], ref) and (buf[n:] == -1).all() and len(buf) - n >= PAD
    again = _entry_points(gpu, vertices, faces, normals, rule)
    assert again[0] == counts and all(np.array_equal(a, b) for a, b in zip(again[1], bufs))
    cut = _entry_points(gpu, vertices, faces, normals, rule, cut_v=5, cut_f=7)
    assert cut[0] == counts and all(np.array_equal(a, b) for a, b in zip(cut[1][:4], bufs[:4]))
    for part, full, n in ((cut[1][4], bufs[4], 3 * (kept_v - 5)), (cut[1][5], bufs[5], 3 * (kept_f - 7)), (cut[1][6], bufs[6], 3 * (kept_v - 5))):
        assert np.array_equal(part[:n], full[:n]) and (part[n:] == -1).all()
    none = _entry_points(gpu, vertices, faces, None, rule)
    assert none[0] == counts and all(np.array_equal(a, b) for a, b in zip(none[1][:6], bufs[:6])) and (none[1][6] == -1).all()


# ---- 8. the Python layer on a model's grid
GRID_N, GRID_LO, GRID_HI = (17, 13, 11), (-0.4, -0.35, -0.3), (0.35, 0.4, 0.4)       # the grid of tests/test_gpu_isosurface.py's model tests


def test_extract_mesh_with_a_rule_is_filter_mesh_of_extract_mesh(hip_lib, gpu):
    import nerf
    c = C.build_case("eval_det_64_128")
    m, expr, latent = U.make_model(nerf, c["p_coarse"], gpu).eval(), c["expr"].to(gpu), c["latent"].to(gpu)
    box = dict(lo=GRID_LO, hi=GRID_HI, resolution=GRID_N)
    level = float(nerf.density_grid(m, expr, latent, **box).median())
    plain = nerf.extract_mesh(m, expr, latent, level=level, **box)
    assert plain.faces.shape[0] > 0
    host = [t.cpu().numpy() for t in plain]
    labels = nerf.mesh_components(plain)
    for g, w in zip(labels, M.mesh_components(host[1], host[0].shape[0])):
        assert np.array_equal(g.cpu().numpy(), w)
    second = int(np.sort(labels.face_counts.cpu().numpy())[-2]) if labels.face_counts.numel() > 1 else 1
    print(f"model grid: V {host[0].shape[0]} F {host[1].shape[0]}, {labels.face_counts.numel()} components, face counts {labels.face_counts.tolist()[:12]}")
    for rule in (dict(largest=True), dict(min_faces=max(second, 1))):
        direct = nerf.extract_mesh(m, expr, latent, level=level, **box, **rule)
        after = nerf.filter_mesh(plain, **rule)
        want = M.filter_mesh(*host, **rule)
        assert isinstance(direct, nerf.Mesh) and isinstance(after, nerf.Mesh) and len(direct) == 3
        for d, a, w in zip(direct, after, want[:3]):
            assert torch.equal(d, a) and np.array_equal(_bits(d.cpu().numpy()), _bits(w))
    without = nerf.extract_mesh(m, expr, latent, level=level, normals=False, largest=True, **box)
    assert without.normals is None and torch.equal(without.faces, nerf.filter_mesh(plain, largest=True).faces)
    again = nerf.extract_mesh(m, expr, latent, level=level, **box)                          # the defaults: today's path, today's bits
    assert all(torch.equal(x, y) for x, y in zip(again, plain))


def test_launcher_with_largest_writes_the_filtered_ply(hip_lib, gpu, tmp_path, capsys):
    """launch.extract_mesh --largest on the synthetic dataset and an untrained checkpoint at 24^3: the .ply holds the largest component
    of the mesh the launcher writes without the flag, and its counts are the ones the stats line prints; --min-faces likewise."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synthetic_dataset as MS
    import nerf
    from launch import common as CM
    from launch import extract_mesh
    base = str(tmp_path)
    data = MS.write(os.path.join(base, "data"))
    cfg_path = os.path.join(base, "config.yml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(MS.config(data, os.path.join(base, "logs")), f)
    torch.manual_seed(7)
    cfg = CM.load_config(cfg_path)
    model_c, model_f = CM.build_models(cfg, gpu)
    ck_path = os.path.join(base, "untrained.ckpt")
    latents = torch.randn(6, 32) * 0.1
    torch.save({"model_coarse_state_dict": model_c.state_dict(), "model_fine_state_dict": model_f.state_dict(), "latent_codes": latents}, ck_path)
    _, poses, _, hwf, _, expressions, _, _ = nerf.load_flame_data(data, half_res=False, testskip=1, test=True)
    lo, hi = extract_mesh.frustum_box(int(hwf[0]), int(hwf[1]), hwf[2], poses[1, :3, :4].float().to(gpu), 0.2, 0.8)
    grid = nerf.density_grid(model_f.eval(), expressions[1].float().to(gpu), latents[1].to(gpu), lo=lo, hi=hi, resolution=24)
    level = float(grid.median())
    common = ["--config", cfg_path, "--checkpoint", ck_path, "--frame", "1", "--level", repr(level), "--resolution", "24"]
    whole = os.path.join(base, "whole.ply")
    extract_mesh.main(common + ["--out", whole])
    assert "components" not in capsys.readouterr().out                                    # no rule: no stats line, no filter
    rows, faces, _, _, _ = R.read_ply(whole)
    for flags, rule in ((["--largest"], dict(largest=True)), (["--min-faces", "3"], dict(min_faces=3))):
        out = os.path.join(base, "kept.ply")
        stats = extract_mesh.main(common + ["--out", out] + flags)
        text = capsys.readouterr().out
        want = M.filter_mesh(rows[:, :3], faces, rows[:, 3:], **rule)
        got_rows, got_faces, props, _, _ = R.read_ply(out)
        assert props == ["x", "y", "z", "nx", "ny", "nz"] and got_rows.shape[0] == stats["vertices"] and got_faces.shape[0] == stats["faces"]
        assert stats["components"] == want[3] and stats["faces"] > 0
        assert f"V = {stats['vertices']}, F = {stats['faces']}" in text
        assert (f"{want[3]['components']} components, {want[3]['kept_components']} kept; vertices {stats['vertices']} of {rows.shape[0]}, "
                f"faces {stats['faces']} of {faces.shape[0]}") in text
        assert np.array_equal(_bits(got_rows[:, :3]), _bits(want[0])) and np.array_equal(_bits(got_rows[:, 3:]), _bits(want[2]))
        assert np.array_equal(got_faces, want[1])
