"""Mesh colours on the GPU: the two kernels of csrc/nf_mesh_colour.hip against tests/mesh_colour_ref.py -- the rays bit for bit (every
float32 operation of the specification is one NumPy float32 operation there), the composite against float64 within the forward gates of
tests/test_gpu_render_sizes.py -- through the C entry points, into buffers pre-filled with 0xFF of which nothing past the named ranges
may change, and through nerf.ops; nerf.radiance against the full forward; nerf.vertex_colours against its own pieces; the launcher's
--colour.  GPU only."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from oracle import nerface_oracle as O
from tests import mesh_colour_ref as K
from tests import test_gpu_density as D                  # its COMBOS and its models, built once per process
from tests.test_gpu_mesh_smooth import GRID_HI, GRID_LO, GRID_N

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 40                       # entries every output buffer is longer than it needs to be
SIZES = (0, 1, 3, 63, 64, 65, 255, 256, 257, 1025)
SAMPLES = (1, 2, 3, 8, 63, 64)
STEP, MIN_OPACITY = 0.01, 1e-3
GATE = 5e-6                    # e_rgb, e_acc of tests/test_gpu_render_sizes.py's forward


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _poison(n, gpu):
    return torch.full((n,), -1, dtype=torch.int32, device=gpu)           # every byte 0xFF


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


# ---- a. the rays kernel
def _camera(seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, :3], c2w[:3, 3] = q.astype(np.float32), rng.standard_normal(3).astype(np.float32)
    return c2w


def _vertices(n_vertices, c2w, seed):
    """Positions round the camera, half of them behind it; vertex 0 is the camera's origin (d == 0 exactly), vertex 1 has a zero normal,
    vertex 2 lies on the camera's axis."""
    rng = np.random.default_rng(seed)
    v = (c2w[:3, 3] + rng.standard_normal((n_vertices, 3)) * 2).astype(np.float32)
    n = rng.standard_normal((n_vertices, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True) + np.float32(1e-9)
    if n_vertices > 0:
        v[0] = c2w[:3, 3]
    if n_vertices > 1:
        n[1] = 0
    if n_vertices > 2:
        v[2] = c2w[:3, 3] - np.float32(1.5) * c2w[:3, 2]
    return v, n.astype(np.float32)


def _rays_entry(gpu, v, n, c2w, stride, view_z, n_samples, depth):
    """nf_mesh_colour_rays into poisoned buffers PAD entries too long -> host (rd, rd_view, z) as int32, the pads checked."""
    from nerf import _hip as H
    lib = H.lib()
    n_vertices = len(v)
    rd, rd_view, z = _poison(3 * n_vertices + PAD, gpu), _poison(3 * n_vertices + PAD, gpu), _poison(n_vertices * n_samples + PAD, gpu)
    d_v, d_n = _dev(v, gpu), _dev(n, gpu)
    d_c = None if c2w is None else _dev(c2w, gpu)
    H.check(lib.nf_mesh_colour_rays(H.ptr(d_v), H.ptr(d_n), n_vertices, H.ptr(d_c), stride, view_z, n_samples, depth, H.ptr(rd), H.ptr(rd_view), H.ptr(z),
                                    H.stream_ptr(gpu)), "nf_mesh_colour_rays")
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in (rd, rd_view, z)]
    for t, used in zip(out, (3 * n_vertices, 3 * n_vertices, n_vertices * n_samples)):
        assert (t[used:] == -1).all() and len(t) - used == PAD
    return out[0][:3 * n_vertices], out[1][:3 * n_vertices], out[2][:n_vertices * n_samples]


@pytest.mark.parametrize("n_samples", SAMPLES)
def test_rays_are_the_restatements_bit_for_bit(hip_lib, gpu, n_samples):
    from nerf import ops
    c2w = _camera(n_samples)
    padded = np.full((3, 7), np.nan, dtype=np.float32)                  # a row stride of 7: what lies between the rows is not read
    padded[:, :4] = c2w[:3]
    for n_vertices in SIZES:
        v, n = _vertices(n_vertices, c2w, 100 + n_vertices)
        for depth in ((0.037, 0.0) if n_vertices in (3, 65) else (0.037,)):
            for view in (c2w, np.float32(-0.8)):
                want = K.rays(v, n, view, n_samples, depth)
                cam = view is c2w
                got = _rays_entry(gpu, v, n, c2w if cam else None, 4, 0.0 if cam else float(view), n_samples, depth)
                for name, g, w in zip(("rd", "rd_view", "z"), got, want):
                    assert np.array_equal(g.view(np.uint32), _bits(w).reshape(-1)), (name, n_vertices, n_samples, depth, cam)
                if n_vertices == 0:
                    continue
                kw = dict(pose=_dev(c2w if n_vertices % 2 else c2w[:3], gpu)) if cam else dict(view_z=float(view))
                rd, rd_view, z = ops.mesh_colour_rays(_dev(v, gpu), _dev(n, gpu), samples=n_samples, depth=depth, **kw)
                assert rd.shape == (n_vertices, 3) and rd_view.shape == (n_vertices, 3) and z.shape == (n_vertices, n_samples)
                for name, g, w in zip(("rd", "rd_view", "z"), (rd, rd_view, z), want):
                    assert g.dtype == torch.float32 and g.is_cuda and np.array_equal(_bits(g.cpu().numpy()), _bits(w)), (name, n_vertices, n_samples, cam)
        if n_vertices == 257:
            got = _rays_entry(gpu, v, n, padded, 7, 0.0, n_samples, 0.037)
            assert all(np.array_equal(g.view(np.uint32), _bits(w).reshape(-1)) for g, w in zip(got, K.rays(v, n, c2w, n_samples, 0.037)))
        if n_vertices > 2:                                              # the cases the draw is built to hold
            rd, rd_view, z = K.rays(v, n, c2w, n_samples, 0.037)
            t = v - c2w[:3, 3]
            d = -((t[:, 0] * c2w[0, 2] + t[:, 1] * c2w[1, 2]) + t[:, 2] * c2w[2, 2])
            assert d[0] == 0 and np.array_equal(_bits(rd_view[0]), _bits(-c2w[:3, 2])) and d[2] > 1 and (n_vertices < 63 or ((d < 0).sum() > 10 < (d > 0).sum()))
            assert np.array_equal(_bits(rd_view[d < 0]), _bits(np.broadcast_to(-c2w[:3, 2], rd_view[d < 0].shape))) and np.signbit(rd[1]).all() and (rd[1] == 0).all()
            assert np.allclose(rd_view[2], -c2w[:3, 2], atol=2e-6)


# ---- b. the integrate kernel
def _raw(n_vertices, n_samples, seed):
    """The draw of tests/test_gpu_render_sizes.py (N(0, 2^2), the density channel x 8) with the regimes written in: every eighth vertex
    (from 0) has no positive density, every eighth (from 1) an opaque first sample; a vertex whose float64 opacity comes within 1e-4
    of min_opacity loses its density, so that neither arithmetic can take the other branch."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn((n_vertices, n_samples, 4), generator=g) * 2.0
    raw[..., 3] *= 8.0
    raw = raw.numpy()
    raw[0::8, :, 3] = -np.abs(raw[0::8, :, 3]) - np.float32(0.1)
    raw[1::8, 0, 3] = np.float32(30.0 / STEP) + np.abs(raw[1::8, 0, 3])
    for _ in range(2):
        _, acc = K.integrate(raw, STEP, MIN_OPACITY)
        raw[np.abs(acc - MIN_OPACITY) <= 1e-4, :, 3] = np.float32(-1.0)
    return raw


def _integrate_entry(gpu, raw, step=STEP, min_opacity=MIN_OPACITY):
    from nerf import _hip as H
    lib = H.lib()
    n_vertices, n_samples = raw.shape[:2]
    colour, opacity = _poison(3 * n_vertices + PAD, gpu), _poison(n_vertices + PAD, gpu)
    d_raw = _dev(raw, gpu)
    H.check(lib.nf_mesh_colour_integrate(H.ptr(d_raw), n_vertices, n_samples, step, min_opacity, H.ptr(colour), H.ptr(opacity), H.stream_ptr(gpu)),
            "nf_mesh_colour_integrate")
    torch.cuda.synchronize()
    colour, opacity = colour.cpu().numpy(), opacity.cpu().numpy()
    assert (colour[3 * n_vertices:] == -1).all() and (opacity[n_vertices:] == -1).all()
    return colour[:3 * n_vertices].view(np.float32).reshape(n_vertices, 3), opacity[:n_vertices].view(np.float32)


def _check_integrate(colour, opacity, raw, what, step=STEP, min_opacity=MIN_OPACITY):
    """The gates: |opacity - ref| < 5e-6; the colour within 1e-5 / ref opacity where the vertex is seen (d(c / a) <= (dc + da) / a with
    colours <= 1) and within 5e-6 where it takes the sample at the vertex.  No vertex of the reference lies within 1e-4 of the branch."""
    want_c, want_a = K.integrate(raw, step, min_opacity)
    assert (np.abs(want_a - min_opacity) > 1e-4).all(), what
    if len(want_a) == 0:
        return want_c, want_a
    seen = want_a >= min_opacity
    e_acc = np.abs(opacity - want_a).max()
    err = np.abs(colour - want_c).max(axis=1)
    e_seen = (err * want_a)[seen].max() if seen.any() else 0.0
    e_dark = err[~seen].max() if (~seen).any() else 0.0
    print(f"{what}: e_acc {e_acc:.3e}  e_colour * opacity (seen) {e_seen:.3e}  e_colour (fallback) {e_dark:.3e}  seen {int(seen.sum())} of {len(seen)}")
    assert e_acc < GATE and e_seen <= 1e-5 and e_dark < GATE, what
    assert ((opacity >= min_opacity) == seen).all(), what                # the share of vertices excluded for a branch flip is zero
    return want_c, want_a


@pytest.mark.parametrize("n_samples", SAMPLES)
def test_integrate_against_the_float64_restatement(hip_lib, gpu, n_samples):
    from nerf import ops
    middle = n_samples // 2
    sig = lambda x: 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    for n_vertices in SIZES:
        raw = _raw(n_vertices, n_samples, 1000 * n_samples + n_vertices)
        colour, opacity = _integrate_entry(gpu, raw)
        what = f"V = {n_vertices}, K = {n_samples}"
        want_c, want_a = _check_integrate(colour, opacity, raw, what)
        if n_vertices == 0:
            assert ops.mesh_colour_integrate(_dev(raw, gpu), STEP, MIN_OPACITY).colours.shape == (0, 3)
            continue
        # the regimes: nothing absorbs -> opacity 0 exactly and the middle sample's colour; an opaque first sample -> its colour, opacity 1
        assert (opacity[0::8] == 0).all() and np.abs(colour[0::8] - sig(raw[0::8, middle, :3])).max() < GATE, what
        if n_vertices > 1:
            assert np.abs(opacity[1::8] - 1).max() < GATE and np.abs(colour[1::8] - sig(raw[1::8, 0, :3])).max() <= 1e-5, what
        assert ((colour >= 0) & (colour <= 1 + 1e-6)).all() and ((opacity >= 0) & (opacity <= 1 + 1e-6)).all(), what
        # the same bits from run to run, and from ops
        again = _integrate_entry(gpu, raw)
        assert np.array_equal(_bits(again[0]), _bits(colour)) and np.array_equal(_bits(again[1]), _bits(opacity)), what
        got = ops.mesh_colour_integrate(_dev(raw, gpu), STEP, MIN_OPACITY)
        assert isinstance(got, ops.MeshColours) and got.colours.shape == (n_vertices, 3) and got.opacity.shape == (n_vertices,)
        assert np.array_equal(_bits(got.colours.cpu().numpy()), _bits(colour)) and np.array_equal(_bits(got.opacity.cpu().numpy()), _bits(opacity)), what
        # a vertex whose row is NaN: its outputs are NaN, every other vertex keeps its bits
        if n_vertices >= 3:
            at = n_vertices // 2
            holed = raw.copy()
            holed[at] = np.nan
            c2, a2 = _integrate_entry(gpu, holed)
            assert np.isnan(c2[at]).all() and np.isnan(a2[at]), what
            keep = np.arange(n_vertices) != at
            assert np.array_equal(_bits(c2[keep]), _bits(colour[keep])) and np.array_equal(_bits(a2[keep]), _bits(opacity[keep])), what


def test_integrate_with_another_step_and_threshold(hip_lib, gpu):
    """step = 0 absorbs nothing (every vertex takes the middle sample); a threshold above every opacity does the same; a larger step."""
    raw = _raw(300, 5, 77)
    sig = lambda x: 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    colour, opacity = _integrate_entry(gpu, raw, step=0.0)
    assert (opacity == 0).all() and np.abs(colour - sig(raw[:, 2, :3])).max() < GATE
    fallback, opacity = _integrate_entry(gpu, raw, min_opacity=2.0)
    assert np.array_equal(_bits(fallback), _bits(colour)) and opacity.max() > 0.5
    raw[:, :, 3] = np.abs(raw[:, :, 3]) + np.float32(1.0)
    _check_integrate(*_integrate_entry(gpu, raw, step=0.5), raw, "step 0.5", step=0.5)


# ---- c. nerf.radiance
@pytest.mark.parametrize("kind,precision", D.COMBOS)
def test_radiance_is_the_full_forward_at_points(hip_lib, gpu, kind, precision):
    """nerf.radiance = hip_forward on the same points bit for bit, in every family and arithmetic; in f32 all four channels also match
    model.forward on the encoded points within 2e-5 * scale + 2e-5, the bound tests/test_gpu_density.py holds that forward to."""
    import nerf
    m, expr, latent = D._model(kind, gpu)
    g = torch.Generator().manual_seed(5)
    pts = ((torch.rand((131, 3), generator=g) - 0.5) * 0.8).to(gpu)
    view = torch.randn((131, 3), generator=g).to(gpu)
    lat = None if not m.NEEDS_LATENT else latent
    nerf.set_mlp_precision(precision)
    with torch.no_grad():
        raw = nerf.radiance(m, pts, view, expr, lat, near=O.NEAR, far=O.FAR)
        one = nerf.radiance(m, pts, view[7], expr, lat, near=O.NEAR, far=O.FAR)
        assert nerf.radiance(m, pts[:0], view[:0], expr, lat, near=O.NEAR, far=O.FAR).shape == (0, 4)
        assert nerf.radiance(m, pts[:0], view[0], expr, lat, near=O.NEAR, far=O.FAR).shape == (0, 4)
    assert raw.shape == (131, 4) and raw.dtype == torch.float32
    zero, z = torch.zeros_like(pts), torch.zeros((131, 1), device=gpu)
    ref, _ = m.hip_forward(pts, zero, z, view, expr, latent, O.NEAR, O.FAR, False)
    assert torch.equal(raw, ref.reshape(131, 4))
    ref, _ = m.hip_forward(pts, zero, z, view[7].expand(131, 3).contiguous(), expr, latent, O.NEAR, O.FAR, False)
    assert torch.equal(one, ref.reshape(131, 4)) and not torch.equal(one[:, :3], raw[:, :3]) and torch.equal(one[:, 3], raw[:, 3])
    with torch.no_grad():
        assert torch.equal(nerf.density(m, pts, expr, lat), raw[:, 3])
    with pytest.raises(NotImplementedError, match="no autograd"):            # the parameters require grad
        nerf.radiance(m, pts, view, expr, lat, near=O.NEAR, far=O.FAR)
    with torch.no_grad(), pytest.raises(ValueError, match="view"):
        nerf.radiance(m, pts, view[:5], expr, lat, near=O.NEAR, far=O.FAR)
    if precision == "f32":
        x87 = O.encode_points(pts.cpu(), view.cpu(), torch.zeros((131, 1)), O.NEAR, O.FAR).to(gpu)
        with torch.no_grad():
            fwd = m(x87, expr, latent)
        scale = float(fwd.abs().max())
        err = float((raw - fwd).abs().max())
        print(f"{kind} radiance vs forward(x87): err {err:.3e} scale {scale:.3e}")
        assert fwd.shape == (131, 4) and err <= 2e-5 * scale + 2e-5


def test_radiance_of_the_smaller_family_refuses_a_split_arithmetic(hip_lib, gpu):
    import nerf
    m, expr, latent = D._model("smaller", gpu)
    pts = torch.zeros((4, 3), device=gpu)
    for precision in ("bf16x3", "f16x3", "f16x2"):
        nerf.set_mlp_precision(precision)
        with torch.no_grad(), pytest.raises(NotImplementedError):
            nerf.radiance(m, pts, pts[0], expr, latent, near=O.NEAR, far=O.FAR)


# ---- d. nerf.vertex_colours
_MESHES = {}
POSE = np.array([[0.96, 0.0, 0.28, 0.33], [0.0, 1.0, 0.0, 0.02], [-0.28, 0.0, 0.96, 1.1], [0.0, 0.0, 0.0, 1.0]], dtype=np.float32)   # looks at the box


def _model_mesh(kind, gpu):
    """The model, its conditioning and the mesh of its density's median level on the grid of tests/test_gpu_mesh_smooth.py (in f32)."""
    import nerf
    m, expr, latent = D._model(kind, gpu)
    if kind not in _MESHES:
        box = dict(lo=GRID_LO, hi=GRID_HI, resolution=GRID_N)
        with torch.no_grad():
            level = float(nerf.density_grid(m, expr, latent, **box).median())
            _MESHES[kind] = nerf.extract_mesh(m, expr, latent, level=level, **box)
        assert _MESHES[kind].faces.shape[0] > 0
    return m, expr, latent, _MESHES[kind]


CELL = float(np.sqrt(sum(((h - l) / (n - 1)) ** 2 for l, h, n in zip(GRID_LO, GRID_HI, GRID_N))))


@pytest.mark.parametrize("kind,precision", [("paper", "f32"), ("paper", "f16x2"), ("lcode", "f32")])
def test_vertex_colours_is_its_pieces_and_does_not_depend_on_the_slabs(hip_lib, gpu, kind, precision):
    import nerf
    from nerf import ops
    m, expr, latent, mesh = _model_mesh(kind, gpu)
    n_vertices = mesh.vertices.shape[0]
    pose = torch.from_numpy(POSE).to(gpu)
    nerf.set_mlp_precision(precision)
    kw = dict(near=O.NEAR, far=O.FAR, samples=5, depth=CELL)
    got = nerf.vertex_colours(m, mesh, expr, latent, pose=pose, **kw)                 # not under no_grad: the pass sets it itself
    assert isinstance(got, nerf.MeshColours) and got.colours.shape == (n_vertices, 3) and got.opacity.shape == (n_vertices,)
    assert got.colours.dtype == torch.float32 and got.colours.is_cuda and bool(((got.colours >= 0) & (got.colours <= 1)).all())
    # the public pieces
    rd, rd_view, z = ops.mesh_colour_rays(mesh.vertices, mesh.normals, samples=5, depth=CELL, pose=pose)
    want = K.rays(mesh.vertices.cpu().numpy(), mesh.normals.cpu().numpy(), POSE, 5, CELL)
    assert all(np.array_equal(_bits(g.cpu().numpy()), _bits(w)) for g, w in zip((rd, rd_view, z), want))
    assert bool((rd_view[:, 2] < 0).all()) and not bool((rd_view == rd_view[0]).all())          # every vertex in front of the camera, each its own pixel
    with torch.no_grad():
        raw, _ = m.hip_forward(mesh.vertices, rd, z, rd_view, expr, latent, O.NEAR, O.FAR, False)
    pieces = ops.mesh_colour_integrate(raw, ops.mesh_colour_step(CELL, 5), 1e-3)
    assert torch.equal(got.colours.view(torch.int32), pieces.colours.view(torch.int32)) and torch.equal(got.opacity.view(torch.int32), pieces.opacity.view(torch.int32))
    assert ops.mesh_colour_step(CELL, 5) == float(np.float32(2) * (np.float32(CELL) / np.float32(5)))
    print(f"{kind} {precision}: V = {n_vertices}, opacity in [{float(got.opacity.min()):.3g}, {float(got.opacity.max()):.3g}], "
          f"{int((got.opacity < 1e-3).sum())} below min_opacity")
    # slabs: one, three with a partial last one, one vertex each
    third = n_vertices // 3 + 1
    assert -(-n_vertices // third) == 3 and n_vertices % third
    for chunk_points in (1 << 22, third * 5 + 4, 5):
        again = nerf.vertex_colours(m, mesh, expr, latent, pose=pose, chunk_points=chunk_points, **kw)
        assert torch.equal(again.colours.view(torch.int32), got.colours.view(torch.int32)), chunk_points
        assert torch.equal(again.opacity.view(torch.int32), got.opacity.view(torch.int32)), chunk_points
    # a tuple, a (3, 4) pose, and a mesh without normals: those of its faces
    assert torch.equal(nerf.vertex_colours(m, tuple(mesh), expr, latent, pose=pose[:3], **kw).colours, got.colours)
    bare = nerf.vertex_colours(m, (mesh.vertices, mesh.faces), expr, latent, pose=pose, **kw)
    from_faces = nerf.vertex_colours(m, nerf.Mesh(mesh.vertices, mesh.faces, nerf.vertex_normals(mesh)), expr, latent, pose=pose, **kw)
    assert torch.equal(bare.colours, from_faces.colours) and torch.equal(bare.opacity, from_faces.opacity) and not torch.equal(bare.colours, got.colours)
    # view_z in place of a camera
    flat = nerf.vertex_colours(m, mesh, expr, latent, view_z=-1.0, **kw)
    assert torch.equal(flat.opacity, got.opacity) and not torch.equal(flat.colours, got.colours)        # the density does not see the direction


@pytest.mark.parametrize("kind,precision", [("paper", "f32"), ("paper", "f16x2"), ("lcode", "f32")])
def test_one_sample_is_the_radiance_at_the_vertex(hip_lib, gpu, kind, precision):
    """samples = 1: the one sample lies on the vertex, so the colour is sigmoid(nerf.radiance(vertices, rd_view)[:, :3]) -- exactly where
    the vertex takes its middle sample, and within the colour gate 5e-6 where it is w * s / w (two roundings) -- and the opacity is
    1 - exp(-relu(sigma) * step) within 5e-6, both against float64 of the network's float32 output."""
    import nerf
    from nerf import ops
    m, expr, latent, mesh = _model_mesh(kind, gpu)
    pose = torch.from_numpy(POSE).to(gpu)
    nerf.set_mlp_precision(precision)
    depth = 4 * CELL
    got = nerf.vertex_colours(m, mesh, expr, latent, near=O.NEAR, far=O.FAR, pose=pose, samples=1, depth=depth)
    _, rd_view, z = ops.mesh_colour_rays(mesh.vertices, mesh.normals, samples=1, depth=depth, pose=pose)
    assert bool((z == 0).all())
    with torch.no_grad():
        raw = nerf.radiance(m, mesh.vertices, rd_view, expr, latent, near=O.NEAR, far=O.FAR)
    raw64 = raw.cpu().numpy().astype(np.float64)
    want_c = 1 / (1 + np.exp(-raw64[:, :3]))
    step = np.float64(np.float32(ops.mesh_colour_step(depth, 1)))
    want_a = 1 - np.exp(-np.maximum(raw64[:, 3], 0) * step)
    colours, opacity = got.colours.cpu().numpy(), got.opacity.cpu().numpy()
    seen = opacity >= np.float32(1e-3)
    e_c, e_a = np.abs(colours - want_c).max(), np.abs(opacity - want_a).max()
    print(f"{kind} {precision}: samples = 1: e_colour {e_c:.3e} e_opacity {e_a:.3e}, seen {int(seen.sum())} of {len(seen)}")
    assert e_c < GATE and e_a < GATE and seen.any()
    pieces = ops.mesh_colour_integrate(raw.reshape(-1, 1, 4), float(step), 1e-3)
    assert torch.equal(pieces.colours, got.colours) and torch.equal(pieces.opacity, got.opacity)


def test_vertex_colours_refuses_by_argument_and_launches_nothing_for_no_vertices(hip_lib, gpu, monkeypatch):
    import nerf
    from nerf import ops
    m, expr, latent, mesh = _model_mesh("paper", gpu)
    pose = torch.from_numpy(POSE).to(gpu)
    ok = dict(near=O.NEAR, far=O.FAR, depth=CELL, pose=pose)
    for change, word in ((dict(samples=0), "samples"), (dict(samples=65), "samples"), (dict(depth=-1e-3), "depth"), (dict(depth=float("nan")), "depth"),
                         (dict(view_z=1.0), "view_z"), (dict(pose=None), "pose"), (dict(pose=pose[:3, :3].contiguous()), "pose")):
        with pytest.raises(ValueError, match=word):
            nerf.vertex_colours(m, mesh, expr, latent, **{**ok, **change})
    with pytest.raises(NotImplementedError, match="latent_code"):
        nerf.vertex_colours(m, mesh, expr, None, **ok)
    nerf.set_mlp_precision("f16x2")
    with pytest.raises(NotImplementedError):
        nerf.vertex_colours(D._model("smaller", gpu)[0], mesh, expr, latent, **ok)
    nerf.set_mlp_precision("f32")
    for name in ("vertex_colours", "mesh_colour_rays", "mesh_colour_integrate", "vertex_normals", "bump_pack_epoch"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("no vertices: nothing may be launched"))
    monkeypatch.setattr(type(m), "hip_forward", lambda *a, **k: pytest.fail("no vertices: the network is not asked"))
    for empty in (nerf.Mesh(mesh.vertices[:0], mesh.faces[:0], mesh.normals[:0]), (mesh.vertices[:0], mesh.faces[:0])):
        got = nerf.vertex_colours(m, empty, expr, latent, **ok)
        assert got.colours.shape == (0, 3) and got.opacity.shape == (0,) and got.colours.is_cuda and got.colours.dtype == torch.float32


# ---- e. the launcher
def test_launcher_with_colour_writes_the_colours_of_the_mesh_it_wrote(hip_lib, gpu, tmp_path, capsys):
    """launch.extract_mesh --largest --colour --colour-samples 3 on the synthetic dataset and an untrained checkpoint at 24^3: positions,
    normals and faces are those of the run without --colour, the colour bytes those of nerf.vertex_colours on that mesh with the frame's
    pose and the cell's diagonal; without --colour the file and the text are what they were."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synthetic_dataset as MS
    import nerf
    from launch import common as CM
    from launch import extract_mesh
    from tests import isosurface_ref as R
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
    pose = poses[1, :3, :4].float().to(gpu)
    near, far = float(cfg.dataset.near), float(cfg.dataset.far)
    lo, hi = extract_mesh.frustum_box(int(hwf[0]), int(hwf[1]), hwf[2], pose, near, far)
    expr, latent = expressions[1].float().to(gpu), latents[1].to(gpu)
    grid = nerf.density_grid(model_f.eval(), expr, latent, lo=lo, hi=hi, resolution=24)
    level = float(grid.median())
    common = ["--config", cfg_path, "--checkpoint", ck_path, "--frame", "1", "--level", repr(level), "--resolution", "24", "--largest"]
    plain = os.path.join(base, "plain.ply")
    stats = extract_mesh.main(common + ["--out", plain])
    text = capsys.readouterr().out
    assert "coloured:" not in text and "colour" not in stats and len(text.strip().splitlines()) == 2
    rows, faces, props, _, _ = R.read_ply(plain)                         # the reader of the uncoloured files reads it: the file is as before
    assert props == ["x", "y", "z", "nx", "ny", "nz"] and len(faces) > 0
    out = os.path.join(base, "coloured.ply")
    stats = extract_mesh.main(common + ["--out", out, "--colour", "--colour-samples", "3"])
    text = capsys.readouterr().out
    got_rows, got_faces, got_colours, got_props = K.read_ply(out)
    assert got_props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(_bits(got_rows), _bits(rows)) and np.array_equal(got_faces, faces)
    cell = float(np.sqrt(sum(((float(h) - float(l)) / 23) ** 2 for l, h in zip(lo, hi))))
    mesh = nerf.Mesh(torch.from_numpy(rows[:, :3].copy()).to(gpu), torch.from_numpy(faces).to(gpu), torch.from_numpy(rows[:, 3:].copy()).to(gpu))
    want = nerf.vertex_colours(model_f, mesh, expr, latent, near=near, far=far, pose=pose, samples=3, depth=cell)
    assert np.array_equal(got_colours, K.quantise(want.colours.cpu().numpy())) and len(np.unique(got_colours, axis=0)) > 1
    below = int((want.opacity < 1e-3).sum())
    assert stats["colour"] == dict(vertices=len(rows), samples=3, depth=cell, min_opacity=1e-3, below_min_opacity=below)
    assert f"coloured: {len(rows)} vertices, 3 samples over a shell of half-thickness {cell:.6g}; {below} vertices below opacity 0.001" in text
    assert len(text.strip().splitlines()) == 3
    # --colour-view-z and --colour-depth, into an .obj
    obj = os.path.join(base, "coloured.obj")
    stats = extract_mesh.main(common + ["--out", obj, "--colour", "--colour-samples", "1", "--colour-depth", "0.05", "--colour-view-z", "-1"])
    capsys.readouterr()
    want = nerf.vertex_colours(model_f, mesh, expr, latent, near=near, far=far, view_z=-1.0, samples=1, depth=0.05)
    ov, oc, on, of = K.read_obj(obj)
    assert np.array_equal(_bits(ov), _bits(rows[:, :3])) and np.array_equal(_bits(oc), _bits(want.colours.cpu().numpy())) and np.array_equal(of, faces)
    assert stats["colour"]["depth"] == 0.05 and stats["colour"]["samples"] == 1
