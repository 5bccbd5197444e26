"""CPU: the sparse-grid specification as tests/sparse_grid_ref.py restates it -- the guarantee (the sparse grid gives the dense grid's
mesh when every brick that is no seed lies on one side and dilate >= 1), its limit (a blob inside one brick is missed at margin 0),
what makes a seed; and the product's refusals without a device and its exported symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import isosurface_ref as R
from tests import sparse_grid_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["nf_sparse_grid_workspace_bytes", "nf_sparse_grid_lattice", "nf_sparse_grid_classify", "nf_sparse_grid_mark", "nf_sparse_grid_emit",
                "nf_sparse_grid_scatter"]


def _field(name):
    x, y, z = R.grid_points(S.FIELD_LO, S.FIELD_HI, S.FIELD_N)
    v = getattr(S, name + "_field")(x, y, z)
    assert v.dtype == np.float32
    return v


def _same_mesh(a, b):
    return [p.shape == q.shape and np.array_equal(p, q) for p, q in zip(a, b)]


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_sparse_grid_gives_the_dense_mesh(name):
    """The precondition is checked on the dense array first; then vertices, faces and normals of the restated sparse grid equal the
    dense grid's, array_equal, with a quarter of the bricks and of the points never evaluated.  At dilate = 0 vertices and faces
    still agree and the normals do not (they reach into a brick that was not evaluated): why extract_mesh asks for dilate >= 1."""
    v = _field(name)
    dense = R.isosurface(v, 0.0, S.FIELD_LO, S.FIELD_HI, normals=True)
    assert dense[1].shape[0] > 1000 and R.mesh_report(dense[0], dense[1])["closed"]
    s = S.restate(v, 0.0, S.FIELD_BRICK)
    assert S.one_sided(v, 0.0, S.FIELD_BRICK, s.seed)
    assert 0 < s.seed.sum() < s.active.sum() <= 48 and s.evaluated.sum() < 0.8 * v.size
    assert np.isinf(s.grid[~s.evaluated]).all() and np.array_equal(s.grid[s.evaluated], v[s.evaluated])
    assert _same_mesh(dense, R.isosurface(s.grid, 0.0, S.FIELD_LO, S.FIELD_HI, normals=True)) == [True, True, True]
    s0 = S.restate(v, 0.0, S.FIELD_BRICK, dilate=0)
    assert np.array_equal(s0.active, s0.seed)
    assert _same_mesh(dense, R.isosurface(s0.grid, 0.0, S.FIELD_LO, S.FIELD_HI, normals=True)) == [True, True, False]


def test_a_blob_inside_one_brick_is_missed_without_a_margin():
    """17^3 points on [-1, 1]^3, bricks of 8 cells; a ball of radius 0.2 round the centre (-0.5, -0.5, -0.5) of the first brick.  Its
    value at the brick's corners is 0.04 - 0.75 = -0.71: at margin 0 no brick is a seed, nothing but the 27 lattice points is
    evaluated and the mesh is empty; at margin 0.8 the corners are within the margin, and the mesh is the dense one."""
    lo, hi, n = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (17, 17, 17)
    v = S.sphere_field(*R.grid_points(lo, hi, n), centre=(-0.5, -0.5, -0.5), r=0.2)
    dense = R.isosurface(v, 0.0, lo, hi, normals=True)
    assert dense[1].shape[0] > 0
    missed = S.restate(v, 0.0, 8)
    assert not missed.seed.any() and not missed.active.any() and missed.evaluated.sum() == 27
    assert not S.one_sided(v, 0.0, 8, missed.seed)                              # the precondition of the guarantee does not hold
    assert (missed.grid[~missed.evaluated] == -np.inf).all()
    assert R.isosurface(missed.grid, 0.0, lo, hi)[1].shape[0] == 0
    found = S.restate(v, 0.0, 8, margin=0.8)
    assert found.seed[0, 0, 0] and S.one_sided(v, 0.0, 8, found.seed)
    assert _same_mesh(dense, R.isosurface(found.grid, 0.0, lo, hi, normals=True)) == [True, True, True]
    assert not S.restate(v, 0.0, 8, margin=0.7).seed.any()                      # below the distance to the corners: still missed


def test_nan_and_level_corners_make_seeds():
    v = np.full((9, 9, 17), 1.0, dtype=np.float32)                             # two bricks along x, all inside
    assert not S.restate(v, 0.0, 8).seed.any() and (S.restate(v, 0.0, 8).grid[0, 0, 1] == np.inf)
    for corner_value in (np.nan, 0.0):
        w = v.copy()
        w[8, 8, 16] = corner_value                                             # a corner of the second brick only
        s = S.restate(w, 0.0, 8)
        assert s.seed.tolist() == [[[False, True]]] and s.active.all() and s.evaluated.all()
        assert S.restate(w, 0.0, 8, dilate=0).active.tolist() == [[[False, True]]]
    w = v.copy()
    w[8, 8, 8] = np.nan                                                        # a corner both bricks share
    assert S.restate(w, 0.0, 8).seed.all()
    w = np.full((9, 9, 9), -1.0, dtype=np.float32)
    assert not S.restate(w, 0.0, 8).seed.any() and S.restate(w, 0.0, 8).grid[4, 4, 4] == -np.inf
    assert S.restate(w, -1.0, 8).seed.all()                                    # every corner == level
    # short last bricks: 19 points in bricks of 4 are [0,4] [4,8] [8,12] [12,16] [16,18]
    assert S.n_bricks(19, 4) == 5 and S.brick_range(4, 19, 4) == (16, 18) and S.lattice_indices(19, 4).tolist() == [0, 4, 8, 12, 16, 18]
    assert S.n_bricks(9, 16) == 1 and S.lattice_indices(9, 16).tolist() == [0, 8] and S.n_bricks(17, 8) == 2


def test_arguments_are_validated_before_anything_runs():
    """ValueError for brick < 2, margin < 0 (NaN too) and dilate < 0, a bad box or resolution, and normals with dilate = 0 -- all
    before a device is asked for, so they hold here; a grid past the isosurface plan is refused the same way."""
    import nerf
    import torch
    from nerf import ops
    never = lambda pts: pytest.fail("fn must not be called")
    box = ((-1, -1, -1), (1, 1, 1), 9)
    for bad in (dict(brick=1), dict(brick=0), dict(brick=-8), dict(brick=2.5), dict(margin=-1e-9), dict(margin=float("nan")), dict(dilate=-1),
                dict(dilate=0.5), dict(chunk_points=0)):
        with pytest.raises(ValueError):
            ops.sparse_grid(never, 0.0, *box, **bad)
    with pytest.raises(ValueError):
        ops.sparse_grid(never, 0.0, (0, 0, 0), (1, 0, 1), 9)
    with pytest.raises(ValueError):
        ops.sparse_grid(never, 0.0, (0, 0, 0), (1, 1, 1), (9, 1, 9))
    with pytest.raises(ValueError, match="past the plan"):
        ops.sparse_grid(never, 0.0, (0, 0, 0), (1, 1, 1), 675)
    m = nerf.models.ConditionalBlendshapePaperNeRFModel(num_encoding_fn_xyz=10, num_encoding_fn_dir=4, include_input_dir=False)
    args = dict(lo=(-1, -1, -1), hi=(1, 1, 1), resolution=9, level=0.0)
    with pytest.raises(ValueError, match="dilate"):
        nerf.extract_mesh(m, torch.zeros(76), torch.zeros(32), brick=8, dilate=0, **args)
    for bad in (dict(brick=1), dict(brick=8, margin=-1.0), dict(brick=8, dilate=-1)):
        with pytest.raises(ValueError):
            nerf.extract_mesh(m, torch.zeros(76), torch.zeros(32), **bad, **args)
    with pytest.raises(RuntimeError):                                          # density_grid's guard: no CPU path
        nerf.density_grid_sparse(m, torch.zeros(76), torch.zeros(32), **args)
    with pytest.raises(TypeError):                                             # level has no default
        nerf.density_grid_sparse(m, torch.zeros(76), torch.zeros(32), lo=(0, 0, 0), hi=(1, 1, 1), resolution=9)
    assert ops.SparseGridStats._fields == ("bricks", "seed_bricks", "active_bricks", "points", "evaluated_points")


def test_every_declared_symbol_is_exported(hip_lib):
    """The entry points include/nerface_hip.h declares are the ones the binding has prototypes for and the library exports; the ABI
    revision is still 5; the Python names are in place."""
    import nerf
    from nerf import _hip, ops
    header = open(os.path.join(ROOT, "include", "nerface_hip.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|size_t)\s+(nf_sparse_grid_\w+)\(", header, re.M)))
    assert declared == sorted(ENTRY_POINTS)
    for name in declared:
        assert name in _hip._PROTOTYPES and name not in _hip._OPTIONAL and hasattr(hip_lib, name), name
    assert _hip.ABI_VERSION == 5 and hip_lib.nf_abi_version() == 5
    assert callable(nerf.density_grid_sparse) and callable(ops.sparse_grid) and "nf_sparse_grid.hip" in open(
        os.path.join(ROOT, "4d-facial-avatars_amd", "build.py")).read()


def test_entry_points_refuse_before_touching_the_device(hip_lib):
    """NF_EINVAL (-22) for NULL pointers, an axis below 2, brick below 2, a grid past the isosurface plan, a workspace or capacity that
    is too small, lo >= hi, a negative or NaN margin, a negative dilate and a count the grid cannot hold; the size query answers 0
    for what it does not serve.  No pointer is dereferenced on these paths, so a small integer stands in for device memory."""
    ws_bytes = hip_lib.nf_sparse_grid_workspace_bytes
    assert ws_bytes(1, 9, 9, 8) == 0 and ws_bytes(9, 9, 1, 8) == 0 and ws_bytes(9, 9, 9, 1) == 0 and ws_bytes(9, 9, 9, -8) == 0
    assert ws_bytes(675, 675, 675, 8) == 0 and ws_bytes(564, 564, 564, 8) > 0 and ws_bytes(565, 565, 565, 8) == 0
    assert ws_bytes(9, 9, 9, 2 ** 31 - 1) == ws_bytes(9, 9, 9, 8) == ws_bytes(9, 9, 9, 16)      # one brick either way
    n = ws_bytes(19, 13, 10, 4)
    bricks, blocks = 5 * 3 * 3, -(-19 * 13 * 10 // 256)
    assert n % 256 == 0 and 256 + 3 * bricks + 4 * blocks <= n <= 256 + 5 * 256
    assert ws_bytes(512, 512, 512, 8) < 512 ** 3 // 32                          # no per-point storage: three bytes per brick, four per 256 points
    P = 4096
    lo, hi = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(1, 1, 1)
    a = ctypes.addressof
    lattice = dict(nx=19, ny=13, nz=10, brick=4, lo=a(lo), hi=a(hi), index=P, coords=P, capacity=6 * 4 * 4, stream=None)
    for change in (dict(lo=None), dict(hi=None), dict(index=None), dict(coords=None), dict(nx=1), dict(brick=1), dict(capacity=6 * 4 * 4 - 1),
                   dict(nx=675, ny=675, nz=675)):
        assert hip_lib.nf_sparse_grid_lattice(*{**lattice, **change}.values()) == -22, change
    classify = dict(grid=P, nx=19, ny=13, nz=10, brick=4, level=0.0, margin=0.0, dilate=1, ws=P, ws_bytes=n, stream=None)
    for change in (dict(grid=None), dict(ws=None), dict(nz=1), dict(brick=0), dict(ws_bytes=n - 1), dict(margin=-0.5), dict(margin=float("nan")),
                   dict(dilate=-1)):
        assert hip_lib.nf_sparse_grid_classify(*{**classify, **change}.values()) == -22, change
    mark = dict(nx=19, ny=13, nz=10, brick=4, ws=P, ws_bytes=n, counts=P, stream=None)
    for change in (dict(ws=None), dict(counts=None), dict(ny=0), dict(brick=1), dict(ws_bytes=n - 1)):
        assert hip_lib.nf_sparse_grid_mark(*{**mark, **change}.values()) == -22, change
    emit = dict(grid=P, nx=19, ny=13, nz=10, brick=4, lo=a(lo), hi=a(hi), ws=P, ws_bytes=n, index=P, coords=P, capacity=5, stream=None)
    for change in (dict(grid=None), dict(lo=None), dict(hi=None), dict(ws=None), dict(index=None), dict(coords=None), dict(capacity=-1), dict(nx=1),
                   dict(brick=1), dict(ws_bytes=n - 1)):
        assert hip_lib.nf_sparse_grid_emit(*{**emit, **change}.values()) == -22, change
    for axis in range(3):
        for bad in (1.0, 2.0, float("nan")):
            lo_bad = (ctypes.c_float * 3)(-1, -1, -1)
            lo_bad[axis] = bad
            assert hip_lib.nf_sparse_grid_emit(*{**emit, "lo": a(lo_bad)}.values()) == -22
            assert hip_lib.nf_sparse_grid_lattice(*{**lattice, "lo": a(lo_bad)}.values()) == -22
    scatter = dict(values=P, index=P, count=5, grid=P, nx=19, ny=13, nz=10, stream=None)
    for change in (dict(values=None), dict(index=None), dict(grid=None), dict(count=-1), dict(count=19 * 13 * 10 + 1), dict(nx=1)):
        assert hip_lib.nf_sparse_grid_scatter(*{**scatter, **change}.values()) == -22, change
    assert hip_lib.nf_sparse_grid_scatter(None, None, 0, None, 19, 13, 10, None) == 0          # nothing to write
