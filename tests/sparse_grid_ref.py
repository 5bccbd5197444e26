"""NumPy restatement of the sparse-grid specification (DESIGN.md "Sparse density grid"): from a DENSE array of values v[nz][ny][nx],
which bricks are seeds, which are active, which points are evaluated, and the grid ops.sparse_grid must return.  The tests compare
the library against it; nothing in the product imports it.

    restate(v, level, brick, margin=0.0, dilate=1) -> Sparse(seed, active, side, lattice, evaluated, grid)
    one_sided(v, level, brick, seed)               -> the precondition of the guarantee: every brick that is no seed lies on one side
"""
from typing import NamedTuple

import numpy as np


class Sparse(NamedTuple):
    seed: np.ndarray          # (mz, my, mx) bool
    active: np.ndarray        # (mz, my, mx) bool
    side: np.ndarray          # (mz, my, mx) bool: all 8 corners > level + margin (meaningful where the brick is no seed)
    lattice: np.ndarray       # (nz, ny, nx) bool: the brick corners
    evaluated: np.ndarray     # (nz, ny, nx) bool: the lattice and every point of every active brick
    grid: np.ndarray          # (nz, ny, nx) float32: v where evaluated, +inf / -inf elsewhere


def n_bricks(n, brick):
    return -(-(n - 1) // brick)


def brick_range(b, n, brick):
    """Point indices [first, last] of brick b on an axis of n points, both included."""
    return brick * b, min(brick * (b + 1), n - 1)


def lattice_indices(n, brick):
    return np.array(sorted(set(range(0, n, brick)) | {n - 1}), dtype=np.int64)


def _regions(shape, brick):
    nz, ny, nx = shape
    for bz in range(n_bricks(nz, brick)):
        for by in range(n_bricks(ny, brick)):
            for bx in range(n_bricks(nx, brick)):
                (z0, z1), (y0, y1), (x0, x1) = brick_range(bz, nz, brick), brick_range(by, ny, brick), brick_range(bx, nx, brick)
                yield (bz, by, bx), (slice(z0, z1 + 1), slice(y0, y1 + 1), slice(x0, x1 + 1))


def restate(v, level, brick, margin=0.0, dilate=1):
    v = np.ascontiguousarray(v, dtype=np.float32)
    nz, ny, nx = v.shape
    assert min(v.shape) >= 2 and brick >= 2 and margin >= 0 and dilate >= 0
    cz, cy, cx = (lattice_indices(n, brick) for n in (nz, ny, nx))
    mz, my, mx = (n_bricks(n, brick) for n in (nz, ny, nx))
    assert (len(cz), len(cy), len(cx)) == (mz + 1, my + 1, mx + 1)
    above, below = np.float32(level) + np.float32(margin), np.float32(level) - np.float32(margin)
    with np.errstate(invalid="ignore"):
        corner = v[np.ix_(cz, cy, cx)]
        eight = np.stack([corner[dz:mz + dz, dy:my + dy, dx:mx + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)])
        all_in, all_out = (eight > above).all(axis=0), (eight < below).all(axis=0)          # a NaN corner fails both
    seed = ~(all_in | all_out)
    active = np.zeros_like(seed)
    for bz, by, bx in zip(*np.nonzero(seed)):                                               # Chebyshev distance <= dilate
        active[max(bz - dilate, 0):bz + dilate + 1, max(by - dilate, 0):by + dilate + 1, max(bx - dilate, 0):bx + dilate + 1] = True
    lattice = np.zeros(v.shape, dtype=bool)
    lattice[np.ix_(cz, cy, cx)] = True
    evaluated = lattice.copy()
    fill = np.zeros(v.shape, dtype=np.float32)
    for b, region in _regions(v.shape, brick):
        if active[b]:
            evaluated[region] = True
        else:
            fill[region] = np.float32(np.inf) if all_in[b] else np.float32(-np.inf)
    # a point that is not evaluated lies only in bricks that are not active, hence no seeds: they share a corner and agree
    return Sparse(seed, active, all_in, lattice, evaluated, np.where(evaluated, v, fill).astype(np.float32))


def one_sided(v, level, brick, seed):
    """True iff every brick that is no seed has all of its points inside (v > level) or all of them outside."""
    with np.errstate(invalid="ignore"):
        inside = np.asarray(v, dtype=np.float32) > np.float32(level)
    for b, region in _regions(inside.shape, brick):
        if not seed[b] and inside[region].any() and not inside[region].all():
            return False
    return True


# ---- the fields of the tests: 33^3 points on [-1, 1]^3 in bricks of 8 cells (4 per axis, 0.5 wide).  Both surfaces pass through
# brick corners and stay in the lower z bricks, so that with dilate = 1 a quarter of the bricks stays inactive; that every brick
# without a crossing corner pair lies on one side is checked by the tests (one_sided), not assumed.
FIELD_N, FIELD_LO, FIELD_HI, FIELD_BRICK = (33, 33, 33), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 8
SPHERE = dict(centre=(-0.45, -0.5, -0.55), r=0.41)          # seeds: the 8 bricks round the corner (-0.5, -0.5, -0.5)
TORUS = dict(centre=(0.0, 0.0, -0.5), big=0.5, small=0.2)   # the ring passes through (+-0.5, 0, -0.5) and (0, +-0.5, -0.5)


def sphere_field(x, y, z, centre=SPHERE["centre"], r=SPHERE["r"]):
    """r^2 - |p - centre|^2 in float32, with operations NumPy arrays and torch tensors share."""
    dx, dy, dz = x - centre[0], y - centre[1], z - centre[2]
    return r * r - (dx * dx + dy * dy + dz * dz)


def torus_field(x, y, z, centre=TORUS["centre"], big=TORUS["big"], small=TORUS["small"]):
    dx, dy, dz = x - centre[0], y - centre[1], z - centre[2]
    q = (dx * dx + dy * dy) ** 0.5 - big
    return small * small - (q * q + dz * dz)
