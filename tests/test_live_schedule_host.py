"""The host model of the live-colour kernel's schedule (tests/live_schedule_ref.py) on hand-made liveness masks: every branch of a
pass is driven, and the model's invariants hold -- 0 <= R <= 31, every live point is coloured exactly once and no dead one, ring rows
are consumed oldest first.  Also: the constants the model takes from nerf.ops agree with the library's scratch sizing.  No GPU."""
import numpy as np
import pytest

from tests import live_schedule_ref as M


def _check(passes, coloured, live):
    assert np.array_equal(coloured, live.astype(np.int64))                   # live: exactly once; dead: never
    waves = {}
    for p in passes:
        waves.setdefault((p.wg, p.wave), []).append(p)
    for ps in waves.values():
        assert [p.k for p in ps] == sorted(p.k for p in ps)
        ring = []
        for p in ps:
            assert 0 <= p.R <= 31 and p.R == len(ring), (p.R, len(ring))
            assert p.from_registers + p.loaded == len(p.taken)
            if p.branch == "append":
                assert p.R < p.D and p.R + p.L <= 31 and not p.taken
                ring += p.appended
            else:
                n = p.D if p.branch == "fill" else p.R
                assert (p.R >= p.D) if p.branch == "fill" else (p is ps[-1] and p.R > 0)
                assert p.taken == ring[:n]                                     # oldest first
                ring = ring[n:]
        assert not ring                                                        # the flush leaves nothing behind


def _wave_mask(counts_per_wave, n_passes):
    """One workgroup, one ray: pass k of wave w covers points [128 k + 32 w, + 32); its first counts_per_wave[w][k] points are live."""
    live = np.zeros(128 * n_passes, dtype=bool)
    for w, counts in enumerate(counts_per_wave):
        for k, c in enumerate(counts):
            live[128 * k + 32 * w:128 * k + 32 * w + c] = True
    return live


def test_hand_made_masks_drive_every_branch(hip_lib):
    from nerf import ops
    assert ops.LIVE_PREFETCH_ROWS < 27
    wave0 = [20, 11, 0, 1, 32, 5, 32, 27, 1]
    live = _wave_mask([wave0, [30] + [0] * 8, [0] * 9, [0] * 9], 9)
    n = live.size
    passes, coloured = M.replay(live, n, n, 1)
    full = M.live_points(live, n, n)
    assert full.sum() == live.sum() + 1                                        # the ray's last sample
    _check(passes, coloured, full)
    w0 = [p for p in passes if p.wave == 0]
    assert [p.branch for p in w0] == ["append", "append", "append", "fill", "fill", "append", "fill", "fill", "append", "flush"]
    assert [p.R for p in w0] == [0, 20, 31, 31, 0, 0, 5, 5, 0, 1]
    assert (w0[3].D, w0[3].from_registers, w0[3].loaded) == (31, ops.LIVE_PREFETCH_ROWS, 31 - ops.LIVE_PREFETCH_ROWS)
    assert (w0[7].D, w0[7].from_registers, w0[7].loaded) == (5, min(5, ops.LIVE_PREFETCH_ROWS), max(0, 5 - ops.LIVE_PREFETCH_ROWS))
    w1 = [p for p in passes if p.wave == 1]
    assert w1[-1].branch == "flush" and w1[-1].R == 30 and all(p.branch == "append" for p in w1[:-1])
    assert [p.branch for p in passes if p.wave == 2] == ["append"] * 9          # nothing live: no colour run at all
    w3 = [p for p in passes if p.wave == 3]
    assert w3[-1].branch == "flush" and w3[-1].taken == [n - 1]
    hit = M.branches(passes)
    assert M.REQUIRED <= hit and "all_live_R_zero" in hit, M.REQUIRED - hit


@pytest.mark.parametrize("n_rays,S,grid", [(1, 1, 1), (13, 5, 1), (64, 32, 1), (64, 32, 2), (64, 32, 5), (1000, 37, 290), (96, 64, 7)])
@pytest.mark.parametrize("frac", [0.0, 0.03, 0.5, 0.97, 1.0])
def test_random_masks_keep_the_invariants(hip_lib, n_rays, S, grid, frac):
    """Ragged sizes, several workgroups (the block rotation), live fractions from none to all."""
    n = n_rays * S
    live = np.random.default_rng(7 + n + grid).random(n) < frac
    passes, coloured = M.replay(live, n, S, grid)
    _check(passes, coloured, M.live_points(live, n, S))
    G = min(grid, (n + 127) // 128)
    assert {p.wg for p in passes} <= set(range(G))
    blocks = sorted((p.k, p.wg) for p in passes if p.wave == 0 and p.branch != "flush")
    assert len(blocks) == (n + 127) // 128                                     # the rotation visits every block once


def test_constants_agree_with_the_scratch_size(hip_lib):
    from nerf import ops
    size = hip_lib.nf_paper_mlp_fwd_live_scratch_floats
    assert size(1) == M.WAVES * ops.LIVE_RING_ROWS * ops.LIVE_ROW_BYTES // 4
    assert size(3) == 3 * size(1)
    assert ops.LIVE_RING_ROWS >= 2 * M.ROWS - 1 and 0 <= ops.LIVE_PREFETCH_ROWS <= M.ROWS
    assert [ops.live_rotation_step(g) for g in (1, 2, 3, 13, 256)] == [0, 1, 1, 5, 99]
