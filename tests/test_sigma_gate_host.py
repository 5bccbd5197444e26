"""CPU: the sigma gate's restatement (tests/sigma_bound_ref.py) is sound against float64, and the host model of the live-colour
schedule (tests/live_schedule_ref.py) holds with "not proven dead" in place of "live"."""
import numpy as np
import pytest
import torch

from oracle import cases as C
from oracle import nerface_oracle as O
from tests import live_schedule_ref as M
from tests import sigma_bound_ref as B
from tests.test_gpu_live_colour import _points
from tests.test_gpu_live_fill import BIASES


def _x87(n_rays, s, seed):
    ro, rd, z = _points(n_rays, s, seed)
    return O.encode_points(ro, rd, z, O.NEAR, O.FAR).reshape(-1, 87)


def _conditioning():
    c = C.build_case("eval_det_64_128")
    return c["expr"], c["latent"]


def _sigma64_of(p, h):
    """sigma_raw in float64 from the float32 h the gate saw: what the bound is a bound on."""
    q = {k: p[k].double() for k in ("fc_feat.weight", "fc_feat.bias", "fc_alpha.weight", "fc_alpha.bias")}
    feat = h.double() @ q["fc_feat.weight"].t() + q["fc_feat.bias"]
    return (feat @ q["fc_alpha.weight"].t() + q["fc_alpha.bias"]).reshape(-1).numpy()


def _sound(p, x87, expr, latent):
    """-> (dead share, unproven share of the dead rows); asserts that no proven row has sigma >= 0, in float64 and as float32 computes it."""
    h, sigma32 = B.trunk(p, x87, expr, latent)
    s, u, bound, proven = B.gate(h.numpy(), *B.bound_vectors(p))
    sigma64 = _sigma64_of(p, h)
    assert not bool((proven & ~(sigma64 < 0)).any())
    assert not bool((proven & ~(sigma32.numpy() <= 0)).any())
    assert bool((sigma64[proven] <= bound[proven].astype(np.float64)).all())          # it IS an upper bound
    assert bool((bound[proven] < 0).all()) and not bool(np.isnan(bound[proven]).any())
    dead = sigma64 <= 0
    return float(dead.mean()), float((dead & ~proven).sum() / max(1, dead.sum()))


@pytest.mark.parametrize("boost", [True, "survey"], ids=["x1000", "x40"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_nets_are_never_proven_wrongly(seed, boost):
    expr, latent = _conditioning()
    p = O.init_paper_params(seed, boost=boost)
    x87 = _x87(64, 32, 50 + seed)
    _, sigma = B.trunk(p, x87, expr, latent, torch.float64)                     # the bias at the 70 % quantile: both sides of zero are populated
    p["fc_alpha.bias"] = p["fc_alpha.bias"] - float(torch.quantile(sigma, 0.7))
    dead, unproven = _sound(p, x87, expr, latent)
    print(f"seed {seed} head {boost}: dead {dead:.3f}, unproven share of the dead rows {unproven:.4f}")
    assert 0.6 < dead < 0.8


def test_cancelling_net_is_never_proven_wrongly():
    """fc_alpha.weight x 1e-3 and the bias at minus the median density: sigma is a small difference, densities crowd around zero.
    Whatever the gate proves there it proves rightly; the share it leaves unproven is printed."""
    expr, latent = _conditioning()
    x87 = _x87(64, 32, 57)
    p = B.cancelling(O.init_paper_params(1, boost=True), x87, expr, latent)
    dead, unproven = _sound(p, x87, expr, latent)
    print(f"cancelling net: dead {dead:.3f}, unproven share of the dead rows {unproven:.4f}")
    assert 0.4 < dead < 0.6


@pytest.mark.parametrize("where", ["fc_alpha.weight", "fc_alpha.bias", "fc_feat.weight", "fc_feat.bias"])
@pytest.mark.parametrize("what", [float("nan"), float("inf"), float("-inf")])
def test_nan_and_inf_prove_nothing(where, what):
    expr, latent = _conditioning()
    x87 = _x87(16, 32, 58)
    p = O.init_paper_params(1, boost=True)
    p["fc_alpha.bias"] = torch.full_like(p["fc_alpha.bias"], -50.0)            # (finite, this net proves nearly every row)
    h, _ = B.trunk(p, x87, expr, latent)
    assert B.gate(h.numpy(), *B.bound_vectors(p))[3].mean() > 0.9
    p[where] = p[where].clone()
    p[where].reshape(-1)[-1] = what
    # (fc_feat.weight: one w[k], v[k] is not finite; every row's s and u are then NaN or infinite, whether h[k] is zero or not)
    assert not bool(B.gate(h.numpy(), *B.bound_vectors(p))[3].any())


def test_the_inputs_of_the_gpu_tests_leave_few_dead_rows_unproven():
    """A condition on the inputs of tests/test_gpu_sigma_gate.py's 2048-point cases, not a measurement: over the ten biases the
    restatement's own unproven share of the dead rows (sigma <= 0 in float64, not a ray's last sample) stays under one quarter."""
    c = C.build_case("eval_det_64_128")
    n_rays, s = 32, 64
    x87 = _x87(n_rays, s, 41)
    dead_all = unproven_all = 0
    for bias in BIASES:
        p = {k: v.clone() for k, v in c["p_fine"].items()}
        p["fc_alpha.bias"] = torch.full_like(p["fc_alpha.bias"], bias)
        h, _ = B.trunk(p, x87, c["expr"], c["latent"])
        dead = _sigma64_of(p, h) <= 0
        dead[s - 1::s] = False
        proven = B.gate(h.numpy(), *B.bound_vectors(p))[3]
        proven[s - 1::s] = False
        assert not bool((proven & ~dead).any()), bias
        dead_all += int(dead.sum())
        unproven_all += int((dead & ~proven).sum())
    print(f"unproven share of the dead rows: {unproven_all} / {dead_all}")
    assert unproven_all < 0.25 * dead_all


@pytest.mark.parametrize("grid", [1, 2, 256])
@pytest.mark.parametrize("extra", [0.0, 0.02, 0.3])
def test_schedule_model_holds_with_not_proven_in_place_of_live(extra, grid):
    """The rows the gate keeps are the live rows and some dead ones (`extra`: the share of the dead rows it could not prove).  The
    model of fill / append / flush takes any mask: every kept row is gathered exactly once, no proven row ever is, the ring's bounds
    hold (asserted inside replay), and the live rows are among the gathered ones."""
    rng = np.random.default_rng(7)
    n_rays, s = 67, 11
    n = n_rays * s
    sig_pos = rng.random(n) < 0.4
    kept = sig_pos | (rng.random(n) < extra)
    passes, gathered = M.replay(kept, n, s, grid)
    want = M.live_points(kept, n, s)
    assert np.array_equal(gathered.astype(bool), want) and int(gathered.max()) == 1
    assert not bool((M.live_points(sig_pos, n, s) & ~gathered.astype(bool)).any())
    assert len(passes) >= (n + 31) // 32
