"""CPU tests of tests/slice_host.py, the NumPy statement of the slice sampler that ``vbmc_is_mcmc`` runs on the device:
its law on a target with known moments, and the preconditions under which the GPU replay
(tests/test_ais_mcmc_gpu.py) is certain to take the host's decisions."""
import numpy as np
import pytest

import ais_mcmc_cases as cases
import slice_host

RHO = 0.8
LB, UB = np.array([-0.5, -4.0]), np.array([4.0, 4.0])  # the box cuts the left tail of the first coordinate
PREC = np.linalg.inv(np.array([[1.0, RHO], [RHO, 1.0]]))


def log_gauss(x):
    return -0.5 * x @ PREC @ x


def truncated_moments():
    """Mean and covariance of the truncated law by the midpoint rule on a 1600 x 1600 grid of the box (the integrand is
    smooth inside it: the rule's error, O(h^2) with h = 0.003 / 0.005, is far below the chain's standard errors)."""
    g = [np.linspace(lo, hi, 1601) for lo, hi in zip(LB, UB)]
    m = [0.5 * (a[1:] + a[:-1]) for a in g]
    A, B = np.meshgrid(m[0], m[1], indexing="ij")
    w = np.exp(-0.5 * (PREC[0, 0] * A * A + 2 * PREC[0, 1] * A * B + PREC[1, 1] * B * B))
    w /= w.sum()
    mean = np.array([(w * A).sum(), (w * B).sum()])
    dA, dB = A - mean[0], B - mean[1]
    return mean, np.array([[(w * dA * dA).sum(), (w * dA * dB).sum()], [(w * dA * dB).sum(), (w * dB * dB).sum()]])


def batch_se(v, nb=40):
    """Standard error of the mean of the correlated series ``v`` from the means of ``nb`` consecutive batches (that is:
    with the effective sample size the batch means imply)."""
    b = v[: len(v) // nb * nb].reshape(nb, -1).mean(axis=1)
    return b.std(ddof=1) / np.sqrt(nb)


def test_law_on_a_truncated_correlated_gaussian():
    """4 000 kept samples, thin 2, fixed key: mean and covariance within 5 batch-means standard errors of the truncated
    law's.  The chain is a pure function of its key, so the outcome cannot change from run to run."""
    res = slice_host.chain(log_gauss, [0.5, 0.5], [1.5, 1.5], LB, UB, 4000, thin=2, burn_in=200, seed=1)
    X = res["samples"]
    assert X.shape == (4000, 2) and np.all(X >= LB) and np.all(X <= UB)
    assert res["stats"][2] == 0 and res["stats"][3] == 0
    np.testing.assert_array_equal(res["f_vals"], [log_gauss(x) for x in X])  # the f(x) in hand is f at the kept point
    mean, cov = truncated_moments()
    for d in range(2):
        err, se = abs(X[:, d].mean() - mean[d]), batch_se(X[:, d])
        print(f"mean[{d}]: chain {X[:, d].mean():.4f}, law {mean[d]:.4f}, |err| = {err / se:.2f} se")
        assert err <= 5 * se
    for i, j in ((0, 0), (0, 1), (1, 1)):
        prod = (X[:, i] - mean[i]) * (X[:, j] - mean[j])
        err, se = abs(prod.mean() - cov[i, j]), batch_se(prod)
        print(f"cov[{i}{j}]: chain {prod.mean():.4f}, law {cov[i, j]:.4f}, |err| = {err / se:.2f} se")
        assert err <= 5 * se


def test_draw_stream_and_sampler_class():
    """Draw i of chain s is a function of (seed, s, i) alone; the class hands out the chain indices in construction order."""
    a, b = slice_host.Draws(7, 2), slice_host.Draws(7, 2)
    ua = [a.u_pos(), a.u(), a.u()]
    b.i = 1
    assert b.u() == ua[1] and 0.0 < ua[0] <= 1.0 and 0.0 <= ua[1] < 1.0
    assert slice_host.Draws(7, 3).u() != slice_host.Draws(7, 2).u() != slice_host.Draws(8, 2).u()
    cls = slice_host.sampler_class(5)
    first, second = (cls(log_gauss, [0.1, 0.2], [1.0, 1.0], LB, UB, {}) for _ in range(2))
    out = second.sample(6, 2, 3)
    ref = slice_host.chain(log_gauss, [0.1, 0.2], [1.0, 1.0], LB, UB, 6, 2, 3, seed=5, s=1)
    assert first.s == 0 and np.array_equal(out["samples"], ref["samples"]) and np.array_equal(out["f_vals"], ref["f_vals"])
    assert out["samples"].shape == (6, 2) and len(cls.results) == 1
    with pytest.raises(ValueError, match="Invalid value."):
        slice_host.chain(lambda x: np.nan, [0.0, 0.0], [1.0, 1.0], LB, UB, 2)


def test_caps_bound_every_loop():
    """A target that is never below the level steps out to both caps (the box is wider than 32 widths), one that is never
    above it exhausts the shrink cap and leaves the point where it was."""
    wide = slice_host.chain(lambda x: 0.0 if abs(x[0]) < 1e3 else -np.inf, [0.0], [1.0], [-1e3], [1e3], 1, seed=3)
    assert wide["stats"][2] == 2 and wide["stats"][0] == 1 + 2 * slice_host.OUT_CAP + 1
    calls = [0]

    def first_only(x):
        calls[0] += 1
        return 0.0 if calls[0] == 1 else -np.inf

    stuck = slice_host.chain(first_only, [0.25], [1.0], [0.0], [1.0], 1, seed=3)
    assert stuck["stats"][3] == 1 and stuck["samples"][0, 0] == 0.25
    # f(x0); the interval is as wide as the box, so one end is clipped to a bound and the other evaluated; 64 proposals
    assert stuck["stats"][0] == 1 + 1 + slice_host.SHRINK_CAP


@pytest.mark.parametrize("name,kind", cases.CASES)
def test_replay_preconditions(name, kind):
    """Every comparison f <=> ly of every chain of a replay case has a margin >= 1e-6 -- orders of magnitude above what
    f on the device can differ from f here (1e-10 relative) -- and no cap is hit: the device takes the same decisions."""
    with np.errstate(all="ignore"):
        chains, _, _ = cases.host_replay(name, kind)
    margin = min(c["margin"] for c in chains)
    evals = [int(c["stats"][0]) for c in chains]
    print(f"{name} {kind}: evaluations per chain {evals}, smallest |f - ly| = {margin:.2e}")
    assert margin >= 1e-6
    for c in chains:
        assert c["stats"][2] == 0 and c["stats"][3] == 0


def test_kept_points_depend_on_decisions_only():
    """f perturbed by 1e-10 relative -- the size of the device's error -- moves no kept point: a point is made of draws,
    widths and bounds, f only decides.  (What justifies the replay's bound on X, 1e-12 of the box.)"""
    name, kind = "d3_n70", cases.KINDS[0]
    with np.errstate(all="ignore"):
        base, _, _ = cases.host_replay(name, kind)
        moved = cases.run_host(name, kind, cases.SEEDS[(name, kind)], scale=1.0 + 1e-10)
    for a, b in zip(base, moved):
        assert np.array_equal(a["samples"], b["samples"]) and np.array_equal(a["stats"], b["stats"])
        assert not np.array_equal(a["f_vals"], b["f_vals"])
