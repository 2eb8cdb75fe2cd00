"""The CMA-ES of the acquisition search's refinement on the CPU: the NumPy statement tests/cmaes_host.py against known
optima, its determinism and stop rules, pyvbmc_amd/cmaes.py against it (bit for bit), and the two conditions that make
the GPU replay (tests/test_search_cmaes_gpu.py) certain -- the margins between ranked values and the twin's drift.

Margins: over a whole run of every replay case the smallest gap between neighbouring ranked values is at least 1000 times
the acquisition parity bound the project asserts (1e-9 max(1, |value|), tests/test_search_gpu.py): the device's values then
rank as the host's do.  Exact ties are allowed between bitwise identical evaluated rows (the update is the same either
way) and between non-finite values (+inf from the hard-bound mask on both sides; the index decides).  The seeds were
chosen on the CPU (tools/search_cmaes_seeds.py).

Drift: the twin multiplies every operation in which the device's arithmetic differs by 1 + 4 eps xi.  The GPU tolerance
is 100 times the twin's deviation per quantity, computed from the twin (cmaes_host.drift_bounds), never hard-coded.
"""
import math

import cmaes_host as ch
import numpy as np
import pytest

from pyvbmc_amd import cmaes

CASES = list(ch.SPECS)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def runs(golden):
    """Every replay case and its run of the statement, computed once."""
    out = {}
    for name in CASES:
        k = ch.build_case(name, golden)
        out[name] = (k, ch.replay(k))
    return out


# ---------------------------------------------------------------------------------------------- the cases
def test_case_shapes(runs):
    lam = {n: runs[n][0].lam for n in CASES}
    assert lam["d2"] == 6 and lam["d32"] == 14 and lam["lam64"] == 64 and runs["d5"][0].D == 5
    k, es = runs["b_int"]
    assert k.state["integer_vars"].sum() == 1
    # the start's neighbourhood crosses a hard bound: some candidates were masked, the best never was
    masked = sum(int(np.isposinf(v).sum()) for _, v in es.history)
    assert masked > 0 and np.isfinite(es.f_best)
    assert not ch.sh.hard_bound_mask(es.x_best[None, :], k.case.pt, k.state)[0]
    xo = k.case.pt.inverse(es.x_best[None, :])[0]
    assert abs(xo[1] - round(xo[1])) < 1e-9  # the best point's integer column is integral in original space
    for name in CASES:
        k, es = runs[name]
        assert es.stop in (1, 2, 3) and es.generations >= 5, (name, es.stats)
        assert es.f_best <= es.f0 and np.all(es.x_best >= k.lb) and np.all(es.x_best <= k.ub)
    assert any(runs[n][1].stop == 1 for n in CASES)  # a run that ends by tolfun is among them


@pytest.mark.parametrize("name", CASES)
def test_margins(runs, name):
    k, es = runs[name]
    print(name, "stats", es.stats.tolist(), "smallest ranked gap", es.gap, "=", es.gap / ch.PARITY, "parity bounds")
    assert es.tied_rows_only
    assert es.gap >= 1000 * ch.PARITY


@pytest.mark.parametrize("name", CASES)
def test_twin_keeps_the_ranks_and_measures_the_drift(runs, name):
    k, es = runs[name]
    bounds, dev, same = ch.drift_bounds(k, es)
    print(name, "twin deviation", {q: f"{v:.2e}" for q, v in dev.items()}, "GPU bounds", {q: f"{v:.2e}" for q, v in bounds.items()})
    assert same
    # the recursion must not amplify rounding into something a tolerance could not tell from a wrong update
    assert all(v < 1e-9 for v in bounds.values())


# ---------------------------------------------------------------------------------------------- known optima
def quadratic(centre, scale):
    return lambda X: np.sum(scale * (np.asarray(X) - centre) ** 2, axis=1)


@pytest.mark.parametrize("where", ["interior", "face"])
@pytest.mark.parametrize("D", [2, 3, 6])
def test_convex_quadratic_in_a_box(D, where):
    r = np.random.default_rng(D)
    lb, ub = np.full(D, -2.0), np.full(D, 3.0)
    centre = r.uniform(-1.0, 2.0, D)
    if where == "face":
        centre[0] = 4.5  # outside: the optimum lies on the face x_0 = ub_0
    scale = 1.0 + 9.0 * r.random(D)
    f = quadratic(centre, scale)
    x_opt = np.minimum(np.maximum(centre, lb), ub)
    f_opt = float(f(x_opt[None, :])[0])
    tol_fun = 1e-8
    es = ch.run(ch.CMAES(r.uniform(-1.5, 2.5, D), 1.0, lb, ub, max_fevals=500 * (D + 2), tol_fun=tol_fun, seed=11), f)
    print(D, where, es.stats.tolist(), es.f_best - f_opt)
    assert es.stop in (1, 2)
    assert 0.0 <= es.f_best - f_opt <= 10 * tol_fun
    assert np.all(es.x_best >= lb) and np.all(es.x_best <= ub)
    if where == "face":
        assert abs(es.x_best[0] - ub[0]) < 1e-3


# ---------------------------------------------------------------------------------------------- determinism
def test_same_seed_same_bits_and_runs_are_independent(runs):
    k, es = runs["d5"]
    again = ch.replay(k)
    assert np.array_equal(es.stats, again.stats)
    for q in ("x_best", "mean", "C"):
        assert np.array_equal(bits(getattr(es, q)), bits(getattr(again, q)))
    assert es.sigma == again.sigma and es.f_best == again.f_best
    # run r depends on its own start and sub_seed(seed, r) only
    assert ch.run_key(k.seed, 0) == cmaes.sub_seed(k.seed, 0) and ch.run_key(k.seed, 3) == (k.seed + 4 * ch.KEY_STEP) % 2**64
    other = ch.replay(k, run_index=1)
    assert not np.array_equal(bits(es.mean), bits(other.mean))
    es3 = ch.CMAES(k.x0, k.sigma0, k.lb, k.ub, lam=k.lam, max_fevals=k.max_fevals, tol_fun=k.tol_fun,
                   seed=(k.seed + ch.KEY_STEP) % 2**64, run=0)
    ch.run(es3, ch.objective(k), ch.evaluated(k))
    assert np.array_equal(bits(es3.mean), bits(other.mean)) and np.array_equal(es3.stats, other.stats)


# ---------------------------------------------------------------------------------------------- stop reasons
def stop_case(reason):
    """A small constructed input that ends with the given reason: (f, x0, sigma0, lb, ub, keywords)."""
    lb, ub = np.full(2, -5.0), np.full(2, 5.0)
    sphere = quadratic(np.zeros(2), np.ones(2))
    if reason == 1:  # a flat function: every range is zero
        return lambda X: np.zeros(len(X)), np.zeros(2), 1.0, lb, ub, dict(max_fevals=10000, tol_fun=1e-3)
    if reason == 2:  # a generous tol_x, a negative tol_fun that never holds
        return sphere, np.ones(2), 1.0, lb, ub, dict(max_fevals=10000, tol_fun=-1.0, tol_x=0.5)
    if reason == 3:
        return sphere, np.ones(2), 1.0, lb, ub, dict(max_fevals=1 + 6 * 3, tol_fun=-1.0)
    if reason == 4:  # a ridge: one direction collapses, nothing else stops the run
        return (lambda X: 1e6 * np.asarray(X)[:, 0] ** 2 + 1e-9 * np.asarray(X)[:, 1]), np.array([1.0, 0.0]), 1.0, np.full(2, -1e30), \
            np.full(2, 1e30), dict(max_fevals=10**6, tol_fun=-1.0, tol_x=1e-300)
    return lambda X: np.full(len(X), np.inf) if len(X) > 1 else np.zeros(1), np.zeros(2), 1.0, lb, ub, dict(max_fevals=10000, tol_fun=1e-3)


@pytest.mark.parametrize("reason", [1, 2, 3, 4, 5])
def test_stop_reasons(reason):
    f, x0, sigma0, lb, ub, kw = stop_case(reason)
    es = ch.run(ch.CMAES(x0, sigma0, lb, ub, seed=5, **kw), f)
    print(reason, cmaes.STOP_REASONS[reason], es.stats.tolist())
    assert es.stop == reason
    res = cmaes.fmin(f, x0, sigma0, lb, ub, seed=5, **kw)
    assert np.array_equal(res.stats, es.stats)
    if reason == 3:
        assert es.evaluations == 19 and es.generations == 3
    if reason == 5:
        assert es.generations == 1 and es.f_best == es.f0 == 0.0
    # a start whose value is not finite ends at once
    bad = ch.run(ch.CMAES(x0, sigma0, lb, ub, seed=5, **kw), lambda X: np.full(len(X), np.nan))
    assert bad.stats.tolist() == [0, 1, 5, 0]


# ---------------------------------------------------------------------------------------------- product NumPy
@pytest.mark.parametrize("name", CASES)
def test_product_fmin_equals_the_statement(runs, name):
    k, es = runs[name]
    res = cmaes.fmin(ch.objective(k), k.x0, k.sigma0, k.lb, k.ub, lam=k.lam, max_fevals=k.max_fevals, tol_fun=k.tol_fun,
                     seed=k.seed, evaluated=ch.evaluated(k))
    assert np.array_equal(res.stats, es.stats)
    assert res.f_best == es.f_best and res.f0 == es.f0 and res.sigma == es.sigma
    for q in ("x_best", "mean", "C"):
        assert np.array_equal(bits(getattr(res, q)), bits(getattr(es, q))), q


def test_product_constants_and_draws():
    for D, lam in ((2, 6), (5, 8), (32, 14), (4, 64)):
        c = cmaes.constants(D, lam)
        es = ch.CMAES(np.zeros(D), 1.0, -np.ones(D), np.ones(D), lam=lam, max_fevals=1000, tol_fun=1e-3, seed=1)
        assert cmaes.default_lambda(D) == 4 + int(math.floor(3 * math.log(D)))
        assert np.array_equal(bits(c.w), bits(np.array(es.w))) and abs(sum(es.w) - 1.0) < 1e-15
        assert (c.mueff, c.cs, c.ds, c.cc, c.c1, c.cmu, c.chi, c.hist) == (es.mueff, es.cs, es.ds, es.cc, es.c1, es.cmu, es.chi, es.hist)
        z = cmaes.normals(3 * lam, lam, D, ch.run_key(9, 2))
        zr = ch.philox_ref.normals(np.arange(3 * lam, 4 * lam, dtype=np.uint64), D, ch.run_key(9, 2), ch.STREAM)
        assert np.array_equal(bits(z), bits(zr))
    with pytest.raises(ValueError):
        cmaes.fmin(lambda X: np.zeros(len(X)), np.zeros(1), 1.0, [-1.0], [1.0], max_fevals=100, tol_fun=1e-3, seed=1)
