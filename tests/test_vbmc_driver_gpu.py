"""``VBMC.optimize`` end to end on the device (pyvbmc_amd/vbmc.py): whole inferences on small problems, every stage the
package's own -- the first tests in which one stage's output feeds the next.

Problems and bounds (tests/vbmc_driver_cases.py): the reference's own end-to-end tests at D = 2 with its own bound, 0.5 on
the RMS error of the posterior mean and on ``|elbo - lnZ|`` (testing/vbmc/test_vbmc_optimize.py:125-126).  The budgets, the
seeds and what was measured before they were fixed: profiles/vbmc_driver.md.

Every run is deterministic by its seed, so a run is made once (module-scoped fixtures) and shared by the tests on it.
"""
import numpy as np
import pytest
import vbmc_driver_cases as cases

pytestmark = pytest.mark.gpu

BUDGET = 60
SEED = 1
RESULT_KEYS = ("function", "problem_type", "iterations", "func_count", "best_iter", "train_set_size", "components", "r_index",
               "convergence_status", "overhead", "rng_state", "algorithm", "version", "message", "elbo", "elbo_sd",
               "success_flag")


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


class Run:
    """One finished inference with what ``on_iteration`` saw in every iteration."""

    def __init__(self, case, seed, ctx):
        self.case = case
        self.driver = cases.make(case, seed, ctx=ctx)
        self.seen = []
        self.vp, self.results = self.driver.optimize(on_iteration=self.look)

    def look(self, d):
        """The reference's per-iteration invariants (test_vbmc_optimize.py:12-26), and a snapshot."""
        log = d.function_logger
        self.seen.append(dict(
            iter=d.iteration, K=int(d.vp.K), K_agrees=d.vp.K == d.optim_state["vp_K"],
            one_transformer=d.parameter_transformer is d.vp.parameter_transformer is log.parameter_transformer,
            warmup=bool(d.optim_state["warmup"]), n_flag=int(np.sum(log.X_flag)), gp_N=int(d.gp.X.shape[0]),
            func_count=int(log.func_count), optimize_weights=bool(d.vp.optimize_weights), Xn=int(log.Xn)))


def check_run(run, budget):
    d, h, res = run.driver, run.driver.iteration_history, run.results
    n_iter = d.iteration + 1
    assert len(run.seen) == n_iter and [s["iter"] for s in run.seen] == list(range(n_iter))
    assert all(s["K_agrees"] and s["one_transformer"] for s in run.seen)
    assert d.function_logger.func_count == budget == res["func_count"]
    assert res["message"] == "Inference terminated: reached maximum number of function evaluations options.max_fun_evals."
    from pyvbmc_amd.vbmc import HISTORY_KEYS

    assert set(h) == set(HISTORY_KEYS)
    for k in HISTORY_KEYS:
        assert len(h[k]) == n_iter, k
    elbo, sd, skl = (np.array(h[k], dtype=np.float64) for k in ("elbo", "elbo_sd", "sKL"))
    assert np.all(np.isfinite(elbo)) and np.all(sd >= 0) and np.all(skl >= 0) and np.all(np.isfinite(skl))
    assert all(k in res for k in RESULT_KEYS)
    assert np.isfinite(res["elbo"]) and res["elbo_sd"] >= 0 and res["iterations"] == d.iteration
    assert res["components"] == run.vp.K and 0 <= res["best_iter"] < n_iter
    assert set(res["timings"]) == {"active_sampling", "gp_train", "variational_fit", "finalize", "boost"}
    assert all(p.L is not None for g in h["gp"] for p in g.posteriors)  # host records: a kept GP can be installed again
    # the history holds snapshots: every kept GP, posterior, state and logger is its iteration's and its own object
    for i, s in enumerate(run.seen):
        g, state, log = h["gp"][i], h["optim_state"][i], h["function_logger"][i]
        assert g.X.shape[0] == g.y.shape[0] == s["n_flag"] == g.posteriors[0].L.shape[0], i
        assert state["iter"] == i and state["N"] == s["Xn"] + 1 == log.Xn + 1 and log.func_count == s["func_count"], i
        assert h["vp"][i].K == s["K"] and h["vp"][i].parameter_transformer is d.parameter_transformer, i
    for key in ("gp", "vp", "optim_state", "function_logger"):
        assert len({id(o) for o in h[key]} | {id(getattr(d, key))}) == n_iter + 1, key
    assert h["optim_state"][0]["lb_search"] is not d.optim_state["lb_search"]


@pytest.fixture(scope="module")
def mvn_run(ctx):
    return Run(cases.mvn(2, max_fun_evals=BUDGET), SEED, ctx)


@pytest.fixture(scope="module")
def half_normal_run(ctx):
    return Run(cases.half_normal(2, max_fun_evals=BUDGET), SEED, ctx)


def test_unbounded_normal(mvn_run):
    check_run(mvn_run, BUDGET)
    assert mvn_run.results["problem_type"] == "unconstrained"
    err_mean, err_lnZ = cases.errors(mvn_run.case, mvn_run.vp, mvn_run.results)
    print("mvn D=2: err_mean %.4f err_lnZ %.4f" % (err_mean, err_lnZ))
    assert err_mean < 0.5
    assert err_lnZ < 0.5


def test_half_normal_with_bounds(half_normal_run):
    """Finite bounds: the bounded transform, the Jacobian term in the logger and the bounded search box."""
    run = half_normal_run
    check_run(run, BUDGET)
    assert np.all(run.driver.parameter_transformer.type != 0) and np.all(np.isinf(run.driver.optim_state["lb_tran"]))
    log = run.driver.function_logger
    X = log.X_orig[: log.Xn + 1]
    assert np.all((X > run.case.lb) & (X < run.case.ub))
    assert np.all(log.y[: log.Xn + 1] != log.y_orig[: log.Xn + 1])  # the Jacobian term
    err_mean, err_lnZ = cases.errors(run.case, run.vp, run.results)
    print("half-normal D=2: err_mean %.4f err_lnZ %.4f" % (err_mean, err_lnZ))
    assert err_mean < 0.5
    assert err_lnZ < 0.5


def test_noisy_target(ctx):
    """Reported noise SD 0.3 (uncertainty handling level 2) with the default acquisition of that case, VIQR: the
    importance-sampling calls run, the GP is retrained and the posterior refitted after every point.  Structure and
    finiteness only.  ``ns_gp_max`` and ``gp_train_n_init`` are cut (see profiles/vbmc_driver.md): the run fits the GP about
    thirty times."""
    budget = 40
    run = Run(cases.noisy(0.3, max_fun_evals=budget, ns_gp_max=20, gp_train_n_init=128), SEED, ctx)
    check_run(run, budget)
    d = run.driver
    assert d.optim_state["uncertainty_handling_level"] == 2 and d.options["search_acq_fcn"] == ["AcqFcnVIQR()"]
    assert "active_importance_sampling" in d.optim_state
    log = d.function_logger
    assert np.allclose(log.S[: log.Xn + 1], 0.3) and d.gp.s2 is not None
    assert np.all(np.isfinite(run.vp.moments(rng="philox", seed=3)))


def test_same_seed_same_run(mvn_run, ctx):
    again = Run(cases.mvn(2, max_fun_evals=BUDGET), SEED, ctx)
    a, b = mvn_run.driver, again.driver
    assert np.array_equal(a.function_logger.X_orig, b.function_logger.X_orig, equal_nan=True)
    assert a.iteration_history["elbo"] == b.iteration_history["elbo"]
    assert mvn_run.results["elbo"] == again.results["elbo"]


def test_warmup_end_trims_and_switches(ctx, monkeypatch):
    """``stop_warmup_thresh`` / ``tol_stable_warmup`` set so that warm-up ends at iteration 3 of a 40-evaluation run
    (the ELCBO test passes at once, ``stop_warmup_reliability`` takes any solution); ``warmup_keep_threshold`` 3 so that
    the trim removes points of this shallow target; the iteration after skips active sampling as its option says."""
    budget = 40
    over = dict(max_fun_evals=budget, stop_warmup_thresh=1e3, tol_stable_warmup=10, stop_warmup_reliability=1e9,
                warmup_keep_threshold=3, skip_active_sampling_after_warmup=True)
    from pyvbmc_amd import gp as gp_mod

    reupdates, reupdate = [], gp_mod.reupdate

    def spy(function_logger, gp, **kw):  # (without noise the loop appends point by point: the only call is the trim's)
        out = reupdate(function_logger, gp, **kw)
        reupdates.append((int(function_logger.func_count), int(out.X.shape[0]), out))
        return out

    monkeypatch.setattr(gp_mod, "reupdate", spy)
    run = Run(cases.mvn(2, **over), SEED, ctx)
    d, h, seen = run.driver, run.driver.iteration_history, run.seen
    warm = h["warmup"]
    end = warm.index(False)
    assert end == 3 and all(warm[:end]) and not any(warm[end:]) and d.optim_state["last_warmup"] == end
    assert "end warm-up" in h["logging_action"][end]
    before, after = seen[end], seen[end + 1]
    assert before["warmup"] and not after["warmup"]
    assert after["n_flag"] < before["n_flag"] and after["n_flag"] >= 3                   # X_flag shrank (D + 1 kept at least)
    assert h["gp"][end].X.shape[0] == before["n_flag"]           # the kept GP of that iteration still has the untrimmed set
    assert len(reupdates) == 1 and reupdates[0][:2] == (before["func_count"], after["n_flag"])  # the driver's GP: trimmed
    assert reupdates[0][2] is not h["gp"][end]
    assert after["gp_N"] == after["n_flag"]                       # ... and the next one trained on it
    assert after["func_count"] == before["func_count"] and after["Xn"] == before["Xn"]    # active sampling skipped
    assert seen[end + 2]["func_count"] == before["func_count"] + 5
    assert not before["optimize_weights"] and after["optimize_weights"]
    assert d.function_logger.func_count == budget
    assert all(s["K_agrees"] and s["one_transformer"] for s in seen)
