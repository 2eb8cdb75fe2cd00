"""Checkpoints of ``VBMC.optimize`` on the device: a run that is stopped and resumed from its checkpoint in a FRESH context
is, bit for bit, the run that was never stopped -- the contract of tests/test_vbmc_driver_gpu.py::test_same_seed_same_run
across a save and a load.  A load that restarted the seed counters or reseeded NumPy's stream would draw other points; one
that did not put the GP back as the device built it would rebuild where the uninterrupted run appends, and round otherwise.

Targets: tests/vbmc_driver_cases.py (module-level functions, which plain pickle takes), seed 1.  Every run is deterministic
by its seed; the uninterrupted runs are module fixtures.
"""
import logging

import numpy as np
import pytest
import vbmc_driver_cases as cases

pytestmark = pytest.mark.gpu

SEED = 1
WARMUP_END = dict(max_fun_evals=40, stop_warmup_thresh=1e3, tol_stable_warmup=10, stop_warmup_reliability=1e9,
                  warmup_keep_threshold=3, skip_active_sampling_after_warmup=True)  # (test_warmup_end_trims_and_switches)


class Stop(Exception):
    pass


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


@pytest.fixture()
def fresh_ctx():
    """The context of the resuming process: nothing installed, nothing cached."""
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def run(case, ctx, **kw):
    d = cases.make(case, SEED, ctx=ctx)
    vp, results = d.optimize(**kw)
    return d, vp, results


def stopped_and_resumed(case, ctx, fresh_ctx, path, stop_at, caplog):
    """The run with a checkpoint, killed in iteration ``stop_at``; then the file, loaded on another context, run to its
    end.  Also required here: the caller's NumPy stream is untouched by either call, nothing about exactness is logged."""
    from pyvbmc_amd import VBMC

    def kill(d):
        if d.iteration == stop_at:
            raise Stop

    first = cases.make(case, SEED, ctx=ctx)
    np.random.seed(4321)
    before = np.random.get_state()
    with pytest.raises(Stop):
        first.optimize(on_iteration=kill, checkpoint=path)
    assert np.array_equal(np.random.get_state()[1], before[1])
    assert [c[0] for c in first.checkpoint_log] == list(range(stop_at))
    with caplog.at_level(logging.WARNING):
        d = VBMC.load(path, ctx=fresh_ctx)
        assert d.iteration == stop_at - 1 and not d.is_finished and d._ctx is fresh_ctx
        seen = []
        vp, results = d.optimize(on_iteration=lambda drv: seen.append((drv.iteration, drv.vp.K == drv.optim_state["vp_K"])))
    assert not [r for r in caplog.records if "bit-exact" in r.getMessage()]
    after = np.random.get_state()
    assert np.array_equal(after[1], before[1]) and after[2:] == before[2:]
    assert [s[0] for s in seen] == list(range(stop_at, d.iteration + 1)) and all(s[1] for s in seen)
    return d, vp, results


def assert_same_run(a, res_a, b, res_b):
    from pyvbmc_amd.vbmc import HISTORY_KEYS

    assert np.array_equal(a.function_logger.X_orig, b.function_logger.X_orig, equal_nan=True)
    for k in ("elbo", "elbo_sd", "sKL"):
        assert a.iteration_history[k] == b.iteration_history[k], k
    for k in ("elbo", "best_iter", "func_count"):
        assert res_a[k] == res_b[k], k
    assert a.iteration == b.iteration and res_a["message"] == res_b["message"]
    for k in HISTORY_KEYS:
        assert len(b.iteration_history[k]) == b.iteration + 1, k
    assert b.iteration_history["iter"] == list(range(b.iteration + 1))
    assert set(res_b["timings"]) == {"active_sampling", "gp_train", "variational_fit", "finalize", "boost"}


@pytest.fixture(scope="module")
def mvn_run(ctx):
    return run(cases.mvn(2, max_fun_evals=60), ctx)


@pytest.fixture(scope="module")
def warmup_end_run(ctx):
    return run(cases.mvn(2, **WARMUP_END), ctx)


@pytest.fixture(scope="module")
def half_normal_run(ctx):
    return run(cases.half_normal(2, max_fun_evals=60), ctx)


@pytest.fixture(scope="module")
def finished_file(ctx, tmp_path_factory):
    """A finished run of budget 40 and its last checkpoint."""
    path = tmp_path_factory.mktemp("ckpt") / "finished.pkl"
    d, vp, results = run(cases.mvn(2, max_fun_evals=40), ctx, checkpoint=path)
    assert d.is_finished and results["func_count"] == 40
    assert [c[0] for c in d.checkpoint_log] == list(range(d.iteration + 1)) + [d.iteration]
    return path, d, results


def test_resume_inside_warmup(mvn_run, ctx, fresh_ctx, tmp_path, caplog):
    a, _, res_a = mvn_run
    b, _, res_b = stopped_and_resumed(cases.mvn(2, max_fun_evals=60), ctx, fresh_ctx, tmp_path / "run.pkl", 3, caplog)
    assert_same_run(a, res_a, b, res_b)


def test_resume_after_the_warmup_trim(warmup_end_run, ctx, fresh_ctx, tmp_path, caplog):
    """Warm-up ends at iteration 3; the stop is in iteration 5: the live GP of the checkpoint (end of iteration 4) was
    trained after an iteration that skipped active sampling on the set ``reupdate`` had trimmed."""
    a, _, res_a = warmup_end_run
    assert a.iteration_history["warmup"].index(False) == 3
    b, _, res_b = stopped_and_resumed(cases.mvn(2, **WARMUP_END), ctx, fresh_ctx, tmp_path / "run.pkl", 5, caplog)
    assert_same_run(a, res_a, b, res_b)
    assert b.iteration_history["warmup"] == a.iteration_history["warmup"]


def test_resume_right_after_the_trim(warmup_end_run, ctx, fresh_ctx, tmp_path, caplog):
    """The stop is in iteration 4, so the checkpoint's live GP is the one ``reupdate`` built at the end of iteration 3."""
    a, _, res_a = warmup_end_run
    b, _, res_b = stopped_and_resumed(cases.mvn(2, **WARMUP_END), ctx, fresh_ctx, tmp_path / "run.pkl", 4, caplog)
    assert_same_run(a, res_a, b, res_b)


def test_resume_bounded_target(half_normal_run, ctx, fresh_ctx, tmp_path, caplog):
    a, _, res_a = half_normal_run
    b, _, res_b = stopped_and_resumed(cases.half_normal(2, max_fun_evals=60), ctx, fresh_ctx, tmp_path / "run.pkl", 2, caplog)
    assert_same_run(a, res_a, b, res_b)


def test_extend_a_finished_run(finished_file, fresh_ctx):
    from pyvbmc_amd import VBMC

    path, first, _ = finished_file
    d = VBMC.load(path, new_options={"max_fun_evals": 60}, ctx=fresh_ctx)
    assert d.is_finished and d.iteration == first.iteration
    vp, results = d.optimize()
    assert results["func_count"] == d.function_logger.func_count == 60
    assert d.iteration > first.iteration and len(d.iteration_history["elbo"]) == d.iteration + 1
    assert d.iteration_history["elbo"][: first.iteration + 1] == first.iteration_history["elbo"]
    err_mean, err_lnZ = cases.errors(cases.mvn(2), vp, results)
    print("extended mvn D=2: err_mean %.4f err_lnZ %.4f" % (err_mean, err_lnZ))
    assert err_mean < 0.5
    assert err_lnZ < 0.5


def test_rewind_and_go_on(finished_file, fresh_ctx):
    from pyvbmc_amd import VBMC
    from pyvbmc_amd.vbmc import HISTORY_KEYS

    path, first, _ = finished_file
    d = VBMC.load(path, iteration=2, ctx=fresh_ctx)
    assert d.iteration == 2 and d.function_logger.func_count == first.iteration_history["func_count"][2]
    seen = []
    vp, results = d.optimize(on_iteration=lambda drv: seen.append(drv.vp.K == drv.optim_state["vp_K"]))
    assert results["func_count"] == 40 and d.is_finished and all(seen) and len(seen) == d.iteration - 2
    h = d.iteration_history
    for k in HISTORY_KEYS:
        assert len(h[k]) == d.iteration + 1, k
    assert h["iter"] == list(range(d.iteration + 1)) and h["elbo"][:3] == first.iteration_history["elbo"][:3]
    assert np.all(np.isfinite(np.array(h["elbo"], dtype=np.float64))) and np.all(np.isfinite(np.array(h["sKL"], dtype=np.float64)))
    assert np.isfinite(results["elbo"]) and vp.K == results["components"]
    assert h["function_logger"][2] is not d.function_logger and h["function_logger"][2].func_count == 20
