"""CPU tests of the active-sampling loop (pyvbmc_amd/active_sample.py) against the reference's recorded runs
(tests/golden/active_sample.npz, tools/make_active_sample_golden.py) and of its routing (pyvbmc_amd/dropin.py
``patch_active_sample_loop``).  No GPU: the search is the NumPy restatement (tests/active_sample_host.py
``numpy_search``), the GP updates run on the host.

The recorded trajectories have a relative gap of at least 1e-6 between the best and the second-best acquisition value at
every step (asserted when the file is generated; measured >= 0.1), so the restated acquisition, which agrees with the
reference's to rounding, picks the same rows: the acquired X are compared exactly, everything derived from them to 1e-12.
"""
import copy
import sys
import types
from types import SimpleNamespace

import numpy as np
import pytest

import active_sample_host as ash

TOL = 1e-12


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b))))


@pytest.fixture(scope="module")
def g(golden):
    return golden("active_sample")


@pytest.mark.parametrize("name", ["a", "b"])
def test_plain_logger_replays_the_recorded_values(g, name):
    c = ash.load_case(g, name)
    log = ash.make_logger(c)
    assert close(log.y[log.X_flag], c.ref.y0)
    if c.noisy:
        assert close(log.S[log.X_flag], c.ref.S0)
    for x in c.ref.X:
        log(x)
    n = c.X0.shape[0]
    assert close(log.y[n : log.Xn + 1], c.ref.y) and close(log.X_orig[n : log.Xn + 1], c.ref.X_orig)
    assert log.func_count == len(c.ref.X) and log.y_max == np.max(log.y[log.X_flag])


def run_host(c, **kw):
    from pyvbmc_amd import active_sample

    log = ash.make_logger(c)
    gp = ash.make_gp(c, log)
    vp = ash.make_vp(c)
    st = ash.make_optim_state(c)
    options = ash.make_options(c)
    np.random.seed(c.np_seed)
    out = active_sample(gp, c.sample_count, st, log, ash.iteration_history(), vp, options, rng="numpy", device=False,
                        _search=ash.numpy_search, **kw)
    return out, np.random.rand()


def check_trajectory(c, log, st, next_rand, x_tol=0.0):
    n = c.X0.shape[0]
    X = log.X[n : log.Xn + 1]
    assert X.shape == c.ref.X.shape
    if x_tol:
        assert np.max(np.abs(X - c.ref.X)) <= x_tol
    else:
        assert np.array_equal(X, c.ref.X)
    assert close(log.y[n : log.Xn + 1], c.ref.y)
    if c.noisy:
        assert close(log.S[n : log.Xn + 1], c.ref.S)
    assert close(st["lb_search"], c.ref.lb_search) and close(st["ub_search"], c.ref.ub_search)
    assert st["N"] == int(c.ref.N) and np.ravel(st["N_eff"])[0] == int(c.ref.N_eff)
    assert close(st["cache"]["x_orig"], c.ref.cache_x_orig)
    assert np.array_equal(np.isnan(st["cache"]["y_orig"]), np.isnan(c.ref.cache_y_orig))
    assert close(np.nan_to_num(st["cache"]["y_orig"]), np.nan_to_num(c.ref.cache_y_orig))
    # (the recorded count includes the training points' evaluations; make_logger starts counting after them)
    assert log.func_count == int(c.ref.func_count) - n and log.cache_count == int(c.ref.cache_count)
    assert next_rand == float(c.ref.next_rand)  # the stream was consumed call for call


@pytest.mark.parametrize("name", ash.TRAJECTORIES)
def test_trajectory_equals_the_reference(g, name):
    c = ash.load_case(g, name)
    (log, st, vp, gp), next_rand = run_host(c)
    check_trajectory(c, log, st, next_rand)
    if name == "c":
        assert int(c.ref.cache_count) >= 1  # a point came from the cache with its known value
    # the GP followed: every point but the last went in at the present samples (c acquires its cache point again, through
    # the search cache, as the reference does: a repeated point is averaged, not appended)
    n = gp.X.shape[0]
    assert n == (c.X0.shape[0] + c.sample_count - 1 if name != "c" else int(c.ref.N))
    assert np.array_equal(gp.X, log.X[:n]) and (name == "c" or np.array_equal(gp.y, log.y[:n]))
    ogp = ash.gp_ref.make_gp(gp.X, gp.y, c.hyp, ash.gp_ref.MEAN_NEGQUAD, s2=gp.s2, noise_user=gp.s2 is not None)
    for p, q in zip(gp.posteriors, ogp.posteriors):
        assert np.max(np.abs(p.alpha - q.alpha)) <= 1e-9 * np.max(np.abs(q.alpha))
    assert (gp.s2 is not None) == c.noisy and (not c.noisy or close(gp.s2, log.S[:n] ** 2))


@pytest.mark.parametrize("name", ash.DESIGNS)
def test_initial_design_equals_the_reference(g, name):
    from pyvbmc_amd import active_sample

    c = ash.load_case(g, name)
    log = ash.make_logger(c, X0=np.zeros((0, c.D)))
    st, vp = ash.make_optim_state(c), ash.make_vp(c)
    np.random.seed(c.np_seed)
    out = active_sample(None, c.sample_count, st, log, ash.iteration_history(), vp, ash.make_options(c))
    assert out[0] is log and out[1] is st and out[3] is None
    n = c.sample_count
    assert log.Xn + 1 == n
    assert close(log.X[:n], c.ref.X) and close(log.y[:n], c.ref.y) and close(log.X_orig[:n], c.ref.X_orig)
    assert log.func_count == int(c.ref.func_count) and log.cache_count == int(c.ref.cache_count)
    assert close(st["cache"]["x_orig"], c.ref.cache_x_orig) and st["cache"]["y_orig"].shape == c.ref.cache_y_orig.shape
    assert np.random.rand() == float(c.ref.next_rand)


def test_unknown_initial_design_raises(g):
    from pyvbmc_amd import active_sample

    c = ash.load_case(g, "i1")
    log = ash.make_logger(c, X0=np.zeros((0, c.D)))
    with pytest.raises(ValueError, match="Unknown initial design"):
        active_sample(None, c.sample_count, ash.make_optim_state(c), log, ash.iteration_history(), ash.make_vp(c),
                      ash.make_options(c, init_design="grid"))


# ------------------------------------------------------------------------------------------------ the full update
class StubVP:
    """A posterior that records nothing but its parameters and its ELBO."""

    def __init__(self, theta, elbo, like):
        self.theta, self.stats = np.asarray(theta, dtype=np.float64), {"elbo": elbo}
        for k in ("D", "K", "mu", "sigma", "lambd", "w", "parameter_transformer"):  # what the search reads
            setattr(self, k, getattr(like, k))

    def get_parameters(self):
        return self.theta.copy()


def full_update_run(g, monkeypatch, elbo0, elbo_new):
    from pyvbmc_amd import active_sample

    c = ash.load_case(g, "a")
    log = ash.make_logger(c)
    gp = ash.make_gp(c, log)
    real_vp = ash.make_vp(c)
    st = ash.make_optim_state(c)
    st.update(hyp_dict={"run_cov": "before"}, recompute_var_post=True, entropy_alpha=0.25)
    options = ash.make_options(c, active_sample_vp_update=True, active_sample_gp_update=True,
                               active_sample_full_update_past_warmup=10, gp_tol_opt=1e-5, gp_tol_opt_mcmc=1e-2,
                               gp_tol_opt_active=1e-4, gp_tol_opt_mcmc_active=1e-1, tol_weight=1e-2, ns_ent=lambda K: 100 * K,
                               ns_ent_fast=lambda K: 0, ns_ent_fine=lambda K: 1024 * K, ns_ent_active=lambda K: 20 * K,
                               ns_ent_fast_active=lambda K: 0, ns_ent_fine_active=lambda K: 200 * K, ns_elbo=lambda K: 50 * K,
                               ns_elbo_incr=0.1, update_random_alpha=True)
    before = dict(options)
    calls = SimpleNamespace(train=[], vp=[], elcbo=[])

    def train_gp(hyp_dict, optim_state, function_logger, iteration_history, opts, plb_tran, pub_tran):
        calls.train.append((hyp_dict, opts["gp_tol_opt"], opts["gp_tol_opt_mcmc"], opts["tol_weight"], opts["ns_ent"](2),
                            opts["ns_ent_fast"](2), opts["ns_ent_fine"](2), plb_tran is optim_state["plb_tran"]))
        optim_state["recompute_var_post"] = False  # (what the real one may leave behind)
        new = ash.make_gp(c, function_logger)
        return new, None, 0.5, {"run_cov": f"trained {len(calls.train)}"}

    def optimize_vp(opts, optim_state, vp, gp_, fast_opts_N, slow_opts_N=2):
        calls.vp.append((opts["tol_weight"], fast_opts_N, slow_opts_N, gp_.X.shape[0], optim_state["entropy_alpha"]))
        return StubVP([len(calls.vp), 2.0], elbo_new, vp), None, None

    def neg_elcbo(theta, gp_, vp0, beta, ns, compute_grad, compute_var):
        calls.elcbo.append((theta.copy(), vp0, beta, ns, compute_grad, compute_var))
        return (-elbo0, None, 0.0, 0.0, 0.0)

    monkeypatch.setattr(sys.modules["pyvbmc_amd.active_sample"], "_neg_elcbo", neg_elcbo)
    vp_in = StubVP([0.0, 0.0], 0.0, real_vp)
    np.random.seed(c.np_seed)
    out = active_sample(gp, c.sample_count, st, log, ash.iteration_history(), vp_in, options, rng="numpy", device=False,
                        _search=ash.numpy_search, train_gp=train_gp, optimize_vp=optimize_vp)
    return c, out, calls, options, before, vp_in


def test_full_update_calls_and_restores(g, monkeypatch):
    c, (log, st, vp, gp), calls, options, before, vp_in = full_update_run(g, monkeypatch, elbo0=-5.0, elbo_new=-1.0)
    assert len(calls.train) == c.sample_count - 1 and len(calls.vp) == c.sample_count - 1
    # the callables saw the overridden values; the first training call gets the caller's hyp_dict, later ones what was returned
    assert calls.train[0] == ({"run_cov": "before"}, 1e-4, 1e-1, 0, 40, 0, 400, True)
    assert calls.train[1][0] == {"run_cov": "before"}
    for i, (tol_weight, n_fast, n_slow, n_gp, alpha) in enumerate(calls.vp):
        assert (tol_weight, n_fast, n_slow) == (0, 10, 1) and n_gp == c.X0.shape[0] + i + 1 and 0.0 <= alpha <= 1.0
    assert set(options) == set(before) and all(options[k] is before[k] for k in before)  # the caller's options: untouched
    assert st["recompute_var_post"] is True and st["entropy_alpha"] == 0.25 and st["hyp_dict"] == {"run_cov": "before"}
    assert st["sn2_hpd"] == 0.5 and len(st["vp_repo"]) == 1
    assert gp.X.shape[0] == c.X0.shape[0] + c.sample_count - 1
    # the comparison with the posterior of before: its parameters, no gradient, the variance, ceil(200 K / K) draws
    (theta0, vp0, beta, ns, compute_grad, compute_var), = calls.elcbo
    assert np.array_equal(theta0, [0.0, 0.0]) and vp0 is not vp_in and (beta, ns, compute_grad, compute_var) == (0.0, 200, False, True)
    assert vp is not vp0 and np.array_equal(vp.theta, [c.sample_count - 1, 2.0])  # elbo0 = -5 < -1: the new one stays


def test_full_update_returns_the_old_posterior_when_it_is_better(g, monkeypatch):
    c, (log, st, vp, gp), calls, options, before, vp_in = full_update_run(g, monkeypatch, elbo0=3.0, elbo_new=-1.0)
    assert vp is calls.elcbo[0][1] and np.array_equal(vp.theta, [0.0, 0.0]) and vp is not vp_in  # vp0, the deep copy


def test_full_update_without_callables_needs_the_reference(g, monkeypatch):
    from pyvbmc_amd import active_sample

    monkeypatch.setitem(sys.modules, "pyvbmc", None)  # (importing it then raises ImportError)
    c = ash.load_case(g, "a")
    log = ash.make_logger(c)
    options = ash.make_options(c, active_sample_gp_update=True, active_sample_full_update_past_warmup=10)
    vp = ash.make_vp(c)
    state = np.random.get_state()[1].copy()
    with pytest.raises(ImportError, match="train_gp"):
        active_sample(ash.make_gp(c, log), c.sample_count, ash.make_optim_state(c), log, ash.iteration_history(), vp,
                      options, rng="numpy", device=False, _search=ash.numpy_search)
    assert log.func_count == 0 and np.array_equal(np.random.get_state()[1], state)


# ------------------------------------------------------------------------------------- refusals before side effects
class ForeignAcq:
    acq_info = {}


def refused(c, gp, options, st=None, **kw):
    from pyvbmc_amd import _lib, active_sample

    log = ash.make_logger(c)
    st = ash.make_optim_state(c) if st is None else st
    st0, vp = copy.deepcopy(st), ash.make_vp(c)
    np.random.seed(5)
    state = np.random.get_state()[1].copy()
    with pytest.raises(_lib.UnsupportedShape):
        active_sample(gp, c.sample_count, st, log, ash.iteration_history(), vp, options, **kw)
    assert log.func_count == 0 and log.cache_count == 0 and log.Xn + 1 == c.X0.shape[0]
    assert np.array_equal(np.random.get_state()[1], state)
    assert set(st) == set(st0) and all(np.array_equal(st[k], st0[k]) for k in st0 if k != "cache")


def test_refusals_come_before_side_effects(g):
    c = ash.load_case(g, "a")
    log = ash.make_logger(c)
    wide = SimpleNamespace(D=33, X=np.zeros((4, 33)), y=np.zeros((4, 1)), posteriors=[], temporary_data={})
    refused(c, wide, ash.make_options(c))
    refused(c, wide, ash.make_options(c), rng="philox", seed=3)
    gp = ash.make_gp(c, log)
    refused(c, gp, ash.make_options(c, search_acq_fcn=[ForeignAcq()]))
    refused(c, gp, ash.make_options(c, search_acq_fcn=["AcqFcnLog()", "NoSuchAcq()"]))
    refused(c, gp, ash.make_options(c, search_optimizer="Nelder-Mead"))
    refused(c, gp, ash.make_options(c, search_optimizer="bads"), device=False, _search=ash.numpy_search)


def test_as_package_acq():
    from pyvbmc_amd import _lib, acquisition as acq

    assert isinstance(acq.as_package_acq("AcqFcnNoisy()"), acq.AcqFcnNoisy)
    own = acq.AcqFcnLog()
    assert acq.as_package_acq(own) is own
    foreign = type("AcqFcnVIQR", (), {"acq_info": {"quantile": 0.9}})()
    mapped = acq.as_package_acq(foreign)
    assert isinstance(mapped, acq.AcqFcnVIQR) and mapped.acq_info["quantile"] == 0.9
    assert isinstance(acq.as_package_acq(type("AcqFcnVanilla", (), {})()), acq.AcqFcnVanilla)
    for bad in (ForeignAcq(), "NoSuchAcq()", acq.AbstractAcqFcn()):
        with pytest.raises(_lib.UnsupportedShape):
            acq.as_package_acq(bad)


# ------------------------------------------------------------------------------------------------------- routing
def test_patch_active_sample_loop_on_a_stand_in_module(monkeypatch):
    import pyvbmc_amd
    from pyvbmc_amd import _lib, dropin

    seen = []

    def reference(gp, sample_count, optim_state, function_logger, iteration_history, vp, options):
        seen.append(("reference", sample_count))
        return "reference"

    def driver(gp, sample_count, optim_state, function_logger, iteration_history, vp, options, **kw):
        seen.append(("driver", sample_count, kw))
        if sample_count == 33:
            raise _lib.UnsupportedShape("refused")
        if sample_count == 34:
            raise _lib.NoDeviceError(_lib.E_NODEV, "no device")
        return "driver"

    monkeypatch.setattr(sys.modules["pyvbmc_amd.active_sample"], "active_sample", driver)
    timer, train, opt = object(), object(), object()
    mod = types.ModuleType("vbmc_stand_in")
    mod.active_sample, mod.timer, mod.train_gp, mod.optimize_vp = reference, timer, train, opt
    assert pyvbmc_amd.patch_active_sample_loop(mod, rng="philox", seed=7, n_starts=3) is mod
    first = mod.active_sample
    assert first is not reference
    assert mod.active_sample(None, 2, {}, None, None, None, {}) == "driver"
    assert seen[-1] == ("driver", 2, dict(rng="philox", seed=7, n_starts=3, timer=timer, train_gp=train, optimize_vp=opt))
    assert mod.active_sample(None, 33, {}, None, None, None, {}) == "reference" and seen[-1] == ("reference", 33)
    assert mod.active_sample(None, 34, {}, None, None, None, {}) == "reference" and seen[-1] == ("reference", 34)
    dropin.patch_active_sample_loop(mod)  # idempotent: the reference behind it is still the reference's
    assert mod.active_sample(None, 33, {}, None, None, None, {}) == "reference"
    assert seen[-2][2] == dict(timer=timer, train_gp=train, optimize_vp=opt)
    assert pyvbmc_amd.unpatch_active_sample_loop(mod) is mod and mod.active_sample is reference
    assert dropin.unpatch_active_sample_loop(mod).active_sample is reference
    with pytest.raises(TypeError):
        dropin.patch_active_sample_loop(mod, fetch=True)
    assert mod.active_sample is reference


# ---------------------------------------------------------------------------------- the GP update's host route
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("duck", ["package", "plain"])
def test_append_point_and_reupdate_on_the_host(g, name, duck):
    """``append_point`` / ``reupdate`` without a device, for this package's GP and for a duck that has neither a noise
    object nor a ``_posterior``: the records are the oracle's on the extended data."""
    from pyvbmc_amd import append_point, reupdate

    c = ash.load_case(g, name)
    log = ash.make_logger(c)
    gp = ash.make_gp(c, log) if duck == "package" else ash.make_plain_gp(c, log)
    n = c.X0.shape[0]

    def check(rows):
        assert gp.X.shape == (rows, c.D) and gp.y.shape == (rows, 1) and (gp.s2 is None) == (not c.noisy)
        assert np.array_equal(gp.X, log.X[:rows]) and np.array_equal(np.ravel(gp.y), np.ravel(log.y[:rows]))
        ogp = ash.gp_ref.make_gp(gp.X, gp.y, c.hyp, ash.gp_ref.MEAN_NEGQUAD, s2=gp.s2, noise_user=gp.s2 is not None)
        for p, q in zip(gp.posteriors, ogp.posteriors):
            assert np.max(np.abs(np.ravel(p.alpha) - np.ravel(q.alpha))) <= 1e-9 * np.max(np.abs(q.alpha))
            assert np.max(np.abs(p.L - q.L)) <= 1e-9 * np.max(np.abs(q.L)) and np.array_equal(p.sW, q.sW)

    y, _, i = log(c.ref.X[0])
    if c.noisy:
        with pytest.raises(ValueError):
            append_point(gp, c.ref.X[0], y, device=False)  # a GP with s2 needs the new point's
        assert gp.X.shape[0] == n
        assert append_point(gp, c.ref.X[0], y, log.S[i] ** 2, device=False) is gp
    else:
        assert append_point(gp, c.ref.X[0], y, device=False) is gp
    check(n + 1)
    log(c.ref.X[1])
    assert reupdate(log, gp, device=False) is gp  # one new row: the append
    check(n + 2)
    log(c.ref.X[2])
    log(c.ref.X[2])  # evaluated twice: the logger averages, the GP takes the logger's data as it stands
    assert reupdate(log, gp, device=False) is gp
    check(n + 3)
