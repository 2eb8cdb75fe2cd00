"""Save, load and checkpoints of the VBMC driver, the parts that need no device (pyvbmc_amd/vbmc.py, options.py,
_persist.py, variational_posterior.py, gp.py): what pickles, the file rules, ``load``'s arguments on a hand-built history,
the posterior's own ``save`` / ``load``, and the records' ``sn2_div``.  The runs themselves: tests/test_vbmc_checkpoint_gpu.py.
"""
import copy
import logging
import os
import pickle
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import vbmc_driver_cases as cases

from pyvbmc_amd import VBMC, Options, VariationalPosterior
from pyvbmc_amd import gp as gp_mod
from pyvbmc_amd.options import DEFAULTS
from pyvbmc_amd.vbmc import HISTORY_KEYS


# ---- module-level targets: what plain pickle takes
def flat_prior(x):
    return -0.5 * float(np.sum(np.square(x))) / 100.0


def noisy_normal(x):
    return cases._scaled_normal(x), 0.3


def my_ns_ent(K):
    return 7 * K


def _equal(a, b):
    """Equality of option / state values: arrays element-wise (NaN equal to NaN), containers item by item."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and (np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b):
        return True
    return type(a) is type(b) and a == b


def _same_options(a, b):
    assert list(a) == list(b)
    for k in a:
        if callable(a[k]):
            assert callable(b[k]), k
            n_args = {"annealed_gp_mean": 2}.get(k, 1)
            for n in (1, 7, 50):
                assert a[k](*([n] * n_args)) == b[k](*([n] * n_args)), k
        else:
            assert _equal(a[k], b[k]), k
    assert (a.D, a.useroptions, a.is_initialized) == (b.D, b.useroptions, b.is_initialized)


# ---- Options
@pytest.mark.parametrize("D", [1, 2, 6])
def test_options_plain_pickle_round_trip(D):
    o = Options(D)
    q = pickle.loads(pickle.dumps(o))
    assert type(q) is Options and set(q) == set(DEFAULTS)
    _same_options(o, q)
    for k, (_, v) in DEFAULTS.items():  # a callable that is the table's own is the table's again
        if callable(v):
            assert q[k] is v, k


def test_options_user_values_survive():
    o = Options(2, {"max_fun_evals": 33, "ns_ent": my_ns_ent, "search_acq_fcn": ["AcqFcnVIQR()"], "specify_target_noise": True})
    q = pickle.loads(pickle.dumps(o))
    _same_options(o, q)
    assert q["ns_ent"] is my_ns_ent and q["max_fun_evals"] == 33 and q.eval("ns_ent", {"K": 3}) == 21
    assert q.useroptions == {"max_fun_evals", "ns_ent", "search_acq_fcn", "specify_target_noise"}
    assert q["tol_stable_count"] == 90  # (the default that follows from specify_target_noise)
    with pytest.raises(AttributeError):
        q["max_iter"] = 3
    r = q.with_overrides(ns_ent=5, tol_weight=0)
    assert r["ns_ent"] == 5 and q["ns_ent"] is my_ns_ent and r["max_fun_evals"] == 33
    _same_options(q, copy.copy(q))
    _same_options(q, copy.deepcopy(q))
    _same_options(r, pickle.loads(pickle.dumps(r)))


def test_options_lambda_needs_dill(monkeypatch):
    monkeypatch.setitem(sys.modules, "dill", None)  # (``import dill`` raises ImportError)
    o = Options(2, {"ns_ent_fine": lambda K: 3 * K})
    with pytest.raises(TypeError, match="ns_ent_fine"):
        pickle.dumps(o)
    assert copy.deepcopy(o)["ns_ent_fine"](2) == 6  # copies never went through pickle


# ---- an unstarted driver
def _driver(kind, **options):
    case = cases.mvn(2, **options)
    if kind == "prior":
        case = case._replace(log_prior=flat_prior)
    elif kind == "noisy":
        case = case._replace(f=noisy_normal, options=dict(case.options, specify_target_noise=True))
    elif kind == "noisy_prior":
        case = case._replace(f=noisy_normal, log_prior=flat_prior, options=dict(case.options, specify_target_noise=True))
    return cases.make(case, 1)


@pytest.mark.parametrize("kind", ["plain", "prior", "noisy", "noisy_prior"])
def test_unstarted_driver_round_trip(kind, tmp_path):
    a = _driver(kind)
    a.save(tmp_path / "vb.pkl")
    b = VBMC.load(tmp_path / "vb.pkl")
    for name in ("lower_bounds", "upper_bounds", "plausible_lower_bounds", "plausible_upper_bounds", "x0"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    _same_options(a.options, b.options)
    assert _equal(a.optim_state, b.optim_state)
    assert b.iteration == -1 and not b.is_finished and b.gp is None and b._ctx is None and b.vp._ctx is None
    assert b.seed == 1 and b.rng == a.rng and b._stage_calls == {1: 0, 2: 0}
    assert b.parameter_transformer is b.vp.parameter_transformer is b.function_logger.parameter_transformer
    assert b.parameter_transformer == a.parameter_transformer
    assert np.array_equal(a.vp.mu, b.vp.mu) and np.array_equal(a.vp.sigma, b.vp.sigma)
    assert set(b.iteration_history) == set(HISTORY_KEYS) and all(v == [] for v in b.iteration_history.values())
    # the target is still there, through the logger
    x = np.array([[0.3, -0.7]])
    ya, yb = a.function_logger(x), b.function_logger(x)
    assert ya[0] == yb[0] and b.function_logger.func_count == 1
    x_orig = b.parameter_transformer.inverse(x)  # (the logger takes points of the transformed space)
    want = cases._scaled_normal(x_orig) + (flat_prior(x_orig) if "prior" in kind else 0.0)
    assert np.isclose(b.function_logger.y_orig[0], want, rtol=1e-14, atol=0)
    if kind.startswith("noisy"):
        assert b.optim_state["uncertainty_handling_level"] == 2 and b.function_logger.S[0] == 0.3


def test_driver_with_lambda_target_needs_dill(monkeypatch, tmp_path):
    monkeypatch.setitem(sys.modules, "dill", None)
    case = cases.mvn(2)
    vb = cases.make(case._replace(f=lambda x: cases._scaled_normal(x)), 1)
    with pytest.raises(TypeError, match="dill"):
        vb.save(tmp_path / "vb")
    assert os.listdir(tmp_path) == []


# ---- file rules
def test_suffix_exists_overwrite(tmp_path):
    a = _driver("plain")
    assert a.save(tmp_path / "run") == tmp_path / "run.pkl" and os.listdir(tmp_path) == ["run.pkl"]
    assert VBMC.load(tmp_path / "run").iteration == -1  # (the suffix is added on load as well)
    a.save(tmp_path / "run.ckpt")
    assert sorted(os.listdir(tmp_path)) == ["run.ckpt", "run.pkl"]
    with pytest.raises(FileExistsError):
        a.save(tmp_path / "run")
    with pytest.raises(FileExistsError):
        a.save(tmp_path / "run.pkl", overwrite=False)
    a.iteration = 5  # (a mark to tell the two files apart)
    a.save(tmp_path / "run", overwrite=True)
    assert pickle.load(open(tmp_path / "run.pkl", "rb")).iteration == 5
    assert sorted(os.listdir(tmp_path)) == ["run.ckpt", "run.pkl"]


def test_save_is_atomic(tmp_path, monkeypatch):
    a = _driver("plain")
    a.save(tmp_path / "run")
    before = open(tmp_path / "run.pkl", "rb").read()

    def dies(obj, f, *args, **kw):
        f.write(b"half a file")
        raise OSError("disk full")

    monkeypatch.setattr(pickle, "dump", dies)
    a.iteration = 5
    with pytest.raises(OSError, match="disk full"):
        a.save(tmp_path / "run", overwrite=True)
    monkeypatch.undo()
    assert os.listdir(tmp_path) == ["run.pkl"]
    assert open(tmp_path / "run.pkl", "rb").read() == before
    assert VBMC.load(tmp_path / "run").iteration == -1


# ---- load's arguments, on a hand-built history of three iterations (no stage runs)
def _with_fake_history(tmp_path, finished=False):
    a = _driver("plain", max_fun_evals=40)
    D = a.D
    noise = gp_mod.GaussianNoise(constant_add=True)
    rng = np.random.default_rng(5)
    for it in range(3):
        N = 10 + 5 * it
        X = rng.standard_normal((N, D))
        for x in X[-(10 if it == 0 else 5):]:
            a.function_logger(x)
        g = gp_mod.GP(D, gp_mod.SquaredExponential(), gp_mod.NegativeQuadratic(), noise)
        g.X, g.y = a.function_logger.X[a.function_logger.X_flag].copy(), a.function_logger.y[a.function_logger.X_flag].reshape(-1, 1).copy()
        hyp = np.concatenate([np.zeros(D), [0.0, -3.0 - it, 0.0], np.zeros(D), np.zeros(D)])
        g.update(hyp=hyp[None, :])
        vp = copy.deepcopy(a.vp, {id(a.parameter_transformer): a.parameter_transformer})
        vp.mu = vp.mu + it
        vp.optimize_weights = False  # (as ``optimize_vp`` leaves a posterior of the warm-up)
        vp.stats = {"elbo": -1.0 - it, "elbo_sd": 0.1, "stable": False, "entropy": 0.0}
        a.optim_state.update(iter=it, N=N, warmup=it < 2, vp_K=vp.K, hyp_dict={"hyp": hyp[None, :].copy(), "run_cov": None})
        a.hyp_dict = a.optim_state["hyp_dict"]
        np.random.seed(100 + it)
        np.random.rand(3)
        from pyvbmc_amd.vbmc import _copy_logger, _copy_state

        for key, value in (("iter", it), ("vp", vp), ("gp", g), ("elbo", -1.0 - it), ("elbo_sd", 0.1), ("sKL", 0.5), ("warmup", it < 2),
                           ("function_logger", _copy_logger(a.function_logger)), ("optim_state", _copy_state(a.optim_state)),
                           ("func_count", N), ("random_state", np.random.get_state()), ("logging_action", ["it %d" % it])):
            a._record(key, value, it)
        for key in HISTORY_KEYS:
            a._record(key, a.iteration_history[key][it] if len(a.iteration_history[key]) > it else None, it)
        a.vp, a.gp, a.iteration = copy.deepcopy(vp, {id(a.parameter_transformer): a.parameter_transformer}), copy.deepcopy(g), it
    a._base_seed, a._stage_calls = 1, {1: 3, 2: 7}
    a.is_finished = finished
    a.save(tmp_path / "run")
    return a


def test_load_new_options(tmp_path):
    _with_fake_history(tmp_path, finished=True)
    b = VBMC.load(tmp_path / "run", new_options={"max_fun_evals": 60})
    assert b.options["max_fun_evals"] == 60 and "max_fun_evals" in b.options.useroptions and b.options.is_initialized
    with pytest.raises(AttributeError):
        b.options["max_fun_evals"] = 70
    with pytest.raises(ValueError, match="does not exist"):
        VBMC.load(tmp_path / "run", new_options={"max_fun_evils": 60})
    from pyvbmc_amd import _lib

    with pytest.raises(_lib.UnsupportedShape):  # what the constructor refuses stays refused
        VBMC.load(tmp_path / "run", new_options={"warp_rotoscaling": True})


@pytest.mark.parametrize("k", [-1, 3, 10])
def test_load_iteration_out_of_range(tmp_path, k):
    _with_fake_history(tmp_path)
    with pytest.raises(ValueError, match="iteration"):
        VBMC.load(tmp_path / "run", iteration=k)


def test_load_live_state(tmp_path):
    a = _with_fake_history(tmp_path)
    b = VBMC.load(tmp_path / "run")
    assert b.iteration == 2 and all(len(b.iteration_history[k]) == 3 for k in HISTORY_KEYS)
    assert b._base_seed == 1 and b._stage_calls == {1: 3, 2: 7} and b._termination_message == ""
    assert b.optim_state["hyp_dict"] is b.hyp_dict  # one dump: what was shared is shared
    assert np.array_equal(b.vp.mu, a.vp.mu) and b.vp is not b.iteration_history["vp"][2]
    assert np.array_equal(b.gp.posteriors[0].L, a.gp.posteriors[0].L) and b.gp._ctx is None
    assert all(v.parameter_transformer is b.parameter_transformer for v in b.iteration_history["vp"])
    assert b._resume["go_on"] and not b._resume["rewind"]
    # the stream state of the save is what the resumed run starts from
    want, got = a._numpy_state, b._resume["numpy_state"]
    assert want[0] == got[0] and np.array_equal(want[1], got[1]) and want[2:] == got[2:]


@pytest.mark.parametrize("k", [0, 1])
def test_load_rewinds_to_an_iteration(tmp_path, k):
    a = _with_fake_history(tmp_path)
    before = np.random.get_state()
    b = VBMC.load(tmp_path / "run", iteration=k)
    h = b.iteration_history
    assert b.iteration == k and set(h) == set(HISTORY_KEYS) and all(len(h[key]) == k + 1 for key in HISTORY_KEYS)
    ha = a.iteration_history
    assert np.array_equal(b.vp.mu, ha["vp"][k].mu) and b.vp.stats["elbo"] == -1.0 - k
    assert np.array_equal(b.gp.X, ha["gp"][k].X) and np.array_equal(b.gp.posteriors[0].alpha, ha["gp"][k].posteriors[0].alpha)
    assert b.function_logger.func_count == ha["function_logger"][k].func_count == 10 + 5 * k
    assert _equal({x: v for x, v in b.optim_state.items() if x != "hyp_dict"},
                  {x: v for x, v in ha["optim_state"][k].items() if x != "hyp_dict"})
    assert b.optim_state["iter"] == k and b.hyp_dict is b.optim_state["hyp_dict"]
    assert np.array_equal(b.hyp_dict["hyp"], ha["optim_state"][k]["hyp_dict"]["hyp"])
    # copies, so that going on does not write into the history; one transformer still
    assert b.vp is not h["vp"][k] and b.gp is not h["gp"][k] and b.function_logger is not h["function_logger"][k]
    assert b.optim_state is not h["optim_state"][k] and b.function_logger.X is not h["function_logger"][k].X
    assert b.vp.parameter_transformer is b.parameter_transformer is b.function_logger.parameter_transformer
    assert b.vp.optimize_mu and not b.vp.optimize_weights  # (state k is in warm-up)
    assert b._resume["rewind"] and b._resume["go_on"]
    assert np.array_equal(b._resume["numpy_state"][1], ha["random_state"][k][1])
    assert np.array_equal(np.random.get_state()[1], before[1])  # without set_random_state the stream is not touched


def test_rewind_past_warmup_sets_the_flags(tmp_path):
    a = _with_fake_history(tmp_path)
    # a fourth iteration, so that iteration 2 (warm-up over in its state) is an earlier one
    for key in HISTORY_KEYS:
        a._record(key, a.iteration_history[key][2], 3)
    a.iteration = 3
    a.save(tmp_path / "run", overwrite=True)
    b = VBMC.load(tmp_path / "run", iteration=2)
    assert not b.optim_state["warmup"]
    assert b.vp.optimize_mu == b.options["variable_means"] and b.vp.optimize_weights == b.options["variable_weights"]
    assert b.vp.optimize_weights and not b.iteration_history["vp"][2].optimize_weights


def test_load_set_random_state(tmp_path):
    a = _with_fake_history(tmp_path)
    state = np.random.get_state()
    try:
        VBMC.load(tmp_path / "run", iteration=1, set_random_state=True)
        got = np.random.rand(4)
        np.random.set_state(a.iteration_history["random_state"][1])
        assert np.array_equal(got, np.random.rand(4))
        VBMC.load(tmp_path / "run", set_random_state=True)
        got = np.random.rand(4)
        np.random.set_state(a.iteration_history["random_state"][2])
        assert np.array_equal(got, np.random.rand(4))
    finally:
        np.random.set_state(state)


# ---- the posterior
def test_vp_save_and_load(tmp_path):
    a = _driver("plain")
    vp = a.vp
    vp.stats = {"elbo": -1.5, "elbo_sd": 0.25, "stable": True}
    vp.optimize_weights = True
    assert vp.save(tmp_path / "vp") is None and os.listdir(tmp_path) == ["vp.pkl"]
    with pytest.raises(FileExistsError):
        vp.save(tmp_path / "vp")
    vp.save(tmp_path / "vp", overwrite=True)
    q = VariationalPosterior.load(tmp_path / "vp")
    assert type(q) is VariationalPosterior and q._ctx is None
    assert _equal(vp.get_parameters(), q.get_parameters())
    for name in ("mu", "sigma", "lambd", "w", "eta"):
        assert np.array_equal(getattr(vp, name), getattr(q, name)), name
    assert (q.D, q.K, q.optimize_mu, q.optimize_sigma, q.optimize_lambd, q.optimize_weights) == (
        vp.D, vp.K, vp.optimize_mu, vp.optimize_sigma, vp.optimize_lambd, True)
    assert q.stats == vp.stats and q.parameter_transformer == vp.parameter_transformer
    a.save(tmp_path / "driver")
    with pytest.raises(TypeError):
        VariationalPosterior.load(tmp_path / "driver")


# ---- records and reinstall
def _small_gp(with_s2):
    rng = np.random.default_rng(3)
    D, N = 2, 12
    X = rng.standard_normal((N, D))
    y = -0.5 * np.sum(X**2, axis=1, keepdims=True) + 0.01 * rng.standard_normal((N, 1))
    g = gp_mod.GP(D, gp_mod.SquaredExponential(), gp_mod.NegativeQuadratic(),
                  gp_mod.GaussianNoise(constant_add=True, user_provided_add=with_s2))
    s2 = 0.01 + 0.02 * rng.random((N, 1)) if with_s2 else None
    hyp = np.concatenate([np.zeros(D), [0.0, -2.0, 0.0], np.zeros(D), np.zeros(D)])
    g.update(X, y, s2, hyp=np.stack([hyp, hyp + 0.1]))
    return g


@pytest.mark.parametrize("with_s2", [False, True])
def test_records_carry_sn2_div(with_s2):
    g = _small_gp(with_s2)
    for p in g.posteriors:
        want = np.exp(2 * p.hyp[3]) + (np.min(g.s2) if with_s2 else 0.0)
        assert p.sn2_div == want and isinstance(p.sn2_div, float)
        assert np.array_equal(p.sW, np.ones(12) / np.sqrt(p.sn2_div))
    scale = [p.sn2_div for p in g.posteriors]
    gp_mod.append_point(g, np.array([0.2, -0.1]), -0.03, 0.5 if with_s2 else None, device=False)
    assert g.X.shape[0] == 13 and [p.sn2_div for p in g.posteriors] == scale
    q = pickle.loads(pickle.dumps(g))
    assert [p.sn2_div for p in q.posteriors] == scale and q._ctx is None
    # records of another maker, without the field, are taken as before
    duck = SimpleNamespace(X=g.X, y=g.y, s2=g.s2, noise=g.noise, mean=g.mean, D=2,
                           posteriors=np.array([SimpleNamespace(**{k: v for k, v in vars(p).items() if k != "sn2_div"})
                                                for p in g.posteriors], dtype=object))
    gp_mod.append_point(duck, np.array([0.4, 0.4]), -0.2, 0.5 if with_s2 else None, device=False)
    assert duck.X.shape[0] == 14


def test_reinstall_without_a_device_falls_back(monkeypatch, caplog):
    from pyvbmc_amd import _lib

    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    g = _small_gp(False)
    alpha = g.posteriors[0].alpha
    with caplog.at_level(logging.WARNING):
        assert gp_mod.reinstall(g) is False
    assert g.posteriors[0].alpha is alpha and g._ctx is None
