"""The host side of the VBMC driver -- ``ParameterTransformer``, ``Options``, ``FunctionLogger``, ``driver_rules`` and the
``VBMC`` constructor -- against the reference's recorded results (tests/golden/vbmc_driver.npz, written by
tools/make_vbmc_driver_golden.py) and the test suite's own host statements.  No device.

Bounds.
  Transformer values against ``transform_host.RefShapedTransformer`` on the same fields: both state the same formulas, so
  4 ulp of the result's scale (the largest magnitude in the compared array, at least 1).  Constructor fields against the
  reference's: ``type`` exactly, ``mu`` and ``delta`` 1e-15 relative.
  ``FunctionLogger`` against ``active_sample_host.PlainLogger``: the arrays bit for bit.
  ``driver_rules``: flags, indices, masks, message classes exactly; floats 1e-12 relative (the same NumPy calls on both
  sides, ``np.polyfit`` included).
  ``optim_state`` numerics: 1e-14 relative.
"""
import numpy as np
import pytest
from active_sample_host import PlainLogger
from conftest import load_golden
from transform_host import RefShapedTransformer

from pyvbmc_amd import VBMC, FunctionLogger, Options, ParameterTransformer, _lib
from pyvbmc_amd import driver_rules as rules
from pyvbmc_amd import transformer as xf
from pyvbmc_amd.options import DEFAULTS

G = load_golden("vbmc_driver")
INIT = [str(s) for s in G["init_cases"]]
RAISING = [str(s) for s in G["raising_cases"]]
TRACES = [str(s) for s in G["traces"]]
EPS = np.finfo(np.float64).eps
OFF = {"warp_rotoscaling": False, "display": "off"}


def opt(a):
    return None if a.size == 0 else a.copy()


def init_args(name, prefix="init"):
    return [opt(G[f"{prefix}_{name}{'_in' if prefix == 'init' else ''}_{k}"]) for k in ("x0", "lb", "ub", "plb", "pub")]


def never(x):
    raise AssertionError("the target must not be called")


def close(a, b, rel):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore"):  # (inf - inf where both are the same infinity)
        assert np.all(same | (np.abs(a - b) <= rel * np.abs(b))), (a, b)


# ---------------------------------------------------------------------------------------------------- transformer
def build_pt(name):
    x0, lb, ub, plb, pub = init_args(name)
    vb = VBMC(never, x0, lb, ub, plb, pub, dict(OFF, bounded_transform=str(G[f"init_{name}_transform"])))
    return vb.parameter_transformer, vb


@pytest.mark.parametrize("name", INIT)
def test_transformer_fields_are_the_references(name):
    pt, _ = build_pt(name)
    p = f"init_{name}_pt_"
    assert np.array_equal(pt.type, G[p + "type"])
    assert np.array_equal(np.ravel(pt.lb_orig), np.ravel(G[p + "lb_orig"]))
    assert np.array_equal(np.ravel(pt.ub_orig), np.ravel(G[p + "ub_orig"]))
    close(pt.mu, G[p + "mu"], 1e-15)
    close(pt.delta, G[p + "delta"], 1e-15)
    assert pt.R_mat is None and pt.scale is None
    assert xf.candidate(pt) and xf.transformer_fields(pt, pt.type.size) is not None  # the device routes accept it


def ulp4(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    fin = np.isfinite(b)
    assert np.array_equal(a[~fin], b[~fin], equal_nan=True)
    scale = max(1.0, float(np.max(np.abs(b[fin]), initial=0.0)))
    assert np.all(np.abs(a[fin] - b[fin]) <= 4 * EPS * scale), np.max(np.abs(a[fin] - b[fin])) / (EPS * scale)


@pytest.mark.parametrize("name", INIT)
@pytest.mark.parametrize("whiten", [False, True])
def test_transformer_values(name, whiten):
    pt, _ = build_pt(name)
    D = pt.type.size
    r = np.random.default_rng(11)
    if whiten:
        R, _ = np.linalg.qr(r.standard_normal((D, D)))
        pt = ParameterTransformer(D, pt.lb_orig, pt.ub_orig, scale=0.5 + r.random(D), rotation_matrix=R)
        pt.mu, pt.delta = 0.1 * r.standard_normal(D), 0.5 + r.random(D)
    ref = RefShapedTransformer(pt.type, pt.lb_orig, pt.ub_orig, pt.mu, pt.delta, pt.R_mat, pt.scale)
    u = np.concatenate([2.5 * r.standard_normal((40, D)), 30.0 * r.standard_normal((6, D)), np.zeros((1, D))])
    x = ref.inverse(u)
    b = pt.type != 0
    if not whiten:
        x[-1, b] = np.ravel(pt.lb_orig)[b]  # a point on the bound itself: -inf
    ulp4(pt(x), ref(x))
    ulp4(pt.inverse(u), ref.inverse(u))
    ulp4(pt.log_abs_det_jacobian(u), ref.log_abs_det_jacobian(u))
    # 1-D input: a row back, a scalar Jacobian
    assert pt(x[0]).shape == (D,) and pt.inverse(u[0]).shape == (D,) and np.ndim(pt.log_abs_det_jacobian(u[0])) == 0
    ulp4(pt.inverse(u[0]), ref.inverse(u[0]))


def test_transformer_eq_and_errors():
    a = ParameterTransformer(2, np.array([[-1.0, -np.inf]]), np.array([[1.0, np.inf]]), np.array([[-0.5, -1.0]]),
                             np.array([[0.5, 1.0]]), transform_type="probit")
    b = ParameterTransformer(2, np.array([[-1.0, -np.inf]]), np.array([[1.0, np.inf]]), np.array([[-0.5, -1.0]]),
                             np.array([[0.5, 1.0]]), transform_type=12)
    c = ParameterTransformer(2, np.array([[-1.0, -np.inf]]), np.array([[1.0, np.inf]]), np.array([[-0.5, -1.0]]),
                             np.array([[0.5, 2.0]]), transform_type="probit")
    assert a == b and a is not b and not (a == c) and a != c
    assert np.array_equal(a.type, [12.0, 0.0])
    assert np.array_equal(ParameterTransformer(3).type, np.zeros(3))
    with pytest.raises(ValueError):
        ParameterTransformer(1, np.array([[0.0]]), np.array([[1.0]]), transform_type="cauchy")
    with pytest.raises(ValueError):
        ParameterTransformer(1, np.array([[0.0]]), np.array([[1.0]]), np.array([[0.6]]), np.array([[0.4]]))


# -------------------------------------------------------------------------------------------------------- options
@pytest.mark.parametrize("D", [int(d) for d in G["option_Ds"]])
def test_options_defaults_are_the_references(D):
    o = Options(D)
    p = f"opt_d{D}_"
    assert sorted(o) == [str(n) for n in G[p + "names"]] and len(DEFAULTS) == len(G[p + "names"])
    for n, v, is_bool in zip(G[p + "numeric_names"], G[p + "numeric"], G[p + "numeric_is_bool"]):
        mine = o[str(n)]
        assert not callable(mine) and np.ndim(mine) == 0 and float(mine) == v, (n, mine, v)
        assert isinstance(mine, (bool, np.bool_)) == bool(is_bool), n
    for n, v in zip(G[p + "string_names"], G[p + "strings"]):
        assert o[str(n)] == str(v), n
    Ks = [int(k) for k in G["option_Ks"]]
    for n, row in zip(G[p + "k_names"], G[p + "k_values"]):
        assert callable(o[str(n)])
        assert [float(o.eval(str(n), {"K": K})) for K in Ks] == list(row), n
    for n, row in zip(G[p + "n_names"], G[p + "n_values"]):
        assert [float(o.eval(str(n), {"N": K})) for K in Ks] == list(row), n
    for n in G[p + "other_names"]:
        v = o[str(n)]
        assert v is None or callable(v) or isinstance(v, list), n
    assert o["search_acq_fcn"] == ["AcqFcnLog()"] and o["annealed_gp_mean"](5, 10) == 0
    assert all(o[k] == [] for k in ("f_vals", "integer_vars", "noise_size", "ns_ent_fast_boost", "ns_ent_fine_boost",
                                    "output_fcn", "true_cov", "true_mean", "uncertainty_handling", "warmup_options"))


def test_options_user_values_and_errors():
    with pytest.raises(ValueError, match="does not exist"):
        Options(2, {"max_fun_eval": 10})
    o = Options(3, {"max_fun_evals": 77, "ns_ent": 64})
    assert o["max_fun_evals"] == 77 and o.eval("ns_ent", {"K": 9}) == 64 and o.eval("ns_elbo", {"K": 3}) == 150
    with pytest.raises(AttributeError):
        o["max_fun_evals"] = 5
    o.__setitem__("max_fun_evals", 5, force=True)
    assert o["max_fun_evals"] == 5 and isinstance(o, dict) and o.get("nope") is None
    n = Options(2, {"specify_target_noise": True})  # options.py:68-80 of the reference
    assert n["max_fun_evals"] == 300 and n["tol_stable_count"] == 90 and n["search_acq_fcn"] == ["AcqFcnVIQR()"]
    assert n["active_sample_gp_update"] and n["active_sample_vp_update"]
    assert Options(2, {"specify_target_noise": True, "max_fun_evals": 40})["max_fun_evals"] == 40
    w = o.with_overrides(tol_weight=0)
    assert w["tol_weight"] == 0 and o["tol_weight"] == 1e-2 and w.eval("ns_elbo", {"K": 2}) == 100


# --------------------------------------------------------------------------------------------------------- logger
def quad(x):
    return float(-0.5 * np.sum(np.asarray(x) ** 2) - 0.1 * np.sum(np.asarray(x) ** 4))


def noisy(x):
    return quad(x) + 0.3 * float(np.sin(5 * x[0])), 0.2 + 0.1 * abs(float(x[-1]))


LOGGER_ARRAYS = ("X_orig", "y_orig", "X", "y", "n_evals", "X_flag")


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("name", ["d2_both_logit", "d4_mixed", "d1_none"])
def test_function_logger_against_plain_logger(name, noise):
    pt, _ = build_pt(name)
    D = pt.type.size
    fun, level = (noisy, 2) if noise else (quad, 0)
    mine = FunctionLogger(fun, D, noise, level, cache_size=6, parameter_transformer=pt)
    ref = PlainLogger(fun, D, noise, level, cache_size=6, parameter_transformer=pt)
    r = np.random.default_rng(5)
    pts = 0.7 * r.standard_normal((14, D))
    script = [("call", i) for i in range(5)] + [("add", 5), ("call", 2), ("call", 2), ("add", 1)] + \
             [("call", i) for i in range(6, 14)] + [("call", 9), ("add", 13)]  # (grows twice; repeats; adds)
    for step, (what, i) in enumerate(script):
        x = pts[i] if step % 2 else pts[i].reshape(1, -1)
        if what == "call":
            a, b = mine(x), ref(x)
        else:
            a, b = mine.add(x, -1.5 - i, 0.4), ref.add(x, -1.5 - i, 0.4)
        assert np.array_equal(np.ravel(a[0]), np.ravel(b[0])) and a[1] == b[1] and a[2] == b[2]
        for k in LOGGER_ARRAYS + (("S",) if noise else ()):
            assert np.array_equal(getattr(mine, k), getattr(ref, k), equal_nan=True), (step, k)
        assert (mine.Xn, mine.func_count, mine.cache_count, mine.y_max) == (ref.Xn, ref.func_count, ref.cache_count, ref.y_max)
    assert mine.func_count == 16 and mine.cache_count == 3 and mine.Xn == 13 and mine.X.shape[0] == 14
    assert mine.n_evals[2] == 3 and mine.noise_flag == noise and mine.uncertainty_handling_level == level
    assert mine.fun_eval_time.shape == mine.y.shape and np.all(np.isfinite(mine.fun_eval_time[[0, 2, 6]]))
    assert mine.total_fun_eval_time > 0


def test_function_logger_errors():
    pt = ParameterTransformer(2)
    for bad in (lambda x: np.nan, lambda x: np.inf, lambda x: [1.0, 2.0], lambda x: 1j):
        log = FunctionLogger(bad, 2, False, 0, parameter_transformer=pt)
        with pytest.raises(ValueError, match="InvalidFuncValue"):
            log(np.zeros(2))
        assert log.func_count == 0 and log.Xn == -1
    log = FunctionLogger(lambda x: (1.0, -0.5), 2, True, 2, parameter_transformer=pt)
    with pytest.raises(ValueError, match="InvalidNoiseValue"):
        log(np.zeros(2))
    with pytest.raises(ValueError, match="InvalidFuncValue"):
        log.add(np.zeros(2), np.inf)
    with pytest.raises(ValueError, match="one-dimensional"):
        log(np.zeros((2, 2)))
    with pytest.raises(ValueError, match="FuncError"):  # (an array of several values fails in ``.item()``, as there)
        FunctionLogger(lambda x: np.array([1.0, 2.0]), 2, False, 0, parameter_transformer=pt)(np.zeros(2))
    assert FunctionLogger(lambda x: np.array([2.5]), 2, False, 0, parameter_transformer=pt)(np.zeros(2))[0] == 2.5

    def boom(x):
        raise KeyError("inside")

    with pytest.raises(KeyError) as e:
        FunctionLogger(boom, 2, False, 0, parameter_transformer=pt)(np.zeros(2))
    assert "FunctionLogger:FuncError" in e.value.args[-1]


# --------------------------------------------------------------------------------------------------- driver rules
def trace_options(name):
    user = {str(k): (bool(v) if str(k) == "entropy_switch" else int(v)) for k, v in
            zip(G[f"trace_{name}_option_names"], G[f"trace_{name}_option_values"])}
    return Options(2, dict(OFF, **user))


@pytest.mark.parametrize("name", TRACES)
def test_decisions_on_recorded_trace(name):
    """The loop's decisions, iteration by iteration, in the order ``VBMC.optimize`` takes them."""
    p = f"trace_{name}_"
    T = int(G[p + "T"])
    o = trace_options(name)
    elbo, elbo_sd, sKL, lcb, sn2, y = (G[p + k] for k in ("elbo", "elbo_sd", "sKL", "lcb_max", "sn2_hpd", "y_orig"))
    n_max = y.size
    ref_flags = np.unpackbits(G[p + "X_flag"], axis=1)[:, :n_max].astype(bool)
    y_orig = np.full((max(500, n_max), 1), np.nan)
    X_flag = np.full((max(500, n_max),), False)
    warmup, last_warmup, trims = True, np.inf, []
    skip, recompute = False, True  # (optim_state's entries; the variational fit of every iteration resets the second)
    entropy_switch = bool(o["entropy_switch"]) and 2 >= o["det_entropy_min_d"]
    r_hist, stable_hist, fc_hist = [], [], []
    msg_class = {"": 0, rules.MSG_MAX_FUN_EVALS: 1, rules.MSG_MAX_ITER: 2, rules.MSG_STABLE: 3}
    message = ""
    for it in range(T):
        fc = 10 + 5 * it
        new = slice(0 if it == 0 else fc - 5, fc)
        y_orig[new, 0] = y[new]
        X_flag[new] = True
        fc_hist.append(fc)
        t = rules.termination(it, fc, elbo[: it + 1], elbo_sd[: it + 1], sKL[: it + 1], fc_hist, r_hist, sn2[it],
                              entropy_switch, -np.inf, o)
        entropy_switch = t.entropy_switch
        r_hist.append(t.r_index)
        stable_hist.append(t.stable)
        message = t.message or message
        actions = list(t.actions)
        close(t.r_index, G[p + "r_index"][it], 1e-12)
        close(t.elcbo_impro, G[p + "elcbo_impro"][it], 1e-12)
        assert t.stable == G[p + "stable"][it] and t.finished == G[p + "finished"][it], it
        assert msg_class[t.message] == G[p + "msg"][it] and entropy_switch == G[p + "entropy_switch"][it], it
        alarm = False
        if warmup and it > 0:
            alarm = rules.warmup_should_end(it, elbo[: it + 1], elbo_sd[: it + 1], lcb[: it + 1], fc_hist, fc, trims, fc, o)
            if alarm:
                before = X_flag
                a = rules.after_warmup(it, t.r_index, trims, fc, y_orig, fc - 1, X_flag, 2, warmup, last_warmup, o)
                warmup, last_warmup, trims, X_flag = a.warmup, a.last_warmup, a.data_trim_list, a.X_flag
                skip, recompute = a.skip_active_sampling, a.recompute_var_post
                actions += a.actions
                assert np.array_equal(a.X_flag, a.keep & before) and np.sum(a.keep) >= 3
        assert alarm == G[p + "alarm"][it] and warmup == G[p + "warmup"][it] and len(trims) == G[p + "n_trims"][it], it
        assert recompute == G[p + "recompute"][it] and skip == G[p + "skip"][it], it
        assert last_warmup == G[p + "last_warmup"][it]
        assert np.array_equal(X_flag[:n_max], ref_flags[it]), it
        assert "|".join(actions) == str(G[p + "actions"][it]), it
        recompute = False
        for flag, key in ((False, "best"), (True, "best_rank")):
            assert rules.best_iteration(stable_hist, elbo[: it + 1], elbo_sd[: it + 1], r_hist, it, 5, 0.25, flag) == \
                G[p + key][it], (it, key)
    assert np.array_equal(np.asarray(trims, dtype=np.float64), G[p + "data_trim_list"])
    assert t.finished == G[p + "finished"][-1] and rules.best_iteration(stable_hist, elbo, elbo_sd, r_hist) == G[p + "best"][-1]


def test_traces_take_every_path():
    """What the golden file is there for: every listed path occurs in some trace (recorded from the reference)."""
    def col(k):
        return {n: G[f"trace_{n}_{k}"] for n in TRACES}

    alarm, warm, msg, fin, st, sw, trims = (col(k) for k in ("alarm", "warmup", "msg", "finished", "stable",
                                                             "entropy_switch", "n_trims"))
    assert len(TRACES) >= 6 and all(30 <= int(G[f"trace_{n}_T"]) <= 45 for n in TRACES)
    assert any(alarm[n][i] and warm[n][i] for n in TRACES for i in range(len(alarm[n])))      # a false alarm that trims
    assert any(alarm[n][i] and not warm[n][i] and trims[n][i] == 0 for n in TRACES for i in range(len(alarm[n])))
    assert any(alarm[n][i] and not warm[n][i] and trims[n][i] == 1 for n in TRACES for i in range(len(alarm[n])))
    assert {int(msg[n][-1]) for n in TRACES if fin[n][-1]} == {1, 2, 3}
    assert any(np.any((msg[n] > 0) & ~fin[n]) for n in TRACES)                                # a vetoed finish
    assert any(sw[n][0] and not sw[n][-1] for n in TRACES)                                    # the entropy switch flips
    assert any(st[n][-1] for n in TRACES) and any(not np.any(st[n]) for n in TRACES)
    assert any(np.any(st[n]) and not st[n][-1] for n in TRACES)
    assert any(np.any(G[f"trace_{n}_best"] != G[f"trace_{n}_best_rank"]) for n in TRACES)


def test_final_boost_plan_running_moments_update_K():
    o = Options(2, OFF)
    plan = rules.final_boost_plan(3, o)
    assert plan.do_boost and plan.K_new == 50 and plan.n_slow_opts == 1 and plan.n_fast_opts == 250
    assert plan.overrides["tol_weight"] == 0 and plan.overrides["max_iter_stochastic"] == np.inf
    assert plan.overrides["ns_ent"] == 200 * 50 ** (2 / 3) and plan.overrides["ns_ent_fine"] == 2**12 * 50
    same = Options(2, dict(OFF, min_final_components=2, ns_ent_boost=[]))
    assert not rules.final_boost_plan(4, same).do_boost and rules.final_boost_plan(4, same).K_new == 4
    m, c, n = rules.running_moments([], [], np.nan, np.array([[1.0, 2.0]]), np.eye(2), 10, 0.9)
    assert np.array_equal(m, [[1.0, 2.0]]) and np.array_equal(c, np.eye(2)) and n == 10
    m2, c2, n2 = rules.running_moments(m, c, n, np.array([3.0, 4.0]), 2 * np.eye(2), 15, 0.9)
    assert np.array_equal(m2, [[3.0, 4.0]]) and np.array_equal(c2, 2 * np.eye(2)) and n2 == 15  # (the reference's test)
    # update_K (variational_optimization.py:19-87)
    h = {"elbo": [-9.0, -5.0, -3.0, -2.5, -2.0], "elbo_sd": [0.5, 0.3, 0.1, 0.1, 0.1], "warmup": [True, True, False, False, False],
         "pruned": [0, 0, 0, 0, 0], "r_index": [np.inf, np.inf, 5.0, 2.0, 0.5]}
    s = {"vp_K": 2, "n_eff": 35, "warmup": True, "iter": 5, "recompute_var_post": False}
    assert rules.update_K(s, h, o) == 2
    s["warmup"] = False
    assert rules.update_K(s, h, o) == 5  # improving: +1, stable and nothing pruned: +adaptive_k
    s["recompute_var_post"] = True
    assert rules.update_K(s, h, o) == 3
    h["pruned"][-1] = 1
    assert rules.update_K(s, h, o) == 2
    h["pruned"][-1], s["n_eff"], s["recompute_var_post"] = 0, 5, False
    assert rules.update_K(s, h, o) == 3  # ceil(5 ** (2 / 3)) caps it


def test_kl_div_mvn_at_one_dimension():
    """sKL at D = 1: ``np.cov`` gives a 0-D variance, which the reference's ``kl_div_mvn`` lifts to a matrix."""
    from pyvbmc_amd.variational_posterior import kl_div_mvn

    kls = kl_div_mvn(np.array([[0.5]]), np.array(2.0), np.array([[1.0]]), np.array(0.5))
    want = [0.5 * (2.0 / 0.5 + 0.25 / 0.5 - 1 + np.log(0.5 / 2.0)), 0.5 * (0.5 / 2.0 + 0.25 / 2.0 - 1 - np.log(0.5 / 2.0))]
    assert np.allclose(kls, want, rtol=1e-14)
    assert np.array_equal(kls, kl_div_mvn(np.array([[0.5]]), np.array([[2.0]]), np.array([[1.0]]), np.array([[0.5]])))


# ---------------------------------------------------------------------------------------------------- constructor
@pytest.mark.parametrize("name", INIT)
def test_constructor_optim_state(name):
    np.random.seed(int(G["init_seed"]))
    pt, vb = build_pt(name)
    p = f"init_{name}_"
    s = vb.optim_state
    assert len(s) == int(G[p + "n_os_keys"])
    for k in (str(k) for k in G[p + "os_keys"]):
        mine = s["cache"][k[7:]] if k.startswith("cache__") else s[k]
        close(np.asarray(mine, dtype=np.float64), G[p + "os_" + k], 1e-14)
    close(vb.x0, G[p + "x0_tran"], 1e-14)
    assert vb.vp.K == int(G[p + "vp_K"]) == s["vp_K"]
    close(vb.vp.mu, G[p + "vp_mu"], 1e-14)  # (the perturbation drawn from NumPy's stream as the reference draws it)
    assert np.array_equal(vb.vp.sigma, G[p + "vp_sigma"]) and np.array_equal(vb.vp.lambd, G[p + "vp_lambd"])
    assert vb.vp.parameter_transformer is vb.parameter_transformer is vb.function_logger.parameter_transformer
    assert vb.function_logger.func_count == 0 and vb.iteration == -1 and vb.vp.optimize_weights


@pytest.mark.parametrize("name", RAISING)
def test_constructor_raises_the_references_errors(name):
    x0, lb, ub, plb, pub = init_args(name, "raise")
    with pytest.raises(ValueError):
        VBMC(never, x0, lb, ub, plb, pub, OFF)


def test_constructor_misc():
    with pytest.raises(ValueError, match="UnknownDims"):
        VBMC(never, None, None, None, None, None, OFF)
    vb = VBMC(never, None, None, None, np.array([[-1.0, -2.0]]), np.array([[1.0, 2.0]]), OFF)
    assert np.array_equal(vb.optim_state["cache"]["x_orig"], [[0.0, 0.0]])  # the centre of the plausible box
    with pytest.raises(ValueError, match="does not exist"):
        VBMC(never, np.zeros((1, 2)), None, None, -np.ones((1, 2)), np.ones((1, 2)), {"no_such_option": 1})
    with pytest.raises(ValueError, match="MismatchedStartingInputs"):
        VBMC(never, np.zeros((1, 2)), None, None, -np.ones((1, 2)), np.ones((1, 2)), dict(OFF, f_vals=[1.0, 2.0]))
    with pytest.raises(ValueError, match="UnknownGPmean"):
        VBMC(never, np.zeros((1, 2)), None, None, -np.ones((1, 2)), np.ones((1, 2)), dict(OFF, gp_mean_fun="linear"))
    n = VBMC(lambda x: (never(x), 1.0), np.zeros((1, 2)), None, None, -np.ones((1, 2)), np.ones((1, 2)),
             dict(OFF, specify_target_noise=True), log_prior=never)
    assert n.optim_state["uncertainty_handling_level"] == 2 and n.optim_state["gp_noise_fun"] == [1, 1, 0]
    assert n.function_logger.noise_flag and n.log_likelihood is not None
    a = VBMC(never, np.zeros((1, 2)), None, None, -np.ones((1, 2)), np.ones((1, 2)), OFF, seed=3)
    b = VBMC(never, np.zeros((1, 2)), None, None, -np.ones((1, 2)), np.ones((1, 2)), OFF, seed=3)
    assert np.array_equal(a.vp.mu, b.vp.mu)


def test_seeded_constructor_leaves_the_callers_stream_alone():
    np.random.seed(5)
    want = np.random.get_state()[1].copy(), np.random.rand(3)
    np.random.seed(5)
    VBMC(never, np.zeros((1, 2)), None, None, -np.ones((1, 2)), np.ones((1, 2)), OFF, seed=3)
    assert np.array_equal(np.random.get_state()[1], want[0]) and np.array_equal(np.random.rand(3), want[1])


def test_history_snapshots_are_their_own():
    from pyvbmc_amd.vbmc import _copy_logger, _copy_state

    vb = VBMC(quad, np.zeros((1, 2)), None, None, -np.ones((1, 2)), np.ones((1, 2)), OFF)
    vb.function_logger(np.array([0.1, 0.2]))
    state, log = _copy_state(vb.optim_state), _copy_logger(vb.function_logger)
    vb.optim_state["lb_search"][0, 0] = -99.0
    vb.optim_state["data_trim_list"].append(7)
    vb.optim_state["cache"]["x_orig"][0, 0] = 5.0
    vb.optim_state["iter"] = 3
    vb.function_logger(np.array([0.3, 0.4]))
    vb.function_logger.X_flag[0] = False
    assert state["lb_search"][0, 0] != -99.0 and state["data_trim_list"] == [] and state["cache"]["x_orig"][0, 0] == 0.0
    assert state["iter"] == -1 and set(state) == set(vb.optim_state)
    assert log.Xn == 0 and log.func_count == 1 and log.X_flag[0] and np.isnan(log.X[1, 0])
    assert log.fun is vb.function_logger.fun and log.parameter_transformer is vb.parameter_transformer


REFUSED = {
    "D>32": (40, {}),
    "uncertainty_handling_level 1": (2, {"uncertainty_handling": [1]}),
    "warp_rotoscaling (the reference's default)": (2, {"warp_rotoscaling": True}),
    "warp_nonlinear": (2, {"warp_nonlinear": True}),
    "separate_search_gp": (2, {"separate_search_gp": True}),
    "stochastic_optimizer": (2, {"stochastic_optimizer": "sgd"}),
    "gp_hyp_sampler": (2, {"gp_hyp_sampler": "mala"}),
    "gp_mean_fun": (2, {"gp_mean_fun": "negquadse"}),
    "noise_shaping": (2, {"noise_shaping": True}),
    "search_optimizer": (2, {"search_optimizer": "Nelder-Mead"}),
    "acquisition": (2, {"search_acq_fcn": ["AcqFcnThompson()"]}),
    "min_final_components": (2, {"min_final_components": 200}),
    "variable_means off": (2, {"variable_means": False}),
    "ns_ent_fast": (2, {"ns_ent_fast": 100}),
    "ns_ent_fast as a function of K": (2, {"ns_ent_fast": lambda K: 10 * K}),
    "ns_ent_fast_active": (2, {"ns_ent_fast_active": 50}),
    "ns_ent_fast_boost": (2, {"ns_ent_fast_boost": 50}),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refusals_come_before_the_first_target_call(what):
    D, user = REFUSED[what]
    calls = [0]

    def target(x):
        calls[0] += 1
        return 0.0

    options = dict(OFF, **user) if "warp_rotoscaling" not in user else dict(display="off", **user)
    with pytest.raises(_lib.UnsupportedShape):
        VBMC(target, np.zeros((1, D)), None, None, -np.ones((1, D)), np.ones((1, D)), options)
    assert calls[0] == 0
    if what.startswith("warp_rotoscaling"):  # ON in the reference's defaults: no options at all is refused as well
        with pytest.raises(_lib.UnsupportedShape, match="warp_rotoscaling"):
            VBMC(target, np.zeros((1, D)), None, None, -np.ones((1, D)), np.ones((1, D)))
        assert calls[0] == 0
