"""Helpers of the active-sampling loop's tests (pyvbmc_amd/active_sample.py).  TEST INFRASTRUCTURE.

* ``target_exact`` / ``target_noisy``  the targets of tests/golden/active_sample.npz as NumPy formulas (original space)
* ``PlainLogger``    a duck of the reference's ``FunctionLogger`` (function_logger.py:36-421): the call, ``add``, the
                     arrays, the log-Jacobian term and the running mean of repeated points
* ``load_case``      a case of the golden file (tools/make_active_sample_golden.py) as fresh arguments of the driver
* ``numpy_search``   the ``_search`` hook: tests/search_host.py's restatement of the search with the oracle acquisition
* ``host_rebuild``   the posterior of the logger's data at the GP's samples, by oracle/gp_ref.py
"""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import search_host as sh  # noqa: E402
from oracle import acq_ref, gp_ref, mixture_ref  # noqa: E402
from transform_host import RefShapedTransformer  # noqa: E402

TRAJECTORIES = ("a", "b", "c")
DESIGNS = ("i1", "i2", "i3")
NUMERIC_OPTIONS = ("ns_search", "cache_frac", "search_cache_frac", "heavy_tail_search_frac", "mvn_search_frac",
                   "hpd_search_frac", "box_search_frac", "hpd_frac")
DEFAULT_OPTIONS = dict(
    display="off", active_sample_vp_update=False, active_sample_gp_update=False, active_sample_full_update_past_warmup=2,
    active_sample_full_update_threshold=3, acq_hedge=False, ns_search=256, cache_frac=0.5, search_cache_frac=0.0,
    heavy_tail_search_frac=0.25, mvn_search_frac=0.25, hpd_search_frac=0.0, box_search_frac=0.25, hpd_frac=0.8,
    search_optimizer="none", search_cmaes_vp_init=True, search_max_fun_evals=200, noise_shaping=False, active_search_bound=2,
    init_design="plausible", update_random_alpha=False)
ACQ_OF = {"a": "AcqFcnLog", "b": "AcqFcnNoisy", "c": "AcqFcnLog"}
DESIGN_OF = {"i1": "plausible", "i2": "narrow", "i3": "plausible"}
_SCALES = np.array([1.0, 0.5, 2.0, 0.8, 1.3, 0.6, 1.7, 0.9])


def target_exact(x):
    """A smooth anisotropic quadratic-plus-quartic log density."""
    x = np.ravel(x)
    a = np.resize(_SCALES, x.size)
    return float(-0.5 * np.sum(a * x**2) - 0.05 * np.sum(x**4))


def target_noisy(x):
    """The same with a deterministic wobble standing in for the noise draw, and the noise SD the user reports for it
    (uncertainty handling level 2): ``S = 0.3 + 0.1 |x_0|``."""
    x = np.ravel(x)
    return target_exact(x) + 0.3 * float(np.sin(7.0 * x[0] + 3.0 * x[-1])), 0.3 + 0.1 * abs(float(x[0]))


class PlainLogger:
    """The reference's FunctionLogger as far as ``active_sample`` uses it."""

    def __init__(self, fun, D, noise_flag, uncertainty_handling_level, cache_size=500, parameter_transformer=None):
        self.fun, self.D, self.noise_flag = fun, D, noise_flag
        self.uncertainty_handling_level = uncertainty_handling_level
        self.parameter_transformer = parameter_transformer
        self.func_count = self.cache_count = 0
        self.X_orig = np.full([cache_size, D], np.nan)
        self.y_orig = np.full([cache_size, 1], np.nan)
        self.X = np.full([cache_size, D], np.nan)
        self.y = np.full([cache_size, 1], np.nan)
        self.n_evals = np.full([cache_size, 1], 0)
        if noise_flag:
            self.S = np.full([cache_size, 1], np.nan)
        self.Xn = -1
        self.X_flag = np.full((cache_size,), False, dtype=bool)
        self.y_max = float("-Inf")

    def _orig(self, x):
        x = np.asarray(x, dtype=np.float64)
        x = x.squeeze() if x.ndim > 1 else x
        x = np.atleast_1d(x)
        return x, self.parameter_transformer.inverse(np.reshape(x, (1, x.shape[0])))[0]

    def __call__(self, x):
        x, x_orig = self._orig(x)
        if self.noise_flag and self.uncertainty_handling_level == 2:
            f_val_orig, f_sd = self.fun(x_orig)
        else:
            f_val_orig, f_sd = self.fun(x_orig), (1 if self.noise_flag else None)
        self.func_count += 1
        f_val, idx = self._record(x_orig, x, f_val_orig, f_sd)
        return f_val, f_sd, idx

    def add(self, x, f_val_orig, f_sd=None):
        x, x_orig = self._orig(x)
        f_sd = (1 if f_sd is None else f_sd) if self.noise_flag else None
        self.cache_count += 1
        f_val, idx = self._record(x_orig, x, f_val_orig, f_sd)
        return f_val, f_sd, idx

    def _grow(self):
        n = int(np.max((np.ceil(self.Xn / 2), 1)))
        for name, fill in (("X_orig", np.nan), ("y_orig", np.nan), ("X", np.nan), ("y", np.nan), ("n_evals", 0)) + (
                (("S", np.nan),) if self.noise_flag else ()):
            a = getattr(self, name)
            setattr(self, name, np.append(a, np.full([n, a.shape[1]], fill), axis=0))
        self.X_flag = np.append(self.X_flag, np.full((n,), False, dtype=bool))

    def _record(self, x_orig, x, f_val_orig, f_sd):
        pt = self.parameter_transformer
        dup = (self.X == x).all(axis=1)
        if np.any(dup):
            idx = np.argwhere(dup)[0, 0]
            N = self.n_evals[idx]
            if f_sd is not None:
                tau_n, tau_1 = 1 / self.S[idx] ** 2, 1 / f_sd**2
                self.y_orig[idx] = (tau_n * self.y_orig[idx] + tau_1 * f_val_orig) / (tau_n + tau_1)
                self.S[idx] = 1 / np.sqrt(tau_n + tau_1)
            else:
                self.y_orig[idx] = (N * self.y_orig[idx] + f_val_orig) / (N + 1)
            f_val = self.y_orig[idx]  # (a view: as there, the Jacobian term lands in y_orig as well, function_logger.py:388-391)
            f_val += pt.log_abs_det_jacobian(x)
            self.y[idx] = f_val
            self.n_evals[idx] += 1
            return f_val, idx
        self.Xn += 1
        if self.Xn > self.X_orig.shape[0] - 1:
            self._grow()
        self.X_orig[self.Xn], self.X[self.Xn], self.y_orig[self.Xn] = x_orig, x, f_val_orig
        f_val = f_val_orig + pt.log_abs_det_jacobian(np.reshape(x, (1, x.shape[0])))[0]
        self.y[self.Xn] = f_val
        if f_sd is not None:
            self.S[self.Xn] = f_sd
        self.X_flag[self.Xn] = True
        self.n_evals[self.Xn] += 1
        self.y_max = np.nanmax(self.y[self.X_flag])
        return f_val, self.Xn


def make_logger(c, X0=None):
    """A fresh PlainLogger of case ``c`` with the training points ``X0`` (transformed space) evaluated."""
    noisy = bool(c.noisy)
    log = PlainLogger(target_noisy if noisy else target_exact, c.D, noisy, 2 if noisy else 0, cache_size=c.cache_size,
                      parameter_transformer=c.pt)
    for x in (c.X0 if X0 is None else X0):
        log(x)
    log.func_count = 0
    return log


def load_case(g, name):
    """Case ``name`` of tests/golden/active_sample.npz: the inputs as arrays, builders of fresh arguments, and the
    reference's recorded results (``ref_*``)."""
    def a(k):
        return np.array(g[f"{name}_{k}"])

    c = SimpleNamespace(name=name, D=int(a("D")), K=int(a("K")), noisy=bool(a("noisy")), np_seed=int(a("np_seed")),
                        sample_count=int(a("sample_count")), cache_size=int(a("cache_size")))
    c.pt = RefShapedTransformer.from_golden(g, f"{name}_pt")
    c.X0, c.hyp = a("X0"), a("hyp")
    for k in ("mu", "sigma", "lambd", "w", "cache_x_orig", "cache_y_orig", "search_cache", "lb_search", "ub_search",
              "lb_tran", "ub_tran", "plb_tran", "pub_tran", "lb_eps_orig", "ub_eps_orig", "options"):
        setattr(c, k, a(k))
    c.ref = SimpleNamespace(**{k[len(name) + 5:]: np.array(v) for k, v in g.items() if k.startswith(f"{name}_ref_")})
    return c


def synthetic_case(D, noisy=False, K=2, N=24, S=2, seed=0, sample_count=3):
    """A case of the golden file's kind at another dimension (nothing recorded): logit dimensions on (-10, 10), the same
    targets, N training points, S hyper-parameter samples."""
    r = np.random.default_rng(3000 + 10 * D + seed)
    c = SimpleNamespace(name=f"syn{D}", D=D, K=K, noisy=noisy, np_seed=17, sample_count=sample_count, cache_size=N + 16)
    c.pt = RefShapedTransformer(np.full(D, 3.0), np.full(D, -10.0), np.full(D, 10.0), np.zeros(D), np.ones(D))
    c.mu, c.sigma, c.w = 0.3 * r.standard_normal((D, K)), np.array([[0.3, 0.5]]), np.array([[0.4, 0.6]])
    lam = 0.5 + r.random((D, 1))
    c.lambd = lam / np.sqrt(np.sum(lam**2) / D)
    c.X0 = 0.35 * r.standard_normal((N, D))
    c.hyp = np.array([np.concatenate([np.log(0.4 + 0.2 * r.random(D)), [np.log(4.0)], [np.log(0.05 * (s + 1))], [0.0],
                                      np.zeros(D), np.log(np.full(D, 0.4))]) for s in range(S)])
    c.cache_x_orig, c.cache_y_orig, c.search_cache = np.zeros((0, D)), np.zeros(0), np.zeros((0, D))
    one = np.ones((1, D))
    c.lb_search, c.ub_search, c.lb_tran, c.ub_tran = -1.25 * one, 1.25 * one, -np.inf * one, np.inf * one
    c.plb_tran, c.pub_tran = -0.5 * one, 0.5 * one
    c.lb_eps_orig, c.ub_eps_orig = (-10 + 2e-5) * one, (10 - 2e-5) * one
    c.options = np.array([float(DEFAULT_OPTIONS[k]) for k in NUMERIC_OPTIONS])
    c.ref = None
    return c


def make_optim_state(c):
    return {"cache": {"x_orig": c.cache_x_orig.copy(), "y_orig": c.cache_y_orig.copy()}, "search_cache": c.search_cache.copy(),
            "lb_search": c.lb_search.copy(), "ub_search": c.ub_search.copy(), "lb_tran": c.lb_tran.copy(),
            "ub_tran": c.ub_tran.copy(), "plb_tran": c.plb_tran.copy(), "pub_tran": c.pub_tran.copy(),
            "lb_eps_orig": c.lb_eps_orig.copy(), "ub_eps_orig": c.ub_eps_orig.copy(), "integer_vars": None,
            "variance_regularized_acq_fcn": True, "tol_gp_var": 1e-4, "iter": 5, "last_warmup": 0, "hyp_dict": None,
            "recompute_var_post": True, "entropy_alpha": 0.0}


def make_options(c, **over):
    o = dict(DEFAULT_OPTIONS)
    o.update({k: (int(v) if k == "ns_search" else float(v)) for k, v in zip(NUMERIC_OPTIONS, c.options)})
    if c.name in ACQ_OF:
        o["search_acq_fcn"] = [ACQ_OF[c.name] + "()"]
    if c.name in DESIGN_OF:
        o["init_design"] = DESIGN_OF[c.name]
    o.update(over)
    return o


def iteration_history():
    return {"r_index": [1.0]}


def make_vp(c, ctx=None):
    from pyvbmc_amd import VariationalPosterior

    vp = VariationalPosterior(c.D, c.K, parameter_transformer=c.pt)
    vp.mu, vp.sigma, vp.lambd, vp.w = c.mu.copy(), c.sigma.reshape(1, -1).copy(), c.lambd.reshape(-1, 1).copy(), c.w.reshape(1, -1).copy()
    vp.eta = np.log(vp.w)
    if ctx is not None:
        vp.ctx = ctx
    return vp


def training_s2(log):
    return (log.S[log.X_flag] ** 2).reshape(-1, 1) if log.noise_flag else None


def make_gp(c, log, ctx=None, device=False, fetch=True):
    """This package's GP on the logger's data at the case's hyper-parameter samples (host records, or device-built)."""
    from pyvbmc_amd import gp as gpm

    gp = gpm.GP(c.D, gpm.SquaredExponential(), gpm.NegativeQuadratic(),
                gpm.GaussianNoise(constant_add=True, user_provided_add=bool(c.noisy)))
    if ctx is not None:
        gp.ctx = ctx
    gp.update(log.X[log.X_flag].copy(), log.y[log.X_flag].copy(), training_s2(log), c.hyp, device=device, fetch=fetch)
    return gp


def oracle_gp(c, log):
    s2 = training_s2(log)
    return gp_ref.make_gp(log.X[log.X_flag], log.y[log.X_flag], c.hyp, gp_ref.MEAN_NEGQUAD, s2=s2, noise_user=s2 is not None)


def make_plain_gp(c, log):
    """A gpyreg-shaped duck (tests/helpers.py PlainGP): records and data, no noise or covariance object."""
    from helpers import PlainGP

    gp = PlainGP(oracle_gp(c, log))
    if gp.s2 is not None:
        gp.s2 = np.array(gp.s2, dtype=np.float64).reshape(-1, 1)
    return gp


host_rebuild = oracle_gp

_KIND = {"AcqFcn": acq_ref.STD, "AcqFcnLog": acq_ref.LOG, "AcqFcnVanilla": acq_ref.VANILLA, "AcqFcnNoisy": acq_ref.NOISY}


def numpy_search(acq_fcn, gp, vp, function_logger, optim_state, options, *, number_of_points=None, rng=None, seed=None,
                 ctx=None):
    """``active_search.search`` restated in NumPy on NumPy's global stream: tests/search_host.py's points, rounding,
    oracle acquisition with the hard-bound mask, and ranking."""
    mix = mixture_ref.Mixture.make(vp.mu, np.ravel(vp.sigma), np.ravel(vp.lambd), np.ravel(vp.w))
    n = options["ns_search"] if number_of_points is None else number_of_points
    X, idx_cache = sh.points_numpy(n, optim_state, function_logger, mix, options)
    X = sh.real2int(X, function_logger.parameter_transformer, optim_state.get("integer_vars"))
    s2 = getattr(gp, "s2", None)
    ogp = gp_ref.GPData(gp.D, gp.X, gp.y, s2, gp_ref.MEAN_NEGQUAD, list(gp.posteriors), s2 is not None)
    acq = sh.acq_values(_KIND[type(acq_fcn).__name__], X, ogp, mix, function_logger.y_max, optim_state,
                        vp.parameter_transformer, X_rescaled=gp.temporary_data.get("X_rescaled"),
                        sn2_new=gp.temporary_data.get("sn2_new"))
    return sh.rank(X, idx_cache, acq, optim_state, options)
