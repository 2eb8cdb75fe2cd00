#!/usr/bin/env python
"""Generate tests/golden/active_sample.npz by RUNNING THE REFERENCE's ``active_sample`` (vbmc/active_sample.py:27-644).
TEST INFRASTRUCTURE, like tools/make_search_golden.py: it runs only where the reference checkout is present (that tool's
REF, or the VBMC_REFERENCE environment variable), imports it at run time and stores numbers only.

    python tools/make_active_sample_golden.py        # rewrites tests/golden/active_sample.npz

The reference's loop runs with its own FunctionLogger, ParameterTransformer, VariationalPosterior and acquisition
classes over the gpyreg stand-in (oracle/_stubs/gpyreg).  The stand-in's ``update`` REPLACES the data and needs ``hyp``;
``AppendingGP`` below subclasses it locally to give gpyreg's semantics -- ``update(xnew, ynew)`` appends at the present
samples, ``update()`` with nothing rebuilds from ``gp.X, gp.y, gp.s2`` -- and takes ``pyvbmc_amd.gp.GaussianNoise`` as
its noise object, because the stand-in's has no ``compute``.

Shape: D = 3, K = 2, N = 24, S = 2, negative-quadratic mean, ns_search = 256, search_optimizer = "none", sample_count =
3.  Targets (tests/active_sample_host.py): a smooth anisotropic quadratic-plus-quartic log density, exact, and the same
with user-provided noise S = 0.3 + 0.1 |x_0| (uncertainty handling level 2).  Cases:
  a   the exact target, AcqFcnLog                       i1  initial design "plausible"
  b   the noisy target, AcqFcnNoisy (reupdate_gp)       i2  initial design "narrow"
  c   like a with a 6-row starting cache, 3 rows with   i3  more provided points than asked
      values, and search_cache_frac = 0.125
Per case: the inputs, the NumPy seed, and after the call the acquired X / y / S, the search bounds, optim_state["N"] and
["N_eff"], the cache remainder and one ``np.random.rand()``.  tests/active_sample_host.py ``load_case`` reads a case.

Asserted while generating: at every step of a, b, c the best and the second-best finite acquisition value differ by at
least 1e-6 relative (a device evaluation, correct to ~1e-10, then picks the same row); in c at least one acquired point
comes from the cache with a known value -- c's seed is raised from C_SEED until that holds, and the seed used is printed
and stored.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

from make_mtv_golden import _fields  # noqa: E402  (puts the reference checkout, the stubs and tests/ on sys.path)

import active_sample_host as ash  # noqa: E402
import gpyreg  # noqa: E402  (the stand-in)
from pyvbmc.acquisition_functions import AcqFcnLog, AcqFcnNoisy  # noqa: E402
from pyvbmc.function_logger import FunctionLogger  # noqa: E402
from pyvbmc.parameter_transformer import ParameterTransformer  # noqa: E402
from pyvbmc.variational_posterior import VariationalPosterior  # noqa: E402
from pyvbmc.vbmc.active_sample import active_sample  # noqa: E402
from pyvbmc_amd.gp import GaussianNoise  # noqa: E402

OUT = ROOT / "tests" / "golden" / "active_sample.npz"
D, K, N, S, SAMPLE_COUNT, CACHE_SIZE = 3, 2, 24, 2, 3, 40
NP_SEED, C_SEED = 11, 11
MIN_GAP = 1e-6


class ForceDict(dict):
    """``Options``' item assignment with ``force`` on a plain dict."""

    def __setitem__(self, key, value, force=False):
        dict.__setitem__(self, key, value)


class AppendingGP(gpyreg.GP):
    """gpyreg's ``update`` semantics on the stand-in."""

    def update(self, X_new=None, y_new=None, s2_new=None, hyp=None, compute_posterior=True):
        if hyp is None:
            hyp = np.stack([p.hyp for p in self.posteriors])
        if X_new is not None:
            self.X = np.vstack([self.X, np.atleast_2d(X_new)])
            self.y = np.vstack([self.y, np.reshape(y_new, (-1, 1))])
            if s2_new is not None:
                self.s2 = np.vstack([self.s2, np.reshape(s2_new, (-1, 1))])
        self.X = np.atleast_2d(np.asarray(self.X, dtype=np.float64))
        self.y = np.asarray(self.y, dtype=np.float64).reshape(-1, 1)
        super().update(None, None, None, hyp, compute_posterior)


def recording(cls, gaps):
    """The reference's acquisition class with the relative gap between the two best finite values of every set
    evaluation appended to ``gaps``."""

    class Recording(cls):
        def __call__(self, Xs, gp, vp, function_logger, optim_state):
            acq = super().__call__(Xs, gp, vp, function_logger, optim_state)
            if np.size(acq) > 1:
                v = np.sort(acq[np.isfinite(acq)])
                gaps.append(float((v[1] - v[0]) / max(abs(v[0]), abs(v[1]))))
            return acq

    Recording.__name__ = cls.__name__
    return Recording()


def base_inputs(name, noisy, n_cache, over):
    r = np.random.default_rng(2000 + sum(map(ord, name)))
    c = {"D": D, "K": K, "noisy": int(noisy), "sample_count": SAMPLE_COUNT, "cache_size": CACHE_SIZE}
    c["mu"] = 0.6 * r.standard_normal((D, K))
    c["sigma"] = np.array([[0.5, 0.8]])
    lam = 0.5 + r.random((D, 1))
    c["lambd"] = lam / np.sqrt(np.sum(lam**2) / D)
    c["w"] = np.array([[0.4, 0.6]])
    c["X0"] = 0.7 * r.standard_normal((N, D))  # transformed space
    c["hyp"] = np.array([np.concatenate([np.log(0.8 + 0.3 * r.random(D)), [np.log(2.0)], [np.log(0.05 * (s + 1))], [0.1],
                                         np.zeros(D), np.zeros(D)]) for s in range(S)])
    c["cache_x_orig"] = r.uniform(-3, 3, size=(n_cache, D))
    c["search_cache"] = 0.8 * r.standard_normal((50, D))
    opts = dict(ash.DEFAULT_OPTIONS, **over)
    c["options"] = np.array([float(opts[k]) for k in ash.NUMERIC_OPTIONS])
    return c


def reference_objects(c):
    lb, ub = np.full((1, D), -10.0), np.full((1, D), 10.0)
    plb, pub = np.full((1, D), -3.0), np.full((1, D), 3.0)
    pt = ParameterTransformer(D, lb, ub, plb, pub)
    vp = VariationalPosterior(D, K, parameter_transformer=pt)
    vp.mu, vp.sigma, vp.lambd, vp.w = c["mu"].copy(), c["sigma"].copy(), c["lambd"].copy(), c["w"].copy()
    noisy = bool(c["noisy"])
    log = FunctionLogger(ash.target_noisy if noisy else ash.target_exact, D, noisy, 2 if noisy else 0, CACHE_SIZE, pt)
    plb_tran, pub_tran = pt(plb), pt(pub)
    span = pub_tran - plb_tran
    c.update(lb_tran=pt(lb), ub_tran=pt(ub), plb_tran=plb_tran, pub_tran=pub_tran, lb_search=plb_tran - 0.75 * span,
             ub_search=pub_tran + 0.75 * span, lb_eps_orig=lb + 1e-6 * (ub - lb), ub_eps_orig=ub - 1e-6 * (ub - lb))
    return pt, vp, log


def optim_state_of(c):
    keys = ("lb_search", "ub_search", "lb_tran", "ub_tran", "plb_tran", "pub_tran", "lb_eps_orig", "ub_eps_orig")
    st = {k: np.array(c[k], dtype=np.float64) for k in keys}
    st.update(cache={"x_orig": c["cache_x_orig"].copy(), "y_orig": c["cache_y_orig"].copy()},
              search_cache=c["search_cache"].copy(), integer_vars=None, variance_regularized_acq_fcn=True, tol_gp_var=1e-4,
              iter=5, last_warmup=0, hyp_dict=None, recompute_var_post=True, entropy_alpha=0.0)
    return st


def options_of(c, name, acq=None):
    o = ForceDict(ash.DEFAULT_OPTIONS)
    for k, v in zip(ash.NUMERIC_OPTIONS, c["options"]):
        dict.__setitem__(o, k, int(v) if k == "ns_search" else float(v))
    if acq is not None:
        dict.__setitem__(o, "search_acq_fcn", [acq])
    if name in ash.DESIGN_OF:
        dict.__setitem__(o, "init_design", ash.DESIGN_OF[name])
    return o


def results(c, log, st, n0):
    sl = slice(n0, log.Xn + 1)
    c["ref_X"], c["ref_y"] = log.X[sl].copy(), log.y[sl].copy()
    c["ref_X_orig"], c["ref_y_orig"] = log.X_orig[sl].copy(), log.y_orig[sl].copy()
    c["ref_S"] = log.S[sl].copy() if hasattr(log, "S") else np.zeros((0, 1))
    c["ref_cache_x_orig"], c["ref_cache_y_orig"] = st["cache"]["x_orig"], st["cache"]["y_orig"]
    c["ref_func_count"], c["ref_cache_count"] = np.array(log.func_count), np.array(log.cache_count)
    c["ref_next_rand"] = np.array(np.random.rand())


def trajectory(name, seed):
    noisy = name == "b"
    over = dict(search_cache_frac=0.125) if name == "c" else {}
    c = base_inputs(name, noisy, 6 if name == "c" else 0, over)
    pt, vp, log = reference_objects(c)
    y_cache = np.full(c["cache_x_orig"].shape[0], np.nan)
    y_cache[::2] = [ash.target_exact(x) for x in c["cache_x_orig"][::2]]  # 3 of the 6 rows have values
    c["cache_y_orig"] = y_cache
    for x in c["X0"]:
        log(x)
    c["ref_y0"] = log.y[log.X_flag].copy()
    c["ref_S0"] = log.S[log.X_flag].copy() if noisy else np.zeros((0, 1))
    gp = AppendingGP(D, gpyreg.covariance_functions.SquaredExponential(), gpyreg.mean_functions.NegativeQuadratic(),
                     GaussianNoise(constant_add=True, user_provided_add=noisy))
    gp.X, gp.y = log.X[log.X_flag].copy(), log.y[log.X_flag].copy()
    gp.s2 = (log.S[log.X_flag] ** 2).copy() if noisy else None
    gp.update(hyp=c["hyp"])
    gaps = []
    st = optim_state_of(c)
    n_cache = len(y_cache)
    n_known = int(np.sum(~np.isnan(y_cache)))
    options = options_of(c, name, recording(AcqFcnNoisy if noisy else AcqFcnLog, gaps))
    c["np_seed"] = seed
    np.random.seed(seed)
    n0 = log.Xn + 1
    log, st, vp, gp = active_sample(gp, SAMPLE_COUNT, st, log, {"r_index": [1.0]}, vp, options)
    results(c, log, st, n0)
    c["ref_lb_search"], c["ref_ub_search"] = st["lb_search"], st["ub_search"]
    c["ref_N"], c["ref_N_eff"] = np.array(st["N"]), np.array(np.ravel(st["N_eff"])[0])
    assert len(gaps) == SAMPLE_COUNT and min(gaps) >= MIN_GAP, (name, gaps)
    from_cache = n_known - int(np.sum(~np.isnan(st["cache"]["y_orig"])))
    print(name, "seed", seed, "gaps", ["%.2e" % g for g in gaps], "cache rows left", len(st["cache"]["y_orig"]), "of", n_cache,
          "known values taken", from_cache, flush=True)
    return c, pt, from_cache


def design(name):
    n_cache, count = {"i1": (2, 5), "i2": (2, 5), "i3": (7, 4)}[name]
    c = base_inputs(name, False, n_cache, {})
    c["sample_count"] = count
    pt, vp, log = reference_objects(c)
    y_cache = np.full(n_cache, np.nan)
    y_cache[::2] = [ash.target_exact(x) for x in c["cache_x_orig"][::2]]
    c["cache_y_orig"] = y_cache
    st = optim_state_of(c)
    c["np_seed"] = NP_SEED
    np.random.seed(NP_SEED)
    log, st, vp, _ = active_sample(None, count, st, log, {"r_index": [1.0]}, vp, options_of(c, name))
    results(c, log, st, 0)
    print(name, "points", log.Xn + 1, "evaluated", log.func_count, "from the cache", log.cache_count, flush=True)
    return c, pt


def main():
    out = {}

    def store(name, c, pt):
        for k, v in c.items():
            out[f"{name}_{k}"] = np.asarray(v)
        for k, v in _fields(pt, D).items():
            out[f"{name}_pt_{k}"] = v

    for name in ("a", "b"):
        c, pt, _ = trajectory(name, NP_SEED)
        store(name, c, pt)
    seed = C_SEED
    while True:
        c, pt, from_cache = trajectory("c", seed)
        if from_cache >= 1:
            break
        seed += 1
    store("c", c, pt)
    for name in ash.DESIGNS:
        store(name, *design(name))
    out["numeric_options"] = np.array(ash.NUMERIC_OPTIONS)
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
