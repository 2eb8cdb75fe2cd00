"""The target and the replay cases of GP hyper-parameter sampling (``vbmc_gp_hyp_sample``, pyvbmc_amd/csrc/gp_hyp.hip;
``pyvbmc_amd.gp.sample_hyperparameters``), stated in NumPy.  TEST INFRASTRUCTURE shared by tests/test_hyp_slice_host.py
(the cases' preconditions, on the CPU) and tests/test_gp_hyp_gpu.py (the replay itself).

The target is f(h) = lml(h) + log p(h): lml the textbook formula of tests/gp_lml_host.py, a candidate that does not
factorise having f = -inf; log p(h) = sum_p t_p with t_p = 0 where sigma_p is NaN, the Gaussian's log density of
(h_p - mu_p) / sigma_p where df_p is +inf and the Student-t's otherwise.  The sampler is tests/slice_host.py's, unchanged.

A replay is only meaningful when every float comparison the chain makes is decided by more than the two sides can differ:
``replay`` records, next to the chain's own ``margin``, the largest error bound of any value it compared.
"""
import math
from functools import lru_cache

import numpy as np

import gp_lml_host as glh
import gp_post_host as gph
import slice_host
from oracle import gp_ref

EPS = np.finfo(np.float64).eps


def prior_terms(h, priors):
    """(constant parts c_p, h-dependent parts v_p) of the prior's terms t_p = c_p + v_p; both 0 without a prior."""
    h = np.asarray(h, dtype=np.float64)
    c, v = np.zeros(h.size), np.zeros(h.size)
    for p in range(h.size):
        mu, sg, nu = priors["mu"][p], priors["sigma"][p], priors["df"][p]
        if np.isnan(sg):
            continue
        z = (h[p] - mu) / sg
        if np.isinf(nu):
            c[p] = -0.5 * math.log(2 * math.pi) - math.log(sg)
            v[p] = -0.5 * z * z
        else:
            c[p] = math.lgamma((nu + 1) / 2) - math.lgamma(nu / 2) - 0.5 * math.log(math.pi * nu) - math.log(sg)
            v[p] = -(nu + 1) / 2 * math.log1p(z * z / nu)
    return c, v


def log_prior(h, priors):
    c, v = prior_terms(h, priors)
    lp = 0.0
    for p in range(c.size):  # p ascending
        lp += c[p] + v[p]
    return lp


def prior_bound(h, priors):
    """16 eps sum_p (|c_p| + |v_p|): the device's constants are the C library's, its logarithm fastmath.h's (under 2.5
    ulp, profiles/fastmath_ulp.md), and the terms are added one by one."""
    c, v = prior_terms(h, priors)
    return 16 * EPS * float(np.sum(np.abs(c) + np.abs(v)))


class Case:
    """One replay case: data, C starts (3 unless given), the chain's arguments."""

    def __init__(self, N, D, mean, with_s2, seed, chains=3, n=2, thin=2, burn_in=1):
        self.N, self.D, self.mean, self.seed = N, D, mean, seed
        self.X, self.y, self.x0 = gph.make_case(N, D, chains, mean, seed=100 + N)
        self.s2 = glh.reference(N, D, 2, mean, True)[3] if with_s2 else None
        P = self.x0.shape[1]
        self.P = P
        self.lb, self.ub = self.x0.min(0) - 1.5, self.x0.max(0) + 1.5
        self.lb[D + 1] = np.log(0.05)
        self.widths = np.full(P, 0.6)
        pri = {k: np.full(P, np.nan) for k in ("mu", "sigma", "df")}
        pri["mu"][:D], pri["sigma"][:D], pri["df"][:D] = np.log(1.5), 1.0, 3.0
        pri["mu"][D + 1], pri["sigma"][D + 1], pri["df"][D + 1] = np.log(0.3), 0.5, 3.0
        self.priors = pri
        self.n, self.thin, self.burn_in = n, thin, burn_in

    def value(self, h):
        """dict(f, lml_bound = factor_of(h) vabs, prior_bound) of one point; f = -inf (bounds 0) when it does not
        factorise or is not finite."""
        try:
            with np.errstate(all="ignore"):
                r = glh.lml_and_grad(h, self.X, self.y, self.mean, self.s2, self.s2 is not None)
                f = float(r["lml"]) + log_prior(h, self.priors)
            if not np.isfinite(f):
                raise np.linalg.LinAlgError("not finite")
        except np.linalg.LinAlgError:
            return dict(f=-np.inf, lml_bound=0.0, prior_bound=0.0)
        fac = glh.factor_of(h, self.X, self.s2, self.s2 is not None)
        return dict(f=f, lml_bound=fac * float(r["vabs"]), prior_bound=prior_bound(h, self.priors))

    def log_post(self, h):
        return self.value(h)["f"]

    def chain(self, c, x0=None, seed=None):
        """slice_host.chain of chain index c over log_post, plus ``bound``: the largest error bound of a value compared."""
        worst = [0.0]

        def f(h):
            v = self.value(h)
            worst[0] = max(worst[0], v["lml_bound"] + v["prior_bound"])
            return v["f"]

        res = slice_host.chain(f, self.x0[c] if x0 is None else x0, self.widths, self.lb, self.ub, self.n, self.thin,
                               self.burn_in, seed=self.seed if seed is None else seed, s=c)
        res["bound"] = worst[0]
        return res


# (N, D, mean, user noise, seed): 2, 1 and 3 blocks of 64, each with a ragged last block, and all three means.  The seeds
# were chosen on the CPU (tests/test_hyp_slice_host.py asserts the condition they were chosen for).
CASES = {
    65: (65, 3, gp_ref.MEAN_NEGQUAD, False, 2),
    63: (63, 3, gp_ref.MEAN_CONST, True, 2),
    130: (130, 2, gp_ref.MEAN_ZERO, False, 3),
    # the workload's dimensions (bench.py: D = 10 and 20): P = 3 D + 3 = 33 and 63 hyper-parameters in the sweep and in the
    # prior arrays.  The host statement costs seconds per chain there, so D = 20 runs two chains of burn-in 1 and one kept
    # sweep: every coordinate is still swept twice.
    "d10": (65, 10, gp_ref.MEAN_NEGQUAD, False, 1),
    "d20": (70, 20, gp_ref.MEAN_NEGQUAD, True, 1, dict(chains=2, n=1, thin=1, burn_in=1)),
}


@lru_cache(maxsize=None)
def case(key):
    spec = CASES[key]
    return Case(*spec[:5], **(spec[5] if len(spec) > 5 else {}))


@lru_cache(maxsize=None)
def replay(key):
    """The chains of a case on the host, computed once."""
    cs = case(key)
    return [cs.chain(c) for c in range(cs.x0.shape[0])]
