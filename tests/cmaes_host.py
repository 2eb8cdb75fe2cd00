"""The CMA-ES of the acquisition search's refinement, stated in NumPy.  TEST INFRASTRUCTURE: csrc/cmaes.hip (the kernel)
and pyvbmc_amd/cmaes.py (product NumPy) are compared with it; it imports neither.  There is no reference counterpart:
the reference calls the third-party ``cma.fmin`` (vbmc/active_sample.py:398-404), which is not part of its tree.

``CMAES`` is an ask / tell object:

    es = CMAES(x0, sigma0, lb, ub, max_fevals=..., tol_fun=..., seed=...)
    while not es.stop:
        X = es.ask()                      # generation 0: x0 itself, one row; then lambda rows
        Xe = rounded(X)                   # what is evaluated: integer columns rounded (AbstractAcqFcn._real2int)
        es.tell(values_of(Xe), Xe)

A (mu/mu_w, lambda)-CMA-ES for minimisation in a box: explicit covariance C, lower Cholesky factor L recomputed every
generation, candidates clipped to the box, the update on the repaired steps y = (x - m) / sigma and z' = L^-1 y.  Draws:
candidate i of generation g is Philox block (n_lo, n_hi, pair, 8), n = g lambda + i, under the key
seed + (run + 1) 0x9E3779B97F4A7C15 (oracle/philox_ref.py ``normals``).  Sums run in rank order, then d ascending, one
multiply and one add per term.  Ranking: ascending, the index breaks ties, NaN behind +inf.  Stop reasons, checked after
the update, the first that holds: 1 tolfun, 2 tolx, 3 maxfevals, 4 condition, 5 invalid.

``twin``: a NumPy generator.  Every operation in which the device differs from this file -- exp, 1 / sqrt, 1 / sigma,
every normal -- is then multiplied by 1 + 4 eps xi, xi uniform in [-1, 1]: the twin's distance from the plain run
measures how the recursion amplifies errors of that size (tests/test_cmaes_host.py, tests/test_search_cmaes_gpu.py).

``cases()`` are the replay cases of both test files, built from tests/search_host.py's fixtures; ``objective`` is a case's
acquisition function on the host (``acq_values`` after ``real2int``).
"""
import math
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import search_host as sh  # noqa: E402

from oracle import acq_ref, gp_ref, philox_ref  # noqa: E402

STREAM = 8
KEY_STEP = 0x9E3779B97F4A7C15
EPS = np.finfo(np.float64).eps
PARITY = 1e-9  # the acquisition parity bound of tests/test_search_gpu.py: |device - host| <= 1e-9 max(1, |value|)


def run_key(seed, run):
    return (int(seed) + (run + 1) * KEY_STEP) % 2**64


class CMAES:
    def __init__(self, x0, sigma0, lb, ub, *, lam=None, max_fevals, tol_fun, tol_x=None, seed, run=0, twin=None):
        self.x0 = np.array(np.ravel(x0), dtype=np.float64)
        self.lb, self.ub = np.array(np.ravel(lb), dtype=np.float64), np.array(np.ravel(ub), dtype=np.float64)
        D = self.D = self.x0.size
        self.lam = lam = 4 + int(math.floor(3.0 * math.log(D))) if lam is None else int(lam)
        assert 2 <= D <= 32 and 4 <= lam <= 64 and sigma0 > 0 and max_fevals >= 1 + lam
        assert np.all(self.lb <= self.x0) and np.all(self.x0 <= self.ub)
        self.max_fevals, self.tol_fun = int(max_fevals), float(tol_fun)
        self.sigma0 = float(sigma0)
        self.tol_x = float(tol_x) if tol_x is not None and tol_x > 0 else 1e-11 * self.sigma0
        self.key = run_key(seed, run)
        self.twin = twin
        # ---- population, weights, learning rates
        d = float(D)
        mu = self.mu = lam // 2
        w = [math.log((lam + 1) / 2.0) - math.log(float(i)) for i in range(1, mu + 1)]
        sw = 0.0
        for v in w:
            sw = sw + v
        self.w = w = [v / sw for v in w]
        s2 = 0.0
        for v in w:
            s2 = s2 + v * v
        mueff = self.mueff = 1.0 / s2
        self.cs = (mueff + 2.0) / (d + mueff + 5.0)
        self.ds = 1.0 + 2.0 * max(0.0, math.sqrt((mueff - 1.0) / (d + 1.0)) - 1.0) + self.cs
        self.cc = (4.0 + mueff / d) / (d + 4.0 + 2.0 * mueff / d)
        self.c1 = 2.0 / ((d + 1.3) * (d + 1.3) + mueff)
        self.cmu = min(1.0 - self.c1, 2.0 * (mueff - 2.0 + 1.0 / mueff) / ((d + 2.0) * (d + 2.0) + mueff))
        self.chi = math.sqrt(d) * (1.0 - 1.0 / (4.0 * d) + 1.0 / (21.0 * d * d))
        self.hist = 10 + -(-30 * D // lam)
        # ---- state
        self.mean, self.sigma = self.x0.copy(), self.sigma0
        self.C, self.L, self.rdiag = np.eye(D), np.eye(D), [1.0] * D
        self.ps, self.pc = [0.0] * D, [0.0] * D
        self.decay = 1.0  # (1 - c_sigma)^(2 g)
        self.ring = []
        self.generations, self.evaluations, self.best_gen, self.stop = 0, 0, 0, 0
        self.x_best, self.f_best, self.f0 = None, None, None
        self.started = False
        self.history = []  # per generation: (order, values)
        self.gap = math.inf  # smallest distance of neighbouring ranked values over the run, in units of max(1, |value|)
        self.tied_rows_only = True  # exact ties met so far were between bitwise identical evaluated rows, or non-finite

    # the operations in which the device's arithmetic differs
    def _p(self, v):
        return v if self.twin is None else v * (1.0 + 4.0 * EPS * float(self.twin.uniform(-1.0, 1.0)))

    def _rsqrt(self, v):
        return self._p(1.0 / math.sqrt(v))

    @property
    def stats(self):
        return np.array([self.generations, self.evaluations, self.stop, self.best_gen], dtype=np.int64)

    def ask(self):
        assert not self.stop
        if not self.started:
            return self.x0[None, :].copy()
        D, lam, L, m, sigma = self.D, self.lam, self.L, self.mean, self.sigma
        Z = philox_ref.normals(np.arange(self.generations * lam, (self.generations + 1) * lam, dtype=np.uint64), D, self.key, STREAM)
        if self.twin is not None:
            Z = Z * (1.0 + 4.0 * EPS * self.twin.uniform(-1.0, 1.0, size=Z.shape))
        inv_sigma = self._p(1.0 / sigma)
        X, Y, Zp = np.empty((lam, D)), np.empty((lam, D)), np.empty((lam, D))
        for i in range(lam):
            z = [float(v) for v in Z[i]]
            for d in range(D):
                acc = 0.0
                for k in range(d + 1):
                    acc = acc + float(L[d, k]) * z[k]
                x = float(m[d]) + sigma * acc
                x = float(self.lb[d]) if x < self.lb[d] else x
                x = float(self.ub[d]) if x > self.ub[d] else x
                X[i, d] = x
                Y[i, d] = (x - float(m[d])) * inv_sigma
            zp = []
            for d in range(D):
                acc = float(Y[i, d])
                for k in range(d):
                    acc = acc - float(L[d, k]) * zp[k]
                zp.append(acc * self.rdiag[d])
            Zp[i] = zp
        self.X, self.Y, self.Zp = X, Y, Zp
        return X.copy()

    def tell(self, values, X_eval):
        values = np.asarray(values, dtype=np.float64).ravel()
        X_eval = np.asarray(X_eval, dtype=np.float64)
        if not self.started:
            self.started = True
            self.f0 = self.f_best = float(values[0])
            self.x_best = X_eval[0].copy()
            self.evaluations = 1
            if not math.isfinite(self.f0):
                self.stop = 5
            return
        D, lam, mu, w = self.D, self.lam, self.mu, self.w
        order = sorted(range(lam), key=lambda i: (1, 0.0, i) if values[i] != values[i] else (0, float(values[i]), i))
        self.history.append((list(order), values.copy()))
        for a, b in zip(order[:-1], order[1:]):
            va, vb = values[a], values[b]
            if math.isfinite(va) and math.isfinite(vb):
                if va == vb:
                    self.tied_rows_only = self.tied_rows_only and np.array_equal(X_eval[a], X_eval[b])
                else:
                    self.gap = min(self.gap, (vb - va) / max(1.0, abs(va), abs(vb)))
        self.evaluations += lam
        self.generations += 1
        vbest = float(values[order[0]])
        if not math.isfinite(vbest):
            self.stop = 5
            return
        if vbest < self.f_best:
            self.f_best, self.x_best, self.best_gen = vbest, X_eval[order[0]].copy(), self.generations
        Y, Zp, sigma = self.Y, self.Zp, self.sigma
        # ---- recombination and paths
        yw, zw = [0.0] * D, [0.0] * D
        for d in range(D):
            for i in range(mu):
                yw[d] = yw[d] + w[i] * float(Y[order[i], d])
                zw[d] = zw[d] + w[i] * float(Zp[order[i], d])
        self.mean = np.array([float(self.mean[d]) + sigma * yw[d] for d in range(D)])
        a_ps = math.sqrt(self.cs * (2.0 - self.cs) * self.mueff)
        ps = self.ps = [(1.0 - self.cs) * self.ps[d] + a_ps * zw[d] for d in range(D)]
        n2 = 0.0
        for d in range(D):
            n2 = n2 + ps[d] * ps[d]
        nps = math.sqrt(n2)
        self.decay = self.decay * ((1.0 - self.cs) * (1.0 - self.cs))
        hs = 1.0 if nps * self._rsqrt(1.0 - self.decay) < (1.4 + 2.0 / (float(D) + 1.0)) * self.chi else 0.0
        a_pc = math.sqrt(self.cc * (2.0 - self.cc) * self.mueff)
        pc = self.pc = [(1.0 - self.cc) * self.pc[d] + (hs * a_pc) * yw[d] for d in range(D)]
        # ---- covariance: entry by entry, the rank-mu terms in rank order
        keep = (1.0 - hs) * (self.cc * (2.0 - self.cc))
        c_old = 1.0 - self.c1 - self.cmu
        pcv = np.array(pc)
        C = c_old * self.C + self.c1 * (np.multiply.outer(pcv, pcv) + keep * self.C)
        for k in range(mu):
            y = Y[order[k]]
            C = C + (self.cmu * w[k]) * np.multiply.outer(y, y)
        self.C = C
        self.sigma = sigma * self._p(math.exp((self.cs / self.ds) * (nps * (1.0 / self.chi) - 1.0)))
        # ---- L = chol(C)
        L, ok = np.zeros((D, D)), True
        rdiag = [1.0] * D
        for j in range(D):
            s = float(C[j, j])
            for k in range(j):
                s = s - float(L[j, k]) * float(L[j, k])
            if not (0.0 < s < math.inf):
                ok = False
                break
            r = self._rsqrt(s)
            L[j, j], rdiag[j] = s * r, r
            for i in range(j + 1, D):
                t = float(C[i, j])
                for k in range(j):
                    t = t - float(L[i, k]) * float(L[j, k])
                L[i, j] = t * r
        self.L, self.rdiag = L, rdiag
        # ---- stop rules
        self.ring = (self.ring + [vbest])[-self.hist:]
        finite = [float(v) for v in values if math.isfinite(v)]
        if len(self.ring) >= self.hist and max(self.ring) - min(self.ring) < self.tol_fun and max(finite) - vbest < self.tol_fun:
            self.stop = 1
        elif self.sigma * max(max(math.sqrt(C[d, d]) if C[d, d] > 0 else 0.0, abs(pc[d])) for d in range(D)) < self.tol_x:
            self.stop = 2
        elif self.evaluations + lam > self.max_fevals:
            self.stop = 3
        elif not ok:
            self.stop = 4
        else:
            dl = [float(L[d, d]) for d in range(D)]
            if max(dl) * max(dl) > 1e14 * (min(dl) * min(dl)):
                self.stop = 4


def run(es, f_batch, evaluated=None):
    """Drive ``es`` to its stop: ``f_batch(X)`` the values of rows, ``evaluated(X)`` the rows that are evaluated."""
    while not es.stop:
        X = es.ask()
        Xe = X if evaluated is None else np.asarray(evaluated(X.copy()), dtype=np.float64)
        es.tell(f_batch(Xe), Xe)
    return es


# ---------------------------------------------------------------------------------------------- the replay cases
def make_ais(ogp, mix, Na, seed):
    """A small importance state for the VIQR case: Na points around the mixture's centres, the GP's own variances."""
    r = np.random.default_rng(seed)
    k = r.integers(0, mix.K, size=Na)
    Xa = mix.mu.T[k] + 0.5 * r.standard_normal((Na, mix.D)) * mix.lambd.reshape(1, -1)
    _, f_s2 = gp_ref.predict(ogp, Xa, separate_samples=True)
    return {"X": Xa, "f_s2": f_s2, "ln_weights": np.zeros((f_s2.shape[1], Na))}


def _wide(D, N, seed, centre=25.0, sigma_scale=1.0):
    return sh.wide_case(D=D, K=2, N=N, number_of_points=64, seed=seed, centre=centre, sigma_scale=sigma_scale)


# name -> (how the case is built, acquisition, lambda, max_fevals, seed).  The seeds are chosen on the CPU so that the
# margin condition of tests/test_cmaes_host.py holds (tools/search_cmaes_seeds.py searches them).
SPECS = {
    "d2": dict(D=2, N=40, acq="AcqFcnLog", lam=None, gens=40, seed=2),
    "b_int": dict(golden="b", integer=True, acq="AcqFcnLog", lam=None, gens=40, seed=21),
    "d5": dict(D=5, N=40, acq="AcqFcnLog", lam=None, gens=40, seed=1),
    "d32": dict(D=32, N=40, acq="AcqFcnLog", lam=None, gens=30, seed=1),
    "lam64": dict(D=4, N=40, acq="AcqFcnLog", lam=64, gens=8, seed=2),
    "noisy": dict(golden="d", acq="AcqFcnNoisy", lam=None, gens=40, seed=17),
    "viqr": dict(golden="d", acq="AcqFcnVIQR", lam=None, gens=30, seed=3),
    # the workload's dimensions (bench.py: D = 10, 20) with their default populations, lambda = 10 (mu = 5) and 12 (mu = 6);
    # each takes the first seed of 1, 2, ... that tools/search_cmaes_seeds.py calls usable (d20: seed 1 leaves a gap of 306
    # parity bounds, under the 1000 asked)
    "d10": dict(D=10, N=40, acq="AcqFcnLog", lam=None, gens=30, seed=1),
    "d20": dict(D=20, N=40, acq="AcqFcnLog", lam=None, gens=30, seed=2),
    # D = 13 (padded width 16, lambda = 11) with the noisy acquisition.  Its value is a product with exp(f_bar - y_max) p(x):
    # around centre 25 the zero-centred quadratic mean makes it underflow to -0 everywhere, and at the fixture's mixture
    # widths p is ~1e-4 in 13 dimensions, so that no two ranked values are 1e-6 apart.  Centre 0, half the widths and a
    # start step that stays inside the mixture keep the values O(0.1) over the whole run.
    "d13_noisy": dict(D=13, N=40, acq="AcqFcnNoisy", centre=0.0, sigma_scale=0.5, sigma0=0.05, lam=None, gens=30, seed=1),
}
KINDS = {"AcqFcn": acq_ref.STD, "AcqFcnLog": acq_ref.LOG, "AcqFcnVanilla": acq_ref.VANILLA, "AcqFcnNoisy": acq_ref.NOISY,
         "AcqFcnVIQR": "viqr"}
U75 = 0.6744897501960817  # norm.ppf(0.75)


def build_case(name, golden=None, seed=None):
    """The inputs of replay case ``name``: the search fixture, the oracle GP (S = 2), the optimiser's arguments."""
    spec = SPECS[name]
    if "golden" in spec:
        c = sh.load_case(golden("search"), spec["golden"])
    else:
        c = _wide(spec["D"], spec["N"], 5 + spec["D"], spec.get("centre", 25.0), spec.get("sigma_scale", 1.0))
    D = c.D
    ogp, length, sn2_new = sh.gp_fixture(c, 2)
    y = c.flog.y[c.flog.X_flag]
    state = dict(c.optim_state, integer_vars=None, gp_length_scale=length, tol_gp_var=1e-4, variance_regularized_acq_fcn=False)
    lb, ub = np.ravel(c.optim_state["lb_search"]).copy(), np.ravel(c.optim_state["ub_search"]).copy()
    if not (np.isfinite(lb).all() and np.isfinite(ub).all()):  # the box of active_sample.py:372-375
        span = ogp.X.max(0) - ogp.X.min(0)
        lb, ub = ogp.X.min(0) - 0.1 * span, ogp.X.max(0) + 0.1 * span
    if spec.get("integer"):
        # one integer variable; hard bounds that the start's neighbourhood crosses in dimension 0
        state["integer_vars"] = np.array([False, True, False])
        x0 = np.ravel(c.mix.mu[:, 0]).copy()
        x0 = np.minimum(np.maximum(x0, lb), ub)
        xo = np.ravel(c.pt.inverse(x0[None, :]))
        state["lb_eps_orig"] = np.full(D, -9.5)
        state["ub_eps_orig"] = np.full(D, 9.5)
        state["ub_eps_orig"][0] = xo[0] + 0.25 * (9.5 - xo[0]) if xo[0] < 9.0 else 9.5
        sigma0 = 0.5
    elif "golden" in spec:
        state["lb_eps_orig"] = np.full(D, -7.5)  # (the hard bounds of tests/test_search_gpu.py: they cut off part of the box)
        state["ub_eps_orig"] = np.full(D, 8.5)
        x0 = np.minimum(np.maximum(np.ravel(c.mix.mu[:, 0]), lb), ub)
        sigma0 = 0.5
    else:
        state["lb_eps_orig"] = np.full(D, -1e3)
        state["ub_eps_orig"] = np.full(D, 1e3)
        x0 = np.minimum(np.maximum(np.ravel(c.mix.mu[:, 0]) + 0.3, lb), ub)
        sigma0 = spec.get("sigma0", 0.4)
    lam = spec["lam"] if spec["lam"] is not None else 4 + int(math.floor(3.0 * math.log(D)))
    kind = KINDS[spec["acq"]]
    ais = make_ais(ogp, c.mix, 24, 77) if kind == "viqr" else None
    tol_fun = 1e-2 if spec["acq"] in ("AcqFcnLog", "AcqFcnVIQR") else 1e-12
    return SimpleNamespace(name=name, case=c, D=D, ogp=ogp, length=length, sn2_new=sn2_new, X_rescaled=ogp.X / length,
                           y_max=float(np.max(y)), state=state, kind=kind, acq=spec["acq"], ais=ais, x0=x0, sigma0=sigma0, lb=lb,
                           ub=ub, lam=lam, max_fevals=1 + spec["gens"] * lam, tol_fun=tol_fun,
                           seed=spec["seed"] if seed is None else seed)


def evaluated(k):
    """X -> the rows that are evaluated (integer columns rounded)."""
    return lambda X: sh.real2int(X, k.case.pt, k.state["integer_vars"])


def objective(k):
    """The case's acquisition function on the host, hard-bound mask applied, on rows that are rounded already."""
    def f(X):
        return sh.acq_values(k.kind, np.asarray(X, dtype=np.float64), k.ogp, k.case.mix, k.y_max, k.state, k.case.pt,
                             k.X_rescaled, k.sn2_new, ais=k.ais, u=U75)
    return f


def statement(k, twin=None, max_fevals=None, x0=None, run_index=0):
    return CMAES(k.x0 if x0 is None else x0, k.sigma0, k.lb, k.ub, lam=k.lam, max_fevals=k.max_fevals if max_fevals is None else max_fevals,
                 tol_fun=k.tol_fun, seed=k.seed, run=run_index, twin=twin)


def replay(k, twin=None, **kw):
    return run(statement(k, twin, **kw), objective(k), evaluated(k))


def drift(es, tw, k):
    """The twin's deviation from the plain run per quantity: x_best and mean in units of the box, sigma relative, C
    relative to max |C|."""
    box = k.ub - k.lb
    return {"x_best": float(np.max(np.abs(es.x_best - tw.x_best) / box)), "mean": float(np.max(np.abs(es.mean - tw.mean) / box)),
            "sigma": abs(es.sigma - tw.sigma) / es.sigma, "C": float(np.max(np.abs(es.C - tw.C)) / np.max(np.abs(es.C)))}


def drift_bounds(k, es=None):
    """100 x the twin's largest deviation per quantity (fixed NumPy seed), and that the twin kept every rank."""
    es = replay(k) if es is None else es
    tw = replay(k, twin=np.random.default_rng(20261020))
    same_ranks = len(es.history) == len(tw.history) and all(a[0] == b[0] for a, b in zip(es.history, tw.history))
    dev = drift(es, tw, k)
    # a quantity the twin reproduces exactly (a best point on the box's faces) still differs on the device by rounding
    return {q: 100.0 * max(v, 4.0 * EPS) for q, v in dev.items()}, dev, same_ranks and np.array_equal(es.stats, tw.stats)
