"""Extended-precision restatement of the GP posterior, ``predict`` and ``gp_log_joint`` for ill-conditioned training
covariances.  TEST INFRASTRUCTURE, like gp_lml_host.py: it touches neither the library nor the device.

At cond2(A) >= 1e7 (A = K / sl + diag(sn2 / sn2_div), the matrix that gets factorised) the float64 oracle
(oracle/gp_ref.py) is itself off by more than the project's 1e-10 bounds, so a device-against-oracle comparison says
nothing there.  Here the same formulas run in ``np.longdouble`` (64-bit mantissa) on the float64 inputs:

* ``truth(name)``: the Cholesky factor and its inverse by gp_lml_host.cholesky_upper / upper_inverse, and ONE step of
  iterative refinement in long double on every solve, x <- x + C^-1 (b - C x), C = K + diag(sn2).  The refined values
  are the truth; what the refinement step changed in a quantity is kept as the truth's own error estimate
  (``truth(name)["corr"]``).  The posterior is the same mathematics in both noise branches (``L_chol`` or not), so one
  restatement serves both.
* ``e64(name)``: the slack the reference's float64 arithmetic needs.  Per quantity the larger absolute error against
  the truth of two float64 CPU computations: (a) oracle/gp_ref (triangular solves), (b) NumPy by the device's route --
  gp_post_host.posterior's explicit L^-1, V = L^-T k*, alpha = L^-1 L^-T r / sl, one product Z L^-1 plus a Gram matrix
  for J (a sample on the non-Cholesky branch: the host record L = -(K + diag(sn2))^-1, alpha = -L r, k*^T (L k*) and
  Z (L Z^T), as the device reads it).  Both are reference-side arithmetic.

Quantities and their keys (S samples, M query points, K components):
    alpha (S, N) | mu, s2 (M, S) | mu_avg, s2_avg (M) | G_s (S), G | dG_mu, dG_sigma, dG_lambd, dG_w (averaged blocks)
    | I_sk (S, K) | J_sjk (S, K, K) | varG, var_ss (averaged, gp_ref.gp_log_joint's law).
An error is the largest absolute difference over the entries of a key; for the keys with a sample axis it is taken per
sample, so the well-conditioned sample that every case carries gets no slack from the ill-conditioned one.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import gp_lml_host as glh
import gp_post_host as gph
from oracle import gp_ref, mixture_ref

LD = np.longdouble
M_QUERY, M_SMALL, K_MIX = 64, 24, 3
PER_SAMPLE = ("alpha", "mu", "s2", "G_s", "I_sk", "J_sjk")  # keys with a sample axis (axis 1 for mu, s2; else axis 0)
DG_BLOCKS = ("dG_mu", "dG_sigma", "dG_lambd", "dG_w")
PREDICT_KEYS = ("mu", "s2", "mu_avg", "s2_avg")

Case = namedtuple("Case", "name N D f sn mean L_chol")
# The ill-conditioned sample of every case: ell = f (1 + 0.2 U), sf = 1.2, m0 = 0.1, omega = 2.5 on points of spread 2.
# D = 10: f chosen so that cond2(A) >= 1e6 (cond2 is 1.3e6 at f = 12, 7.4e6 at f = 16, 2.6e7 at f = 20); it runs
# glj_block.h's padded widths.
CASES = [
    Case("n130_d3_sn5e-3", 130, 3, 3.0, 5e-3, gp_ref.MEAN_NEGQUAD, True),
    Case("n65_d2_sn1e-3", 65, 2, 2.0, 1e-3, gp_ref.MEAN_CONST, True),
    Case("n130_d3_sn1e-3", 130, 3, 3.0, 1e-3, gp_ref.MEAN_NEGQUAD, True),
    Case("n257_d3_sn1e-3", 257, 3, 4.0, 1e-3, gp_ref.MEAN_NEGQUAD, True),
    Case("n130_d3_sn5e-4", 130, 3, 3.0, 5e-4, gp_ref.MEAN_NEGQUAD, False),
    Case("n130_d10_sn1e-3", 130, 10, 16.0, 1e-3, gp_ref.MEAN_NEGQUAD, True),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
# the append test builds this case's first N - 1 points and appends the last: the truth of the N points is the case's own
APPEND_CASE = "n130_d3_sn1e-3"


def require_extended():
    """np.longdouble must carry a 64-bit mantissa: without it the restatement is no truth at all."""
    nmant = np.finfo(LD).nmant
    assert nmant >= 63, (f"np.longdouble has a {nmant}-bit mantissa on this platform; the extended-precision GP "
                         f"reference needs 63 or more (x87 extended or IEEE quad)")


# ---- data ---------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def data(name):
    """dict(X, y, hyp (2, P), xs (M_QUERY, D), mix) of a case: sample 0 ill-conditioned, sample 1 a
    gp_post_host.make_case(well=True)-style one.  The first M_SMALL query points hold 8 of each kind (training points
    + 0.3 randn, + 1e-3 randn, and themselves), so the M <= 32 path sees all three."""
    c = BY_NAME[name]
    N, D = c.N, c.D
    rng = np.random.default_rng(100 + N)
    X = 2.0 * rng.standard_normal((N, D))
    y = -0.5 * np.sum(X**2, axis=1) / D + 0.3 * rng.standard_normal(N)
    P = D + 2 + gp_ref.mean_n(c.mean, D)
    hyp = np.zeros((2, P))
    hyp[0, :D] = np.log(c.f * (1 + 0.2 * rng.random(D)))
    hyp[0, D], hyp[0, D + 1], hyp[0, D + 2] = np.log(1.2), np.log(c.sn), 0.1
    hyp[1, :D] = np.log(0.8 * np.sqrt(D) * (1 + 0.2 * rng.random(D)))
    hyp[1, D] = np.log(1.0 + 0.3 * rng.random())
    hyp[1, D + 1] = np.log(0.3 * (1 + 0.2 * rng.random()))
    hyp[1, D + 2] = 0.2 * rng.standard_normal()
    if c.mean == gp_ref.MEAN_NEGQUAD:
        hyp[0, 2 * D + 3 :] = np.log(2.5)
        hyp[1, D + 3 : 2 * D + 3] = 0.1 * rng.standard_normal(D)
        hyp[1, 2 * D + 3 :] = np.log(2.0 + rng.random(D))
    far = X[rng.integers(0, N, 32)] + 0.3 * rng.standard_normal((32, D))
    near = X[rng.integers(0, N, 16)] + 1e-3 * rng.standard_normal((16, D))
    on = X[rng.integers(0, N, 16)]
    xs = np.vstack([far[:8], near[:8], on[:8], far[8:], near[8:], on[8:]])
    sigma = 0.3 + 0.3 * rng.random(K_MIX)
    lambd = 1 + 0.3 * rng.random(D)
    lambd = lambd / np.sqrt(np.sum(lambd**2) / D)
    mix = mixture_ref.Mixture.make(X[:K_MIX].T + 0.2, sigma, lambd, [0.5, 0.3, 0.2])
    return dict(X=X, y=y.reshape(-1, 1), hyp=hyp, xs=np.ascontiguousarray(xs), mix=mix)


def scaled_matrix(h, X):
    """A = K / sl + I of one sample under constant noise (float64), symmetric."""
    N, D = X.shape
    sn2, sn2_div, sl = gph.noise_scalars(h, N, D)
    A = gph.cov_matrix(h, X, sn2, sn2_div, sl)
    return A + np.triu(A, 1).T


@lru_cache(maxsize=None)
def cond2(name):
    d = data(name)
    return [float(np.linalg.cond(scaled_matrix(h, d["X"]))) for h in d["hyp"]]


# ---- the formulas, in the dtype of their arguments ----------------------------------------------------------------
def _se(hc, A, B):
    """gp_ref.se_ard (direct differences) in the arguments' dtype."""
    D = A.shape[1]
    ell = np.exp(hc[:D])
    a, b = A / ell, B / ell
    d2 = np.sum((a[:, None, :] - b[None, :, :]) ** 2, axis=2)
    return np.exp(2 * hc[D]) * np.exp(-d2 / 2)


def _mean(kind, hm, X):
    return glh.mean_and_grad(kind, hm, X)[0]


def _average(mu, s2):
    """gp_ref.predict's averaging law over the sample axis (axis 1)."""
    S = mu.shape[1]
    fbar = np.sum(mu, axis=1) / S
    v = np.sum(s2, axis=1) / S
    if S > 1:
        v = v + np.sum((mu - fbar[:, None]) ** 2, axis=1) / (S - 1)
    return fbar, v


def _predict(kind, X, hyp, xs, alpha, quad):
    """mu, s2 (M, S) and the averaged pair; ``quad[s](Ks)`` = k*^T C^-1 k* per column of Ks (N, M)."""
    D = X.shape[1]
    M, S = xs.shape[0], hyp.shape[0]
    mu, s2 = np.zeros((M, S), dtype=X.dtype), np.zeros((M, S), dtype=X.dtype)
    for s, h in enumerate(hyp):
        Ks = _se(h[: D + 1], X, xs)
        mu[:, s] = _mean(kind, h[D + 2 :], xs) + Ks.T @ alpha[s]
        s2[:, s] = np.maximum(np.exp(2 * h[D]) - quad[s](Ks), 0)
    mu_avg, s2_avg = _average(mu, s2)
    return dict(mu=mu, s2=s2, mu_avg=mu_avg, s2_avg=s2_avg)


def _log_joint(kind, X, hyp, mix, alpha, bilin):
    """gp_ref.gp_log_joint's formulas in X's dtype, all four gradient blocks with the Jacobian, the variance and the
    averaging over samples; ``bilin[s](Z)`` = Z C^-1 Z^T (K, K) of the rows of Z (K, N)."""
    dt = X.dtype.type
    N, D = X.shape
    S, K = hyp.shape[0], mix.K
    mu, sigma, lambd, w, eta = (np.asarray(a, dtype=np.float64).astype(dt)
                                for a in (mix.mu, mix.sigma, mix.lambd.reshape(-1, 1), mix.w, mix.eta))
    quad = kind == gp_ref.MEAN_NEGQUAD
    tiny = dt(np.spacing(1))
    G = np.zeros(S, dtype=dt)
    g_mu, g_sigma = np.zeros((D, K, S), dtype=dt), np.zeros((K, S), dtype=dt)
    g_lambd, g_w = np.zeros((D, S), dtype=dt), np.zeros((K, S), dtype=dt)
    varG, I_sk, J_sjk = np.zeros(S, dtype=dt), np.zeros((S, K), dtype=dt), np.zeros((S, K, K), dtype=dt)
    for s, h in enumerate(hyp):
        ell = np.exp(h[:D]).reshape(-1, 1)
        ln_sf2, sum_lnell = 2 * h[D], np.sum(h[:D])
        m0 = dt(0) if kind == gp_ref.MEAN_ZERO else h[D + 2]
        if quad:
            xm = h[D + 3 : 2 * D + 3].reshape(-1, 1)
            omega = np.exp(h[2 * D + 3 :]).reshape(-1, 1)
        Z = np.zeros((K, N), dtype=dt)
        for k in range(K):
            tau = np.sqrt(sigma[k] ** 2 * lambd**2 + ell**2)
            delta = (mu[:, k : k + 1] - X.T) / tau
            z = np.exp(ln_sf2 + sum_lnell - np.sum(np.log(tau)) - np.sum(delta**2, axis=0) / 2)
            Z[k] = z
            I_k = z @ alpha[s] + m0
            if quad:
                I_k = I_k - np.sum((mu[:, k : k + 1] ** 2 + sigma[k] ** 2 * lambd**2 - 2 * mu[:, k : k + 1] * xm + xm**2)
                                   / omega**2) / 2
            G[s] += w[k] * I_k
            I_sk[s, k] = I_k
            g = w[k] * ((-(delta / tau) * z) @ alpha[s])
            if quad:
                g = g - w[k] / omega.ravel() ** 2 * (mu[:, k] - xm.ravel())
            g_mu[:, k, s] = g
            dz = np.sum((lambd / tau) ** 2 * (delta**2 - 1), axis=0) * sigma[k] * z
            g = w[k] * (dz @ alpha[s])
            if quad:
                g = g - w[k] * sigma[k] * np.sum(lambd**2 / omega**2)
            g_sigma[k, s] = g
            dz = (sigma[k] / tau) ** 2 * (delta**2 - 1) * (lambd * z)
            g = w[k] * (dz @ alpha[s])
            if quad:
                g = g - w[k] * sigma[k] ** 2 / omega.ravel() ** 2 * lambd.ravel()
            g_lambd[:, s] += g
            g_w[k, s] = I_k
        Q = bilin[s](Z)
        for k in range(K):
            for j in range(k + 1):
                tjk = np.sqrt((sigma[j] ** 2 + sigma[k] ** 2) * lambd**2 + ell**2)
                djk = (mu[:, j : j + 1] - mu[:, k : k + 1]) / tjk
                J = np.exp(ln_sf2 + sum_lnell - np.sum(np.log(tjk)) - np.sum(djk**2) / 2) - Q[k, j]
                J_sjk[s, j, k] = J_sjk[s, k, j] = J
                varG[s] += w[k] ** 2 * max(tiny, J) if j == k else 2 * w[j] * w[k] * J
    varG = np.maximum(varG, tiny)
    ee = np.exp(eta)
    es = ee.sum()
    Jw = -np.outer(ee, ee) / es**2 + np.diag(ee) / es
    Gbar = G.sum() / S
    vss = np.sum((G - Gbar) ** 2) / (S - 1)
    sd = np.sqrt(np.sum((varG - varG.sum() / S) ** 2) / (S - 1))
    return dict(G_s=G, G=Gbar, I_sk=I_sk, J_sjk=J_sjk, varG=np.sum(varG) / S + vss, var_ss=vss + sd,
                dG_mu=g_mu.reshape((D * K, S), order="F").sum(axis=1) / S,
                dG_sigma=(g_sigma * sigma.reshape(-1, 1)).sum(axis=1) / S,
                dG_lambd=(g_lambd * lambd).sum(axis=1) / S, dG_w=(Jw @ g_w).sum(axis=1) / S)


# ---- the truth ----------------------------------------------------------------------------------------------------
class _Solver:
    """C^-1 b in long double for C = K + sn2 I = sl A, through the factor of A = K / sl + I; ``refine``: with one step
    of iterative refinement."""

    def __init__(self, h, X, refine):
        N, D = X.shape
        self.sl = np.exp(2 * h[D + 1])
        K = _se(h[: D + 1], X, X)
        self.C = K + self.sl * np.eye(N, dtype=LD)
        self.Ui = glh.upper_inverse(glh.cholesky_upper(K / self.sl + np.eye(N, dtype=LD)))
        self.refine = refine

    def raw(self, b):
        return (self.Ui @ (self.Ui.T @ b)) / self.sl

    def __call__(self, b):
        x = self.raw(b)
        return x + self.raw(b - self.C @ x) if self.refine else x


def _evaluate_ld(kind, X, y, hyp, xs, mix, refine):
    Xl, yl, hl, xl = (np.asarray(a, dtype=np.float64).astype(LD) for a in (X, np.ravel(y), hyp, xs))
    D = X.shape[1]
    solvers = [_Solver(h, Xl, refine) for h in hl]
    alpha = np.stack([sv(yl - _mean(kind, h[D + 2 :], Xl)) for sv, h in zip(solvers, hl)])
    out = dict(alpha=alpha)
    out.update(_predict(kind, Xl, hl, xl, alpha, [lambda Ks, sv=sv: np.sum(Ks * sv(Ks), axis=0) for sv in solvers]))
    if mix is not None:
        out.update(_log_joint(kind, Xl, hl, mix, alpha, [lambda Z, sv=sv: Z @ sv(Z.T) for sv in solvers]))
    return out


def err(a, b, key):
    """Largest |a - b| of a quantity, in long double: per sample (S,) for the keys with a sample axis, else a scalar."""
    d = np.abs(np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD))
    if key in PER_SAMPLE:
        d = np.moveaxis(d, 1, 0) if key in ("mu", "s2") else d
        return np.max(d.reshape(d.shape[0], -1), axis=1).astype(np.float64)
    return float(np.max(d))


@lru_cache(maxsize=None)
def _plain(name):
    """The long-double values without the refinement step."""
    require_extended()
    d = data(name)
    return _evaluate_ld(BY_NAME[name].mean, d["X"], d["y"], d["hyp"], d["xs"], d["mix"], False)


@lru_cache(maxsize=None)
def truth(name):
    """The refined long-double values of every quantity of a case, and under "corr" what the refinement step changed."""
    require_extended()
    d = data(name)
    t = _evaluate_ld(BY_NAME[name].mean, d["X"], d["y"], d["hyp"], d["xs"], d["mix"], True)
    plain = _plain(name)
    t["corr"] = {k: err(plain[k], t[k], k) for k in list(t)}
    return t


@lru_cache(maxsize=None)
def truth_predict(name, M):
    """predict at the first M query points (the averaged pair depends on nothing else, so this is a view of truth)."""
    t = truth(name)
    out = {k: t[k][:M] for k in PREDICT_KEYS}
    plain = _plain(name)
    out["corr"] = {k: err(plain[k][:M], out[k], k) for k in PREDICT_KEYS}
    return out


# ---- the two float64 evaluations ----------------------------------------------------------------------------------
def _route_a(kind, X, y, hyp, xs, mix):
    """oracle/gp_ref: triangular solves."""
    ogp = gp_ref.make_gp(X, y, hyp, kind)
    out = dict(alpha=np.stack([p.alpha.ravel() for p in ogp.posteriors]))
    out["mu"], out["s2"] = gp_ref.predict(ogp, xs, separate_samples=True)
    a, b = gp_ref.predict(ogp, xs)
    out["mu_avg"], out["s2_avg"] = a.ravel(), b.ravel()
    if mix is not None:
        D, K = mix.D, mix.K
        _, dG, _, _, _ = gp_ref.gp_log_joint(mix, ogp, True, True, True, False, False)
        out["G_s"] = gp_ref.gp_log_joint(mix, ogp, False, False, True, False, False)[0]
        G, _, varG, _, var_ss, I_sk, J_sjk = gp_ref.gp_log_joint(mix, ogp, False, True, True, True, True)
        out.update(G=G, varG=varG, var_ss=var_ss, I_sk=I_sk, J_sjk=J_sjk)
        out.update(split_dG(dG, D, K))
    return out


def _route_b(kind, X, y, hyp, xs, mix):
    """Float64 NumPy by the device's route: explicit L^-1 (gp_post_host.posterior), V = L^-T k*, Z L^-1 and a Gram
    matrix; a non-Cholesky sample through the host record's L = -(K + sn2 I)^-1."""
    N, D = X.shape
    alpha, quad, bilin = [], [], []
    for h in hyp:
        if np.exp(2 * h[D + 1]) >= 1e-6:
            st = gph.posterior(h, X, y, kind)
            Li, sl = st["Linv"], st["sl"]
            alpha.append(st["alpha"])
            quad.append(lambda Ks, Li=Li, sl=sl: np.sum((Li.T @ (Ks / np.sqrt(sl))) ** 2, axis=0))
            bilin.append(lambda Z, Li=Li, sl=sl: (Z @ Li) @ (Z @ Li).T / sl)
        else:
            p = gp_ref.make_posterior(h, X, y, kind)
            assert not p.L_chol
            alpha.append(p.alpha.ravel())
            quad.append(lambda Ks, L=p.L: -np.sum(Ks.T * (Ks.T @ L), axis=1))
            bilin.append(lambda Z, L=p.L: -(Z @ (Z @ L).T))
    alpha = np.stack(alpha)
    out = dict(alpha=alpha)
    out.update(_predict(kind, X, hyp, xs, alpha, quad))
    if mix is not None:
        out.update(_log_joint(kind, X, hyp, mix, alpha, bilin))
    return out


def split_dG(dG, D, K):
    """The four blocks of a full averaged gradient vector [mu (D K) | sigma (K) | lambda (D) | w (K)]."""
    dG = np.ravel(dG)
    assert dG.size == D * K + K + D + K
    cuts = np.cumsum([D * K, K, D])
    return dict(zip(DG_BLOCKS, np.split(dG, cuts)))


@lru_cache(maxsize=None)
def _routes(name):
    c, d = BY_NAME[name], data(name)
    return {nm: route(c.mean, d["X"], d["y"], d["hyp"], d["xs"], d["mix"])
            for nm, route in (("oracle", _route_a), ("device_route", _route_b))}


@lru_cache(maxsize=None)
def e64(name, M=None):
    """Per quantity the larger error against the truth of the two float64 routes; both parts under "parts".  ``M``:
    predict's four quantities over the first M query points alone (against ``truth_predict(name, M)``)."""
    t = truth(name) if M is None else truth_predict(name, M)
    keys = [k for k in t if k != "corr"]
    cut = (lambda k, v: v[:M]) if M is not None else (lambda k, v: v)
    parts = {nm: {k: err(cut(k, r[k]), t[k], k) for k in keys} for nm, r in _routes(name).items()}
    e = {k: np.maximum(parts["oracle"][k], parts["device_route"][k]) for k in keys}
    e["parts"] = parts
    return e


@lru_cache(maxsize=None)
def factor_truth(name):
    """Per sample the long-double upper Cholesky factor of A = K / sl + I (float64 inputs), or None for a sample on the
    non-Cholesky branch: what the device-built records' ``L`` is compared with."""
    require_extended()
    d = data(name)
    X = d["X"].astype(LD)
    N, D = X.shape
    out = []
    for h in d["hyp"].astype(LD):
        sl = np.exp(2 * h[D + 1])
        out.append(glh.cholesky_upper(_se(h[: D + 1], X, X) / sl + np.eye(N, dtype=LD)) if sl >= 1e-6 else None)
    return out


@lru_cache(maxsize=None)
def lml_reference(name):
    """(refs, factors) of gp_lml_host.check_within for the samples of a Cholesky case: the long-double log marginal
    likelihood and gradient, and f = 4 N eps cond2(A)."""
    require_extended()
    c, d = BY_NAME[name], data(name)
    refs = [glh.lml_and_grad(h, d["X"], d["y"], c.mean, dtype=LD) for h in d["hyp"]]
    return refs, [glh.factor_of(h, d["X"]) for h in d["hyp"]]


# ---- the bound ----------------------------------------------------------------------------------------------------
def sf2_of(hyp, D):
    return float(np.max(np.exp(2 * np.atleast_2d(hyp)[:, D])))


def project_bound(key, t, sf2):
    """B_q: the project's existing bound of a quantity (scalar)."""
    amax = lambda k: float(np.max(np.abs(t[k])))
    if key in ("mu", "mu_avg"):
        return 1e-10 * max(1.0, amax("mu"))
    if key in ("s2", "s2_avg", "J_sjk", "varG", "var_ss"):
        return 1e-10 * sf2
    if key in ("G", "G_s"):
        return 1e-10 * max(1.0, amax(key))
    if key == "I_sk":
        return 1e-10 * amax("I_sk")
    if key in DG_BLOCKS:
        return 1e-9 * amax(key)
    raise KeyError(key)


def check(key, dev, t, e, sf2, what, rel_to=None):
    """Assert |dev - truth| <= max(B_q, 8 e64_q), per sample where the quantity has a sample axis.  Prints one table row
    ``| what | quantity | e64 oracle | e64 device route | device error | share of the tolerance |`` (per-sample figures
    joined by "/"); ``rel_to``: a last column, the error relative to this (the smallest true variance for s2)."""
    d = np.atleast_1d(err(dev, t[key], key))
    tol = np.maximum(project_bound(key, t, sf2), 8.0 * np.atleast_1d(e[key]))
    pa, pb = (np.atleast_1d(e["parts"][r][key]) for r in ("oracle", "device_route"))
    fmt = lambda v: " / ".join(f"{x:.1e}" for x in np.atleast_1d(v))
    tail = "" if rel_to is None else f" {fmt(d / np.atleast_1d(rel_to))} |"
    print(f"| {what} | {key} | {fmt(pa)} | {fmt(pb)} | {fmt(d)} | {fmt(d / tol)} |{tail}")
    assert np.all(d <= tol), (what, key, d, tol)
    return d / tol
