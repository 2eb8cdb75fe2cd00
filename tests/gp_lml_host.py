"""NumPy restatement of the GP log marginal likelihood and its gradient (pyvbmc_amd.gp.log_marginal_likelihood,
csrc/gp_lml.hip), in float64 or ``np.longdouble``.  TEST INFRASTRUCTURE: gpyreg is not part of the reference tree, so the
yardstick is the textbook formula in the conventions of oracle/gp_ref.py (``se_ard``, ``mean_fn``, ``noise_var``;
hyp = [log ell (D) | log sf | log sn | mean]).  The Cholesky factorisation and the triangular inverse are written out,
so that they run in longdouble.

Per candidate, with sn2_div = min sn2, sl = sn2_div, C = K + diag(sn2) = sl A, U^T U = A, r = y - m(X), alpha = C^-1 r:
    lml        = -1/2 r.alpha - sum_i log U_ii - N/2 log(2 pi sl)
    W          = A^-1 / sl - alpha alpha^T
    d/dlog ell_d = -1/2 sum_ij W_ij K_ij (x_id - x_jd)^2 / ell_d^2
    d/dlog sf    = -sum_ij W_ij K_ij
    d/dlog sn    = -1/2 dsn2 tr W,   dsn2 = 2 exp(2 hyp_noise)  (gp_ref.noise_var: constant additive noise)
    d/dtheta_m   = alpha . dm/dtheta_m

Bounds (derived): with f = 4 N eps cond2(A) (gp_post_host.forward_factor, the project's bound for L and alpha) every U_ii
carries relative error f, hence N f on the log sum, and the products carry f times their absolute terms:
    |d lml| <= f vabs,        vabs   = 1/2 |r| |alpha| + N
    |d grad_th| <= f gabs_th, gabs_th = 1/2 sum_ij (|A^-1_ij| / sl + |alpha_i alpha_j|) |dC_ij/dth|,  sum_n |alpha_n| |dm_n/dth|.
"""
from functools import lru_cache

import numpy as np

import gp_post_host as gph
from oracle import gp_ref

# (N, D, S, mean) of gph.make_case(N, D, S, mean, seed=100 + N) the bounds were checked on
CASES = [
    (63, 3, 2, gp_ref.MEAN_CONST),
    (65, 3, 2, gp_ref.MEAN_NEGQUAD),
    (130, 10, 3, gp_ref.MEAN_NEGQUAD),
    (257, 20, 2, gp_ref.MEAN_NEGQUAD),
    (65, 32, 2, gp_ref.MEAN_NEGQUAD),  # D = DMX: the gradient tile's coordinate panels at their full height
    (130, 13, 2, gp_ref.MEAN_CONST),  # an odd D between the workload's two
]


def cholesky_upper(A):
    """U^T U = A, row by row, in A's dtype; LinAlgError on a pivot that is not a positive finite number."""
    a = np.array(A)
    n = a.shape[0]
    U = np.zeros_like(a)
    for k in range(n):
        p = a[k, k]
        if not (p > 0 and np.isfinite(p)):
            raise np.linalg.LinAlgError("pivot %d is not a positive finite number" % k)
        ukk = np.sqrt(p)
        row = a[k, k:] / ukk
        row[0] = ukk
        U[k, k:] = row
        a[k + 1 :, k + 1 :] -= np.outer(row[1:], row[1:])
    return U


def upper_inverse(U):
    """U^-1 by back substitution, in U's dtype."""
    n = U.shape[0]
    X = np.eye(n, dtype=U.dtype)
    for r in range(n - 1, -1, -1):
        X[r, :] = X[r, :] / U[r, r]
        X[:r, :] -= U[:r, r : r + 1] * X[r : r + 1, :]
    return np.triu(X)


def mean_and_grad(mean_kind, hm, X):
    """m(X) (N) and dm/dtheta (mean parameters, N), in X's dtype."""
    N, D = X.shape
    one = np.ones((1, N), dtype=X.dtype)
    if mean_kind == gp_ref.MEAN_ZERO:
        return np.zeros(N, dtype=X.dtype), np.zeros((0, N), dtype=X.dtype)
    if mean_kind == gp_ref.MEAN_CONST:
        return hm[0] * one[0], one
    om = np.exp(hm[1 + D : 1 + 2 * D])
    u = X - hm[1 : 1 + D]
    m = hm[0] - np.sum((u / om) ** 2, axis=1) / 2
    return m, np.vstack([one, (u / om**2).T, ((u / om) ** 2).T])


def lml_and_grad(hyp, X, y, mean_kind, s2=None, noise_user=False, dtype=np.float64):
    """dict(lml, grad (P), vabs, gabs (P)) of one candidate in ``dtype``."""
    N, D = X.shape
    h = np.asarray(hyp, dtype=np.float64).astype(dtype)
    X = np.asarray(X, dtype=np.float64).astype(dtype)
    y = np.ravel(np.asarray(y, dtype=np.float64)).astype(dtype)
    sn2 = np.full(N, np.exp(2 * h[D + 1]))
    if noise_user and s2 is not None:
        sn2 = sn2 + np.ravel(np.asarray(s2, dtype=np.float64)).astype(dtype)
    sn2_div = np.min(sn2)
    sl = sn2_div
    dsn2 = 2 * np.exp(2 * h[D + 1])
    Xs = X / np.exp(h[:D])
    T2 = (Xs[:, None, :] - Xs[None, :, :]) ** 2  # (N, N, D): t_d^2, direct differences as gp_ref.se_ard
    K = np.exp(2 * h[D]) * np.exp(-np.sum(T2, axis=2) / 2)
    A = K / sl + np.diag(sn2 / sn2_div)
    m, dm = mean_and_grad(mean_kind, h[D + 2 :], X)
    r = y - m
    U = cholesky_upper(A)
    Ui = upper_inverse(U)
    Ainv = Ui @ Ui.T
    alpha = (Ainv @ r) / sl
    pi = np.arccos(dtype(-1))
    lml = -(r @ alpha) / 2 - np.sum(np.log(np.diag(U))) - N * np.log(2 * pi * sl) / 2
    W = Ainv / sl - np.outer(alpha, alpha)
    Wabs = np.abs(Ainv) / sl + np.abs(np.outer(alpha, alpha))
    P = h.size
    grad, gabs = np.zeros(P, dtype=dtype), np.zeros(P, dtype=dtype)
    for d in range(D):
        grad[d] = -np.sum(W * K * T2[:, :, d]) / 2
        gabs[d] = np.sum(Wabs * K * T2[:, :, d]) / 2
    grad[D] = -np.sum(W * K)
    gabs[D] = np.sum(Wabs * K)  # (dC/dlog sf = 2 K)
    grad[D + 1] = -dsn2 * np.trace(W) / 2
    gabs[D + 1] = dsn2 * np.trace(Wabs) / 2
    grad[D + 2 :] = dm @ alpha
    gabs[D + 2 :] = np.abs(dm) @ np.abs(alpha)
    vabs = np.sqrt(r @ r) * np.sqrt(alpha @ alpha) / 2 + N
    return dict(lml=lml, grad=grad, vabs=vabs, gabs=gabs)


def factor_of(hyp, X, s2=None, noise_user=False):
    """f = 4 N eps cond2(A) of one candidate (gp_post_host.forward_factor)."""
    N, D = X.shape
    hyp = np.asarray(hyp, dtype=np.float64)
    sn2, sn2_div, sl = gph.noise_scalars(hyp, N, D, s2, noise_user)
    return gph.forward_factor(gph.cov_matrix(hyp, X, sn2, sn2_div, sl))


@lru_cache(maxsize=None)
def reference(N, D, S, mean_kind, with_s2=False):
    """Data of gph.make_case(N, D, S, mean, seed=100 + N) (user noise s2 when asked for), the longdouble restatement and
    the factor f of every candidate, computed once per case: (X, y, hyp, s2, refs, factors)."""
    X, y, hyp = gph.make_case(N, D, S, mean_kind, seed=100 + N)
    s2 = 0.01 + 0.02 * np.random.default_rng(N).random((N, 1)) if with_s2 else None
    refs = [lml_and_grad(h, X, y, mean_kind, s2, with_s2, np.longdouble) for h in hyp]
    return X, y, hyp, s2, refs, [factor_of(h, X, s2, with_s2) for h in hyp]


def check_within(lml, grad, ref, f, what):
    """Assert |lml - ref| <= f vabs and |grad - ref| <= f gabs per parameter; prints and returns the used fractions."""
    dv = abs(float(lml - ref["lml"]))
    bv = f * float(ref["vabs"])
    dg = np.abs(np.asarray(grad, dtype=np.longdouble) - ref["grad"]).astype(np.float64)
    bg = f * ref["gabs"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bg > 0, dg / bg, np.where(dg == 0, 0.0, np.inf))
    print(f"{what}: f {f:.2e}, value uses {dv / bv:.2e} of its bound, gradient at most {np.max(frac):.2e} "
          f"(parameter {int(np.argmax(frac))})")
    assert dv <= bv, (what, dv, bv)
    assert np.all(dg <= bg), (what, dg, bg)
    return dv / bv, float(np.max(frac))
