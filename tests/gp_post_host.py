"""NumPy restatement of the device-built GP posterior (pyvbmc_amd/csrc/gp_post.hip): the blocked upper Cholesky with
its explicit diagonal-block inverses, L^-1, alpha, and the one-point append.  TEST INFRASTRUCTURE: it plays the role of
ais_host.py / mode_host.py / kde_host.py -- the same algorithm as the kernels in plain NumPy, pinned against
oracle/gp_ref.make_posterior on the CPU (tests/test_gp_post_host.py) and compared with the device on the GPU
(tests/test_gp_post_gpu.py).

Blocks are 64 x 64 on the block grid of the kernels; the matrix is padded with the identity to whole blocks.  Per block
step j: factor the diagonal block (right-looking, row by row), invert the factor by back substitution, panel
U_j,rest = Dinv_j^T A_j,rest, trailing update A_ab -= U_ja^T U_jb on and above the diagonal.  What differs from the
device is the rounding inside the products only (the device fuses multiply-adds and sums a product's terms in the
matrix instruction's order).
"""
import numpy as np

from oracle import gp_ref

PB = 64


def noise_scalars(hyp, N, D, s2=None, noise_user=False):
    """sn2 (N), sn2_div, sl for one sample, with the arithmetic of gp.py / gp_ref.make_posterior."""
    sn2 = gp_ref.noise_var(hyp[D + 1 : D + 2], N, s2, noise_user)
    sn2_div = np.min(sn2)
    return sn2, sn2_div, sn2_div * 1.0


def cov_matrix(hyp, X, sn2, sn2_div, sl):
    """Upper triangle (diagonal included) of A = K / sl + diag(sn2 / sn2_div), zeros below."""
    D = X.shape[1]
    K = gp_ref.se_ard(hyp[: D + 1], X, X)
    return np.triu(K / sl + np.diag(sn2 / sn2_div))


def chol_diag(B):
    """U^T U = B for one 64 x 64 block (upper triangle of B read): right-looking, as chol_diag_kernel."""
    a = np.array(B, dtype=np.float64)
    n = a.shape[0]
    U = np.zeros_like(a)
    for k in range(n):
        p = a[k, k]
        if not (p > 0.0 and np.isfinite(p)):
            raise np.linalg.LinAlgError("pivot %d is not a positive finite number" % k)
        ukk = np.sqrt(p)
        row = a[k, k:] / ukk
        row[0] = ukk
        U[k, k:] = row
        for i in range(k + 1, n):
            a[i, i:] -= row[i - k] * row[i - k :]
    return U


def tri_inverse(U):
    """U^-1 by the back substitution of trinv_diag_kernel / chol_dinv_kernel: column c, rows 63 .. 0."""
    n = U.shape[0]
    rinv = 1.0 / np.diag(U)
    X = np.eye(n)
    for r in range(n - 1, -1, -1):
        X[r, :] = X[r, :] * rinv[r]
        X[:r, :] -= U[:r, r : r + 1] * X[r : r + 1, :]
    return np.triu(X)


def blocked_cholesky(A):
    """(U, Dinv): U^T U = A (A's upper triangle read) by 64 x 64 block steps; Dinv[j] = the inverse of diagonal block j."""
    N = A.shape[0]
    nb = (N + PB - 1) // PB
    Np = nb * PB
    W = np.eye(Np)
    W[:N, :N] = np.triu(A)
    Dinv = np.zeros((nb, PB, PB))
    for j in range(nb):
        r = slice(j * PB, (j + 1) * PB)
        W[r, r] = chol_diag(W[r, r])
        Dinv[j] = tri_inverse(W[r, r])
        for c in range(j + 1, nb):
            cs = slice(c * PB, (c + 1) * PB)
            W[r, cs] = Dinv[j].T @ W[r, cs]
        for a in range(j + 1, nb):
            as_ = slice(a * PB, (a + 1) * PB)
            for b in range(a, nb):
                bs = slice(b * PB, (b + 1) * PB)
                upd = W[r, as_].T @ W[r, bs]
                W[as_, bs] -= np.triu(upd) if a == b else upd
    return np.triu(W[:N, :N]), Dinv


def upper_inverse(U, Dinv):
    """U^-1 block row by block row, X_i = Dinv_i (E_i - sum_{m > i} U_im X_m): launch_trinv's second stage."""
    N = U.shape[0]
    nb = Dinv.shape[0]
    Np = nb * PB
    W = np.eye(Np)
    W[:N, :N] = U
    X = np.zeros((Np, Np))
    for i in range(nb - 1, -1, -1):
        r = slice(i * PB, (i + 1) * PB)
        R = np.eye(Np)[r, :] - W[r, (i + 1) * PB :] @ X[(i + 1) * PB :, :]
        X[r, :] = Dinv[i] @ R
    return np.triu(X[:N, :N])


def alpha_from(Uinv, r, sl):
    return (Uinv @ (Uinv.T @ r)) / sl


def posterior(hyp, X, y, mean_kind, s2=None, noise_user=False):
    """dict(A, L, Linv, alpha, r, sW, sl, sn2) of one sample by the device's algorithm."""
    N, D = X.shape
    hyp = np.asarray(hyp, dtype=np.float64)
    sn2, sn2_div, sl = noise_scalars(hyp, N, D, s2, noise_user)
    A = cov_matrix(hyp, X, sn2, sn2_div, sl)
    L, Dinv = blocked_cholesky(A)
    Linv = upper_inverse(L, Dinv)
    r = np.ravel(y) - gp_ref.mean_fn(mean_kind, hyp[D + 2 :], X)
    return dict(A=A, L=L, Linv=Linv, alpha=alpha_from(Linv, r, sl), r=r, sW=np.ones(N) / np.sqrt(sl), sl=sl, sn2=sn2)


def append(st, hyp, X, x, y, mean_kind):
    """The state ``st`` of N points X extended by (x, y) under constant noise: the gp_append_* formulas."""
    D = X.shape[1]
    hyp = np.asarray(hyp, dtype=np.float64)
    sl = st["sl"]
    k = gp_ref.se_ard(hyp[: D + 1], X, x[None, :]).ravel() / sl
    l = st["Linv"].T @ k
    d2 = np.exp(2 * hyp[D]) / sl + st["sn2"][0] / sl - l @ l
    if not (d2 > 0.0 and np.isfinite(d2)):
        raise np.linalg.LinAlgError("appended point: d^2 is not positive and finite")
    d = np.sqrt(d2)
    N = X.shape[0]
    L = np.zeros((N + 1, N + 1))
    L[:N, :N], L[:N, N], L[N, N] = st["L"], l, d
    Linv = np.zeros((N + 1, N + 1))
    Linv[:N, :N], Linv[:N, N], Linv[N, N] = st["Linv"], (st["Linv"] @ l) / -d, 1.0 / d
    r = np.append(st["r"], y - gp_ref.mean_fn(mean_kind, hyp[D + 2 :], x[None, :])[0])
    return dict(L=L, Linv=Linv, alpha=alpha_from(Linv, r, sl), r=r, sW=np.ones(N + 1) / np.sqrt(sl), sl=sl,
                sn2=np.append(st["sn2"], st["sn2"][0]))


# ---- shared test data ---------------------------------------------------------------------------------------------
EPS = np.finfo(np.float64).eps


def make_case(N, D, S, mean_kind, seed, well=True):
    """Seeded training data and S hyper-parameter samples.  ``well``: length scales 0.8 sqrt(D) against points of spread
    2 and noise sn ~ 0.3 sf: the off-diagonal blocks of the factor reach 0.3 - 0.6 of its largest entry while cond2(A)
    stays between 6 and ~200, so an indexing error in a panel or a trailing update can hide neither behind conditioning
    nor behind a nearly diagonal matrix; otherwise long length scales and sn ~ 5e-3."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)) * 2.0
    y = -0.5 * np.sum(X**2, axis=1) / D + 0.3 * rng.standard_normal(N)  # (noise: r != 0 under every mean)
    P = D + 2 + gp_ref.mean_n(mean_kind, D)
    hyp = np.zeros((S, P))
    for s in range(S):
        ell = (0.8 * np.sqrt(D) if well else 3.0) * (1 + 0.2 * rng.random(D))
        hyp[s, :D] = np.log(ell)
        hyp[s, D] = np.log(1.0 + 0.3 * rng.random())
        hyp[s, D + 1] = np.log((0.3 if well else 5e-3) * (1 + 0.2 * rng.random()))
        if mean_kind != gp_ref.MEAN_ZERO:
            hyp[s, D + 2] = 0.2 * rng.standard_normal()
        if mean_kind == gp_ref.MEAN_NEGQUAD:
            hyp[s, D + 3 : 2 * D + 3] = 0.1 * rng.standard_normal(D)
            hyp[s, 2 * D + 3 :] = np.log(2.0 + rng.random(D))
    return X, y.reshape(-1, 1), hyp


def residual_bound(A):
    """max |U^T U - A| allowed: (N + 2) eps max_i a_ii, from |U^T U - A|_ij <= gamma_{N+1} sqrt(a_ii a_jj)."""
    return (A.shape[0] + 2) * EPS * np.max(np.diag(A))


def forward_factor(A):
    """4 N eps cond2(A): the forward-error law of a Cholesky solve, relative to max |L| resp. max |alpha|."""
    Af = np.triu(A) + np.triu(A, 1).T
    return 4 * A.shape[0] * EPS * np.linalg.cond(Af)


def check_factor(L, A):
    """Residual bound and exact zeros below the diagonal; returns the residual as a fraction of the bound."""
    Af = np.triu(A) + np.triu(A, 1).T
    assert np.all(np.tril(L, -1) == 0.0)
    res = float(np.max(np.abs(L.T @ L - Af)))
    assert res <= residual_bound(A), (res, residual_bound(A))
    return res / residual_bound(A)
