"""A NumPy restatement of ``VariationalPosterior.mode`` as this package computes it (csrc/mode.hip), plus the
case table and parameter recipes of tests/golden/mode.npz (tools/make_mode_golden.py imports the same
recipes, so the fixture stores the reference's results and the transformer fields only).

The reference (variational_posterior.py:810-919) runs ``n_opts`` rounds: draw 1e5 samples, append the
component centres in round 0, start SciPy's ``minimize`` of ``-log pdf`` from the best of them, keep the best
round.  Here the start selection is the same and the local search is a monotone ascent in the SEARCH
COORDINATES y:

    transformed space   y = u, the objective is log q(u)
    original space      y_d = x_d on an unbounded dimension, g_d(x_d) (the uncentred bounded transform) on a
                        bounded one, kept in [g(lb + sqrt(eps)), g(ub - sqrt(eps))] (the reference's L-BFGS-B
                        box, :888-898); u = ((y - mu) / delta) @ R / scale is affine in y and the objective is
                        log q(u(y)) - sum_d (const_d + lj_d(y_d)), what pdf(x(y), True, log_flag=True) returns
                        when R is orthogonal (log_abs_det_jacobian forms its argument as u * scale @ R^T)

with analytic gradient and Hessian from the responsibilities r_k:

    grad_u = -sum_k r_k (u - mu_k) / (lambda^2 sigma_k^2)
    hess_u = -diag(sum_k r_k / (lambda^2 sigma_k^2)) + sum_k r_k g_k g_k^T - grad_u grad_u^T,   g_k the k-th term
    grad_y = J grad_u - lj'(y),   hess_y = J hess_u J^T - diag(lj''(y)),   J = du/dy (D x D)

One iteration: the free set drops the dimensions that sit on a bound with the gradient pointing outward; a
Newton step on the free set is tried when the Hessian there is negative definite (Cholesky of its negative),
clipped to the box, and accepted when it does not lower the objective; otherwise a step with guaranteed ascent
is taken -- the mean-shift fixed point sum_k a_k mu_k / sum_k a_k (a_k = r_k / sigma_k^2) in the transformed
space, a projected-gradient step with backtracking in the original space.  "Does not lower" allows for the
rounding of one evaluation, SLACK * max(1, |f|): next to the maximum the Newton step's gain is below that
rounding, and without the allowance the search would stop a few 1e-8 short of the stationary point.  The
search stops when an accepted step is <= 1e-12 max(1, |y|_inf), when no step is accepted, or at the cap.
"""
import sys
from pathlib import Path

import numpy as np

import kde_host
from transform_host import _TABLE, RefShapedTransformer

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import mixture_ref  # noqa: E402

# name -> (D, K, transformer kind, seed, overlap recipe)
CASES = {
    "d1": (1, 2, "identity", 1, False),
    "d2_bounded": (2, 3, "bounded", 3, False),
    "d10": (10, 50, "identity", 4, False),
    "d10_bounded": (10, 5, "bounded", 6, False),
    "d10_roto": (10, 5, "roto", 7, False),
    "d20": (20, 100, "identity", 11, False),
    "d32_roto": (32, 4, "roto", 8, False),
    "d6_overlap": (6, 30, "identity", 21, True),
}
SEEDS = (100, 101, 102, 103)  # np.random.seed before each reference run
N_SAMPLES = int(1e5)
STEP_TOL = 1e-12
MAX_ITER = 200
SLACK = 64 * np.finfo(np.float64).eps
CONVERGED, ON_BOUND, ITER_CAP = 0, 1, 2
SQRT_EPS = np.sqrt(np.finfo(np.float64).eps)


def case_mixture(name):
    """mu (D x K), sigma (1 x K), lambd (D x 1), w (1 x K) of case ``name``."""
    D, K, _, seed, overlap = CASES[name]
    mu, sigma, lambd, w = kde_host.mixture_params(D, K, seed)
    if overlap:
        mu = mu * 0.3  # components closer than their widths: the modes are not the centres
    return mu, sigma, lambd, w


def rotoscale(D, seed):
    """The rotation and scale of a "roto" case."""
    r = np.random.RandomState(seed + 77)
    R, _ = np.linalg.qr(r.randn(D, D))
    return R, np.exp(r.randn(D) * 0.2)


def golden_transformer(g, name):
    """The case's transformer from the fixture's stored fields (None: identity)."""
    p = f"{name}_pt_"
    if int(g[p + "identity"]):
        return None
    R, s = g[p + "R"], g[p + "scale"]
    return RefShapedTransformer(g[p + "type"], g[p + "lb"], g[p + "ub"], g[p + "mu"], g[p + "delta"],
                                R if R.size else None, s if s.size else None)


def golden_vp(g, name, VariationalPosterior=None):
    """The package's posterior of case ``name`` (the global NumPy stream is left as it was)."""
    if VariationalPosterior is None:
        from pyvbmc_amd import VariationalPosterior
    D, K = CASES[name][:2]
    state = np.random.get_state()
    vp = VariationalPosterior(D, K, parameter_transformer=golden_transformer(g, name))
    np.random.set_state(state)
    vp.mu, vp.sigma, vp.lambd, vp.w = case_mixture(name)
    return vp


# ---- the objective ---------------------------------------------------------------------------------------------

_LJ1 = {  # d lj / dy
    3: lambda y: -np.tanh(0.5 * y),
    12: lambda y: -y,
    13: lambda y: -1.25 * y / (1 + y * y / 4),
}
_LJ2 = {  # d^2 lj / dy^2
    3: lambda y: -0.5 / np.cosh(0.5 * y) ** 2,
    12: lambda y: -np.ones_like(y),
    13: lambda y: -1.25 * (1 - y * y / 4) / (1 + y * y / 4) ** 2,
}


class Objective:
    """log density in the search coordinates; ``pt`` None or a reference-shaped transformer."""

    def __init__(self, mu, sigma, lambd, w, pt=None, orig_flag=False):
        self.mu = np.asarray(mu, dtype=np.float64)  # D x K
        self.D, self.K = self.mu.shape
        self.sigma = np.ravel(sigma).astype(np.float64)
        self.lam = np.ravel(lambd).astype(np.float64)
        self.w = np.ravel(w).astype(np.float64)
        self.orig = bool(orig_flag) and pt is not None
        self.pt = pt
        D = self.D
        self.logc = (np.log(self.w) - D * np.log(self.sigma) - 0.5 * D * np.log(2 * np.pi)
                     - np.sum(np.log(self.lam)))
        self.lo = np.full(D, -np.inf)
        self.hi = np.full(D, np.inf)
        self.J = np.eye(D)
        self.type = np.zeros(D, dtype=int)
        self.const = 0.0
        if self.orig:
            self.type = np.ravel(pt.type).astype(int)
            lb, ub = np.ravel(pt.lb_orig), np.ravel(pt.ub_orig)
            self.lb, self.ub = lb, ub
            R = np.eye(D) if pt.R_mat is None else pt.R_mat
            sc = np.ones(D) if pt.scale is None else np.ravel(pt.scale)
            self.J = R / np.ravel(pt.delta)[:, None] / sc[None, :]  # J[i, j] = du_j / dy_i
            self.const = np.sum(np.log(np.ravel(pt.delta))) + np.sum(np.log(sc))
            for d in np.flatnonzero(self.type):
                self.lo[d] = self._g(d, lb[d] + SQRT_EPS)
                self.hi[d] = self._g(d, ub[d] - SQRT_EPS)
                self.const += np.log(ub[d] - lb[d])

    def _g(self, d, x):
        z = (x - self.lb[d]) / (self.ub[d] - self.lb[d])
        return float(_TABLE[self.type[d]][0](np.array([z]))[0])

    def y_from_x(self, x):
        """Original-space point -> search coordinates, clipped to the box."""
        y = np.array(x, dtype=np.float64)
        if self.orig:
            for d in np.flatnonzero(self.type):
                xd = min(max(y[d], self.lb[d]), self.ub[d])
                y[d] = self._g(d, xd)
        return np.minimum(np.maximum(y, self.lo), self.hi)

    def x_from_y(self, y):
        x = np.array(y, dtype=np.float64)
        if self.orig:
            for d in np.flatnonzero(self.type):
                z = _TABLE[self.type[d]][1](np.array([y[d]]))[0]
                x[d] = z * (self.ub[d] - self.lb[d]) + self.lb[d]
                x[d] = min(max(x[d], self.lb[d] + SQRT_EPS), self.ub[d] - SQRT_EPS)
        return x

    def u_of(self, y):
        if not self.orig:
            return np.asarray(y, dtype=np.float64)
        return (y - np.ravel(self.pt.mu)) @ self.J

    def full(self, y):
        """(f, grad, hess, mean-shift point) at y."""
        u = self.u_of(y)
        diff = (u[:, None] - self.mu) / self.lam[:, None]            # D x K, lambda-scaled
        is2 = 1.0 / self.sigma**2
        l = self.logc - 0.5 * is2 * np.sum(diff**2, axis=0)
        m = np.max(l)
        p = np.exp(l - m)
        S = np.sum(p)
        f = m + np.log(S)
        r = p / S
        a = r * is2
        gk = -(diff * is2) / self.lam[:, None]                         # D x K, component log-gradients
        gu = gk @ r
        Hu = -np.diag(np.sum(a) / self.lam**2) + (gk * r) @ gk.T - np.outer(gu, gu)
        ms = (self.mu @ a) / np.sum(a)
        g = self.J @ gu
        H = self.J @ Hu @ self.J.T
        if self.orig:
            f -= self.const
            for d in np.flatnonzero(self.type):
                yd = np.array([y[d]])
                f -= _TABLE[self.type[d]][2](yd)[0]
                g[d] -= _LJ1[self.type[d]](yd)[0]
                H[d, d] -= _LJ2[self.type[d]](yd)[0]
        return f, g, H, ms

    def value(self, y):
        return self.full(y)[0]

    def free_set(self, y, g):
        return ~(((y <= self.lo) & (g < 0)) | ((y >= self.hi) & (g > 0)))


def search(obj, y0, max_iter=MAX_ITER, tol=STEP_TOL):
    """The local ascent from y0: ``(y, f, iterations, status)``."""
    clip = lambda v: np.minimum(np.maximum(v, obj.lo), obj.hi)  # noqa: E731
    y = clip(np.array(y0, dtype=np.float64))
    f, g, H, ms = obj.full(y)
    status, it = ITER_CAP, 0
    while it < max_iter:
        it += 1
        free = obj.free_set(y, g)
        slack = SLACK * max(1.0, abs(f))
        accepted = None
        if np.any(free):
            Hf = -H[np.ix_(free, free)]
            try:
                L = np.linalg.cholesky(Hf)
                p = np.zeros(obj.D)
                p[free] = np.linalg.solve(L.T, np.linalg.solve(L, g[free]))
                yt = clip(y + p)
                ev = obj.full(yt)
                if ev[0] >= f - slack:
                    accepted = (yt, ev)
            except np.linalg.LinAlgError:
                pass
        if accepted is None and not obj.orig:
            ev = obj.full(ms)
            if ev[0] >= f - slack:
                accepted = (ms, ev)
        if accepted is None and obj.orig and np.any(free):
            gm = np.where(free, g, 0.0)
            s = 1.0 / max(np.max(np.sum(np.abs(H), axis=1)), 1e-300)
            for _ in range(30):
                yt = clip(y + s * gm)
                ev = obj.full(yt)
                if ev[0] >= f and np.any(yt != y):
                    accepted = (yt, ev)
                    break
                s *= 0.25
        if accepted is None:
            status = CONVERGED
            break
        yt, (ft, gt, Ht, mst) = accepted
        step = np.max(np.abs(yt - y))
        y, f, g, H, ms = yt, ft, gt, Ht, mst
        if step <= tol * max(1.0, np.max(np.abs(y))):
            status = CONVERGED
            break
    if status == CONVERGED and np.any((y <= obj.lo) | (y >= obj.hi)):
        status = ON_BOUND
    return y, f, it, status


# ---- host log-density and the whole method -----------------------------------------------------------------------


def host_log_pdf(mu, sigma, lambd, w, pt, x, orig_flag):
    """``pdf(x, orig_flag, log_flag=True)`` on the host: the oracle's mixture density around the host transformer."""
    mix = mixture_ref.Mixture.make(mu, np.ravel(sigma), np.ravel(lambd), np.ravel(w))
    x = np.array(np.atleast_2d(x), dtype=np.float64)
    if not orig_flag or pt is None:
        return mixture_ref.pdf(mix, x, log_flag=True).ravel()
    out = np.full(x.shape[0], -np.inf)
    mask = np.all(x > pt.lb_orig, axis=1) & np.all(x < pt.ub_orig, axis=1)
    if np.any(mask):
        u = pt(x[mask])
        out[mask] = mixture_ref.pdf(mix, u, log_flag=True).ravel() - pt.log_abs_det_jacobian(u)
    return out


def fast_log_pdf(mu, sigma, lambd, w, pt, x, orig_flag):
    """host_log_pdf with the squared distances expanded into one matrix product: for picking the start among 1e5
    candidates (its ~1e-13 rounding does not matter there), not for comparing values."""
    x = np.array(np.atleast_2d(x), dtype=np.float64)
    out = np.full(x.shape[0], -np.inf)
    mask, lj = np.full(x.shape[0], True), 0.0
    u = x
    if orig_flag and pt is not None:
        mask = np.all(x > pt.lb_orig, axis=1) & np.all(x < pt.ub_orig, axis=1)
        u = pt(x[mask])
        lj = pt.log_abs_det_jacobian(u)
    lam, sig = np.ravel(lambd), np.ravel(sigma)
    us, ms = u / lam, mu / lam[:, None]
    d2 = np.sum(us**2, axis=1)[:, None] - 2 * us @ ms + np.sum(ms**2, axis=0)[None, :]
    l = np.log(np.ravel(w)) - mu.shape[0] * np.log(sig) - 0.5 * d2 / sig**2
    m = np.max(l, axis=1)
    out[mask] = m + np.log(np.sum(np.exp(l - m[:, None]), axis=1)) - lj
    return out  # (up to the constant -D/2 log(2 pi) - sum log(lambda))


def draw_candidates(mu, sigma, lambd, w, pt, orig_flag, n_opts, n=N_SAMPLES):
    """The reference's start candidates from NumPy's global stream: ``sample(n, orig_flag)`` per round (:872),
    the centres behind round 0's (:875-879)."""
    D, K = mu.shape
    lam, out = np.ravel(lambd)[None, :], []
    for k in range(n_opts):
        if K > 1:
            i = np.random.choice(range(K), size=n, p=np.ravel(w))
            x = mu.T[i] + lam * np.random.randn(n, D) * np.ravel(sigma)[i][:, None]
        else:
            x = mu.T + lam * np.random.randn(n, D) * np.ravel(sigma)
        if k == 0:
            x = np.concatenate([x, mu.T])
        if orig_flag and pt is not None:
            x = pt.inverse(x)
        out.append(x)
    return out


def mode_host(mu, sigma, lambd, w, pt, orig_flag, candidates, fast=False):
    """``(x, f, records, points, ys)`` of the multi-start search from the given per-round candidates: records rows
    (start index, start value, final value, iterations, status), the rounds' final points and their search
    coordinates."""
    obj = Objective(mu, sigma, lambd, w, pt, orig_flag)
    recs, pts, ys = [], [], []
    for cand in candidates:
        vals = (fast_log_pdf if fast else host_log_pdf)(mu, sigma, lambd, w, pt, cand, orig_flag)
        vals = np.where(np.isnan(vals), -np.inf, vals)  # NaN never wins
        idx = int(np.argmax(vals))
        y, _, it, status = search(obj, obj.y_from_x(cand[idx]))
        x = obj.x_from_y(y)
        fx = host_log_pdf(mu, sigma, lambd, w, pt, x, orig_flag)[0]
        recs.append((idx, vals[idx], fx, it, status))
        pts.append(x)
        ys.append(y)
    best = int(np.argmax([r[2] for r in recs]))
    return pts[best], recs[best][2], recs, np.array(pts), np.array(ys)


def stationarity(obj, y):
    """``(largest |gradient| over the free dimensions, whether the gradient points outward on every held one)``."""
    _, g, _, _ = obj.full(y)
    free = obj.free_set(y, g)
    at_lo, at_hi = y <= obj.lo, y >= obj.hi
    outward = bool(np.all(g[at_lo & ~free] < 0) and np.all(g[at_hi & ~free] > 0))
    return (float(np.max(np.abs(g[free]))) if np.any(free) else 0.0), outward


def f_tol(K, D, f):
    """The rounding of one log-density evaluation: K D terms of relative error eps."""
    return K * D * np.finfo(np.float64).eps * max(1.0, abs(f))
