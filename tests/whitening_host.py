"""A NumPy statement of input warping (rotoscaling), written from the formulas, for the tests: the unscented transform of
the warp "old inference space -> original space -> new inference space", ``warp_input``'s whitening transform and box
statistics, and ``warp_gp_and_vp``'s push of the GP hyper-parameters and the mixture through the warp.  Every quantity
is an explicit argument; nothing is read from objects.  tests/test_whitening_host.py pins it against
tests/golden/whitening.npz (the reference's outputs).

A transformer is ``Xf``: the per-dimension maps of tests/transform_host.py (the table in its docstring) followed by the
rotation R and the scale, in a chosen floating-point type.  ``dtype=np.float64`` keeps the reference's order of
operations; ``dtype=np.longdouble`` evaluates the same formulas in extended precision (erfc / erfcinv of the probit type
by a series and Newton steps in long double) and is the "truth" the GPU tests measure both the float64 statement and the device
against:

    bound(q) = max(8 * |float64 statement - truth|, 1e-12 * scale(q))

the margin and the method of tests/test_gp_illcond_gpu.py.

The formulas.  With U = 2 D + 1 sigma points  x, x +- sqrt(D) sigma_d e_d  per base point and W the warp:
    mean = (1 / U) sum_u W(p_u),    sd^2 = (1 / (U - 1)) sum_u (W(p_u) - mean)^2        (two passes)
warp_input:  C = the mixture's covariance brought back to unrotated, unscaled, uncentred coordinates; entries with
|corr| <= thresh zeroed; C <- (1 - r) C + r diag(C); C = U diag(s) V^T, det U made positive by flipping column 0;
R = U, scale = sqrt(s + eps); new mu = 0, delta = 1.  Plausible box: the 0.05 / 0.95 quantiles of new(uniform draws in
the original plausible box), widened by span / 9.  Search box: min / max of W(uniform draws in the old search box),
widened by span / n_search.  Training points: X = new(X_orig), y = y_orig + log|J_new|(X) / T.
warp_gp_and_vp:  log ell_new = mean_n log sd(X_n, ell);  ConstantMean  m0 += (mean dy - mean dy_old) / T;
NegativeQuadratic  (xm, omega) -> (mean, sd) of their unscented warp, m0 += (dy(mean) - dy_old(xm)) / T;  mixture:
(mu_k, sigma_k lambda) -> (mu'_k, s_k), lambda' = sqrt(D mean_k(s_kd^2 / sum_d s_kd^2)), sigma'_k = exp(mean_d log(s_kd /
lambda'_d)), w'_k ~ w_k exp((dy(mu'_k) - dy_old(mu_k)) / T).
"""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
from scipy.special import erfc, erfcinv

GOLDEN = Path(__file__).resolve().parent / "golden" / "whitening.npz"
CASES = ("a", "b", "c", "d")
LD = np.longdouble

_TINY = np.nextafter(0.0, 1.0)
_BELOW_ONE = np.nextafter(1.0, 0.0)
_LOG_MAX = np.log(np.finfo(np.float64).max)


def _pi_ld():
    return LD("3.14159265358979323846264338327950288")


def _erf_ld(x):
    """erf in long double by the all-positive series (2 / sqrt(pi)) exp(-x^2) sum_n 2^n x^(2n+1) / (2n+1)!!: no
    cancellation, absolute error a few long-double eps for |x| <= 6 (the tests' points)."""
    x = np.asarray(x, dtype=LD)
    ax = np.abs(x)
    term = ax.copy()
    total = ax.copy()
    for n in range(240):
        term = term * (2 * ax * ax) / LD(2 * n + 3)
        total = total + term
    return np.sign(x) * np.minimum(LD(2) / np.sqrt(_pi_ld()) * np.exp(-ax * ax) * total, LD(1))


def _erfc(a):
    return erfc(a) if a.dtype == np.float64 else LD(1) - _erf_ld(a)


def _erfcinv(a):
    """float64: SciPy's.  Long double: three Newton steps on erfc(x) = a from SciPy's value (quadratic: exact to the
    precision of _erf_ld, whose absolute error the slope exp(x^2) sqrt(pi) / 2 magnifies -- below 1e-15 for |x| <= 3)."""
    if a.dtype == np.float64:
        return erfcinv(a)
    x = np.asarray(erfcinv(a.astype(np.float64)), dtype=LD)
    for _ in range(3):
        x = x + (_erfc(x) - a) * np.sqrt(_pi_ld()) / 2 * np.exp(x * x)
    return x


class Xf:
    """Transformer fields and the three maps in ``dtype``."""

    def __init__(self, type, lb, ub, mu, delta, R=None, scale=None, dtype=np.float64):
        self.dtype = dtype
        self.type = np.asarray(type, dtype=np.float64).ravel()
        self.lb, self.ub = np.asarray(lb, dtype=np.float64).ravel(), np.asarray(ub, dtype=np.float64).ravel()
        self.mu, self.delta = np.asarray(mu, dtype=dtype).ravel(), np.asarray(delta, dtype=dtype).ravel()
        self.R = None if R is None or np.size(R) == 0 else np.asarray(R, dtype=dtype)
        self.scale = None if scale is None or np.size(scale) == 0 else np.asarray(scale, dtype=dtype).ravel()

    def astype(self, dtype):
        return Xf(self.type, self.lb, self.ub, self.mu, self.delta, self.R, self.scale, dtype)

    @classmethod
    def from_golden(cls, g, prefix, dtype=np.float64):
        return cls(g[prefix + "type"], g[prefix + "lb"], g[prefix + "ub"], g[prefix + "mu"], g[prefix + "delta"],
                   g[prefix + "R"], g[prefix + "scale"], dtype)

    def as_object(self):
        """A reference-shaped duck (tests/transform_host.py) with these fields."""
        from transform_host import RefShapedTransformer

        return RefShapedTransformer(self.type, self.lb, self.ub, np.asarray(self.mu, dtype=np.float64),
                                    np.asarray(self.delta, dtype=np.float64),
                                    None if self.R is None else np.asarray(self.R, dtype=np.float64),
                                    None if self.scale is None else np.asarray(self.scale, dtype=np.float64))

    # per-dimension pieces ------------------------------------------------------------------------------------------
    def _g(self, t, z):
        one = self.dtype(1)
        if t == 3:
            with np.errstate(divide="ignore", invalid="ignore"):
                return np.where(z == 0, -np.inf, np.where(z == 1, np.inf, np.log(z / (one - z))))
        if t == 12:
            return -np.sqrt(self.dtype(2)) * _erfcinv(2 * z)
        a = np.sqrt(4 * z * (one - z))
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(a == 0, np.inf, np.cos(np.arccos(a) / 3) / a)
        return np.sign(z - self.dtype(0.5)) * (2 * np.sqrt(q - one))

    def _ginv(self, t, y):
        one = self.dtype(1)
        if t == 3:
            with np.errstate(over="ignore"):
                return np.where(-y > _LOG_MAX, self.dtype(0), one / (one + np.exp(-y)))
        if t == 12:
            return self.dtype(0.5) * _erfc(-y / np.sqrt(self.dtype(2)))
        s = y**2
        c = one + s / 4
        return self.dtype(0.5) + (self.dtype(3) / 8) * (y / np.sqrt(c)) * (one - s / c / 12)

    def _lj(self, t, y):
        if t == 3:
            return -y + 2 * (-np.log1p(np.exp(-y)))
        if t == 12:
            pi = self.dtype(np.pi) if self.dtype == np.float64 else _pi_ld()
            return -self.dtype(0.5) * np.log(2 * pi) - self.dtype(0.5) * y**2
        return np.log(self.dtype(3) / 8) - (self.dtype(5) / 2) * np.log1p(y**2 / 4)

    # the three maps ------------------------------------------------------------------------------------------------
    def forward(self, x):
        x = np.array(np.atleast_2d(x), dtype=self.dtype)
        out = np.empty_like(x)
        for d, t in enumerate(self.type.astype(int)):
            col = x[:, d]
            if t == 0:
                out[:, d] = (col - self.mu[d]) / self.delta[d]
                continue
            lb, ub = self.dtype(self.lb[d]), self.dtype(self.ub[d])
            z = (col - lb) / (ub - lb)
            z = np.where((z == 0) & (col != lb), self.dtype(_TINY), z)
            z = np.where((z == 1) & (col != ub), self.dtype(_BELOW_ONE), z)
            out[:, d] = (self._g(t, z) - self.mu[d]) / self.delta[d]
        if self.R is not None:
            out = np.dot(out, self.R)
        if self.scale is not None:
            out = out / self.scale
        return out

    def _centred(self, u):
        v = np.array(np.atleast_2d(u), dtype=self.dtype)
        if self.scale is not None:
            v = v * self.scale
        if self.R is not None:
            v = np.dot(v, self.R.T)
        return v

    def inverse(self, u):
        v = self._centred(u)
        out = np.empty_like(v)
        for d, t in enumerate(self.type.astype(int)):
            y = v[:, d] * self.delta[d] + self.mu[d]
            if t == 0:
                out[:, d] = y
            else:
                lb, ub = self.dtype(self.lb[d]), self.dtype(self.ub[d])
                out[:, d] = np.clip(self._ginv(t, y) * (ub - lb) + lb, self.dtype(np.nextafter(self.lb[d], np.inf)),
                                    self.dtype(np.nextafter(self.ub[d], -np.inf)))
        return out

    def log_abs_det(self, u):
        v = self._centred(u)
        terms = np.empty_like(v)
        for d, t in enumerate(self.type.astype(int)):
            if t == 0:
                terms[:, d] = np.log(self.delta[d])
            else:
                terms[:, d] = (np.log(self.dtype(self.ub[d]) - self.dtype(self.lb[d]))
                               + self._lj(t, v[:, d] * self.delta[d] + self.mu[d]) + np.log(self.delta[d]))
        if self.scale is not None:
            terms = terms + np.log(self.scale)
        return terms.sum(axis=1)


def warp(old, new, x):
    """new(old^-1(x)) on rows."""
    return new.forward(old.inverse(x))


def unscent_warp(old, new, x, sigma):
    """(mean, sd, points) of the unscented warp: x (n, D), sigma (n, D) or (1, D); the points are (U, n, D)."""
    dt = new.dtype
    x, sigma = np.array(np.atleast_2d(x), dtype=dt), np.array(np.atleast_2d(sigma), dtype=dt)
    n, D = max(x.shape[0], sigma.shape[0]), x.shape[1]
    if x.shape[0] not in (1, n) or sigma.shape[0] not in (1, n):
        raise ValueError("Mismatch between rows of X and SIGMA.")
    if sigma.shape[1] != D:
        raise ValueError("Mismatch between columns of X and SIGMA.")
    x, sigma = np.broadcast_to(x, (n, D)), np.broadcast_to(sigma, (n, D))
    U = 2 * D + 1
    pts = np.empty((U, n, D), dtype=dt)
    pts[:] = x
    root = np.sqrt(dt(D))
    for d in range(D):
        pts[2 * d + 1, :, d] = x[:, d] + root * sigma[:, d]
        pts[2 * d + 2, :, d] = x[:, d] - root * sigma[:, d]
    w = warp(old, new, pts.reshape(U * n, D)).reshape(U, n, D)
    mean = np.sum(w, axis=0) / dt(U)
    sd = np.sqrt(np.sum((w - mean) ** 2, axis=0) / dt(U - 1))
    return mean, sd, w


def mixture_cov(mu_DK, sigma, lambd, w):
    """Covariance of the mixture in its own inference space: the within-component part on the diagonal, then the
    components' weighted outer products added one by one (the order the SVD's input bits depend on)."""
    mu_DK = np.asarray(mu_DK, dtype=np.float64)
    w, sigma, lambd = np.ravel(w), np.ravel(sigma), np.ravel(lambd)
    mean = np.sum(w * mu_DK, axis=1)
    cov = np.sum(w * sigma**2) * np.diag(lambd**2)
    for k in range(w.size):
        dev = mu_DK[:, k] - mean
        cov = cov + w[k] * np.outer(dev, dev)
    return cov


def rotoscale(cov, old, thresh, cov_reg):
    """(R, scale) of the whitening transform from the mixture's covariance ``cov`` in the old inference space."""
    D = cov.shape[0]
    R = np.eye(D) if old.R is None else np.asarray(old.R, dtype=np.float64)
    s = np.ones(D) if old.scale is None else np.asarray(old.scale, dtype=np.float64)
    delta = np.asarray(old.delta, dtype=np.float64)
    C = R @ np.diag(s) @ cov @ np.diag(s) @ R.T
    C = np.diag(delta) @ C @ np.diag(delta)
    if thresh > 0:
        corr = C / np.sqrt(np.outer(np.diag(C), np.diag(C)))
        C[np.abs(corr) <= thresh] = 0
    r = min(1, max(0, cov_reg))
    C = (1 - r) * C + r * np.diag(np.diag(C))
    U, sv, _ = np.linalg.svd(C)
    if np.linalg.det(U) < 0:
        U[:, 0] = -U[:, 0]
    return U, np.sqrt(sv + np.finfo(np.float64).eps)


def quantile_linear(y, q):
    """np.quantile's default rule per column, from the sorted columns (any dtype)."""
    s = np.sort(y, axis=0)
    n = s.shape[0]
    vi = (n - 1) * q
    lo = int(np.floor(vi))
    hi = min(lo + 1, n - 1)
    g = s.dtype.type(vi - lo)
    return s[lo] + (s[hi] - s[lo]) * g


def warp_input(old, new, *, plb_orig, pub_orig, lb_search, ub_search, X_orig, y_orig, X_flag, X, y, search_cache,
               temperature, u_plausible, u_search, n_search):
    """Everything of warp_input past the whitening transform: ``new`` is the finished new transformer, the uniform draws
    are given (``u_plausible`` (n_plausible, D), ``u_search`` (n_search, D)).  Returns a namespace of the results."""
    dt = new.dtype
    D = new.type.size
    r = SimpleNamespace()
    box = np.asarray(u_plausible, dtype=dt) * (np.ravel(pub_orig).astype(dt) - np.ravel(plb_orig).astype(dt)) \
        + np.ravel(plb_orig).astype(dt)
    yy = new.forward(box)
    r.plausible_image = yy
    lo, hi = (np.quantile(yy, [0.05, 0.95], axis=0) if dt == np.float64
              else (quantile_linear(yy, 0.05), quantile_linear(yy, 0.95)))
    span = hi - lo
    r.plb_tran, r.pub_tran = (lo - span / 9).reshape(1, D), (hi + span / 9).reshape(1, D)
    T = dt(temperature) if temperature else dt(1)
    Xn = new.forward(np.asarray(X_orig)[X_flag, :])
    dy = new.log_abs_det(Xn)
    r.X, r.y = np.array(X, dtype=dt), np.array(y, dtype=dt)
    r.X[X_flag, :] = Xn
    r.y[X_flag] = (np.asarray(y_orig, dtype=dt)[X_flag].T + dy / T).T
    box = np.asarray(u_search, dtype=dt) * (np.ravel(ub_search).astype(dt) - np.ravel(lb_search).astype(dt)) \
        + np.ravel(lb_search).astype(dt)
    yy = warp(old, new, box)
    r.search_image = yy
    lo, hi = np.min(yy, axis=0), np.max(yy, axis=0)
    span = hi - lo
    r.lb_search, r.ub_search = np.atleast_2d(lo - span / n_search), np.atleast_2d(hi + span / n_search)
    cache = np.asarray(search_cache, dtype=dt).reshape(-1, D)
    r.search_cache = warp(old, new, cache) if cache.shape[0] else cache
    return r


def warp_gp_and_vp(old, new, *, mean_kind, gp_X, hyp, mu_DK, sigma, lambd, w, temperature):
    """(hyp_warped (S, P), mu (D, K), sigma (1, K), lambd (D, 1), w (1, K)) after the warp."""
    dt = new.dtype
    gp_X, hyp = np.asarray(gp_X, dtype=dt), np.array(np.atleast_2d(hyp), dtype=dt)
    D = gp_X.shape[1]
    T = dt(temperature) if temperature else dt(1)
    o = D + 2  # squared-exponential covariance (D + 1) and one noise parameter come first
    out = hyp.copy()
    N = gp_X.shape[0]
    for s in range(hyp.shape[0]):
        _, sd, _ = unscent_warp(old, new, gp_X, np.exp(hyp[s, :D]))
        out[s, :D] = np.sum(np.log(sd), axis=0) / dt(N)
    if mean_kind == "ConstantMean":
        dy_old = old.log_abs_det(gp_X)
        dy = new.log_abs_det(warp(old, new, gp_X))
        out[:, o] = hyp[:, o] + (np.sum(dy) / dt(N) - np.sum(dy_old) / dt(N)) / T
    elif mean_kind == "NegativeQuadratic":
        xm, omega = hyp[:, o + 1:o + 1 + D], np.exp(hyp[:, o + 1 + D:o + 1 + 2 * D])
        xmw, omegaw, _ = unscent_warp(old, new, xm, omega)
        out[:, o] = hyp[:, o] + (new.log_abs_det(xmw) - old.log_abs_det(xm)) / T
        out[:, o + 1:o + 1 + D] = xmw
        out[:, o + 1 + D:o + 1 + 2 * D] = np.log(omegaw)
    else:
        raise ValueError("Unsupported GP mean function for input warping.")
    mu = np.asarray(mu_DK, dtype=dt).T
    sl = (np.asarray(lambd, dtype=dt).reshape(-1, 1) * np.asarray(sigma, dtype=dt).reshape(1, -1)).T
    muw, slw, _ = unscent_warp(old, new, mu, sl)
    lam = np.sqrt(dt(D) * np.mean((slw**2).T / np.sum(slw**2, axis=1), axis=1))
    sig = np.exp(np.mean(np.log(slw / lam), axis=1))
    ww = np.ravel(np.asarray(w, dtype=dt)) * np.exp((new.log_abs_det(muw) - old.log_abs_det(mu)) / T)
    return out, muw.T, sig.reshape(1, -1), lam.reshape(-1, 1), (ww / np.sum(ww)).reshape(1, -1)


# ---- the golden cases ------------------------------------------------------------------------------------------------
_G = {}


def golden():
    if "g" not in _G:
        _G["g"] = dict(np.load(GOLDEN, allow_pickle=False))
    return _G["g"]


def load_case(name):
    """The stored inputs and outputs of a case as a namespace (fields without the ``<name>_`` prefix)."""
    g = golden()
    c = SimpleNamespace(**{k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + "_")})
    c.name = name
    c.D, c.K, c.S = int(c.D), int(c.K), int(c.S)
    c.mean = str(c.mean)
    c.temperature = float(c.temperature)
    c.old = Xf.from_golden(g, f"{name}_old_")
    c.new = Xf.from_golden(g, f"{name}_new_")
    return c


def box_draws(c, n_plausible=100000, n_search=1000):
    """The two uniform samples warp_input takes from the seeded global stream, and the draw that follows them."""
    st = np.random.RandomState(int(c.np_seed))
    return st.rand(n_plausible, c.D), st.rand(n_search, c.D), st.rand()


def run_warp_input(c, dtype=np.float64, n_plausible=100000, n_search=1000):
    """The statement's warp_input on a case: (R, scale, results namespace)."""
    R, scale = rotoscale(mixture_cov(c.mu, c.sigma, c.lambd, c.w), c.old, float(c.thresh), float(c.cov_reg))
    new = Xf(c.old.type, c.old.lb, c.old.ub, np.zeros(c.D), np.ones(c.D), R, scale, dtype)
    u1, u2, _ = box_draws(c, n_plausible, n_search)
    r = warp_input(c.old.astype(dtype), new, plb_orig=c.plb_orig, pub_orig=c.pub_orig, lb_search=c.lb_search,
                   ub_search=c.ub_search, X_orig=c.X_orig, y_orig=c.y_orig, X_flag=c.X_flag, X=c.X, y=c.y,
                   search_cache=c.search_cache, temperature=c.temperature, u_plausible=u1, u_search=u2, n_search=n_search)
    return R, scale, r


def run_warp_gp_and_vp(c, dtype=np.float64):
    return warp_gp_and_vp(c.old.astype(dtype), c.new.astype(dtype), mean_kind=c.mean, gp_X=c.gp_X, hyp=c.hyp, mu_DK=c.mu,
                          sigma=c.sigma, lambd=c.lambd, w=c.w, temperature=c.temperature)


# ---- cases at any dimension (nothing recorded) ------------------------------------------------------------------------
WIDE_TYPES = (0, 3, 12, 13)


def box_uniforms(n, D, seed):
    """The (n, D) uniforms of csrc/warp.hip's Philox box draws: dimensions 2 p and 2 p + 1 of draw i are the two 53-bit
    uniforms of block (i, p, stream 9) under the key ``seed``."""
    from oracle import philox_ref as pr

    lo, hi = pr._split(np.arange(n, dtype=np.uint64))
    out = np.empty((n, D))
    for p in range((D + 1) // 2):
        x = pr.philox4x32_10(lo, hi, np.full_like(lo, p), np.full_like(lo, 9), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
        for h in range(2):
            if 2 * p + h < D:
                word = (x[2 * h].astype(np.uint64) << np.uint64(32)) | x[2 * h + 1].astype(np.uint64)
                out[:, 2 * p + h] = (word >> np.uint64(11)).astype(np.float64) * 2.0**-53
    return out


def wide_case(D, K=3, S=2, N=37, wide_golden=None):
    """A case of the entry-point tests at dimension D, with the fields ``load_case`` gives them (no recorded outputs).

    The old transformer cycles the type codes 0, 3, 12, 13 over its dimensions and is rotated and scaled.  Where
    ``wide_golden`` (tests/golden/transform_wide.npz) has a case of this D, a bounded dimension of it lends its finite
    bounds, mu and delta; everything else is drawn from ``default_rng(D)``.  The new transformer is the whitening
    transform ``rotoscale`` derives from the K-component mixture's covariance.  Points, box edges and unscented steps are
    sized so that the centred coordinates stay within about one delta: no bounded map is driven into its saturated tail,
    where the float64 statement itself loses its digits."""
    r = np.random.default_rng(D)
    types = np.array([WIDE_TYPES[d % 4] for d in range(D)], dtype=np.float64)
    lb = r.uniform(-10.0, 0.0, D)
    ub = lb + r.uniform(1.0, 12.0, D)
    mu, delta = 0.2 * r.standard_normal(D), r.uniform(0.5, 2.0, D)
    name = f"w{D}"
    if wide_golden is not None and f"{name}_type" in wide_golden:
        glb, gub = np.ravel(wide_golden[f"{name}_lb"]), np.ravel(wide_golden[f"{name}_ub"])
        take = np.isfinite(glb) & np.isfinite(gub)
        lb, ub = np.where(take, glb, lb), np.where(take, gub, ub)
        mu, delta = np.where(take, wide_golden[f"{name}_mu"], mu), np.where(take, wide_golden[f"{name}_delta"], delta)
    lb, ub = np.where(types == 0, -np.inf, lb), np.where(types == 0, np.inf, ub)
    R, _ = np.linalg.qr(r.standard_normal((D, D)))
    old = Xf(types, lb, ub, mu, delta, R, r.uniform(0.5, 1.0, D))
    c = SimpleNamespace(name=f"wide{D}", D=D, K=K, S=S, old=old)
    c.mu = 0.3 * r.standard_normal((D, K))
    c.sigma = (0.3 / np.sqrt(D)) * r.uniform(0.5, 1.0, (1, K))
    c.lambd = r.uniform(0.7, 1.3, (D, 1))
    c.w = r.uniform(0.5, 1.0, (1, K))
    c.w = c.w / np.sum(c.w)
    Rn, scale = rotoscale(mixture_cov(c.mu, c.sigma, c.lambd, c.w), old, 0.0, 0.0)
    c.new = Xf(types, lb, ub, np.zeros(D), np.ones(D), Rn, scale)
    c.gp_X = 0.3 * r.standard_normal((N, D))
    c.hyp = np.hstack([np.log((0.3 / np.sqrt(D)) * r.uniform(0.5, 1.0, (S, D))), r.standard_normal((S, 2 * D + 3))])
    c.X_orig = old.inverse(0.3 * r.standard_normal((N, D)))
    c.X_flag = np.ones(N, dtype=bool)
    centre = old.inverse(np.zeros((1, D)))
    half = np.where(types == 0, 1.0, 0.2 * (np.where(types == 0, 1.0, ub) - np.where(types == 0, 0.0, lb)))
    c.plb_orig, c.pub_orig = centre - half * r.uniform(0.5, 1.0, D), centre + half * r.uniform(0.5, 1.0, D)
    h = 1.0 / np.sqrt(D)
    c.lb_search, c.ub_search = (-h * r.uniform(0.5, 1.0, D)).reshape(1, D), (h * r.uniform(0.5, 1.0, D)).reshape(1, D)
    return c


# ---- stand-ins with the reference objects' attribute names, for the package's functions ---------------------------------
class PlainVP:
    """The attributes ``pyvbmc_amd.whitening`` reads of a posterior."""

    def __init__(self, c, pt):
        self.D, self.K = c.D, c.K
        self.mu, self.sigma, self.lambd, self.w = c.mu.copy(), c.sigma.copy(), c.lambd.copy(), c.w.copy()
        self.parameter_transformer = pt

    def moments(self, orig_flag=False, cov_flag=True):
        assert not orig_flag and cov_flag
        return np.sum(self.w * self.mu, axis=1).reshape(1, -1), mixture_cov(self.mu, self.sigma, self.lambd, self.w)


class _Count:
    def __init__(self, n):
        self.n = n

    def hyperparameter_count(self, D=None):
        return self.n if not callable(self.n) else self.n(D)


class ConstantMean(_Count):
    def __init__(self):
        super().__init__(1)


class NegativeQuadratic(_Count):
    def __init__(self):
        super().__init__(lambda D: 1 + 2 * D)


class ZeroMean(_Count):
    def __init__(self):
        super().__init__(0)


def package_inputs(c):
    """(vp, optim_state, function_logger, options, gp) stand-ins of a case for ``pyvbmc_amd.whitening``."""
    pt = c.old.as_object()
    vp = PlainVP(c, pt)
    state = {"plb_orig": c.plb_orig, "pub_orig": c.pub_orig, "lb_search": c.lb_search, "ub_search": c.ub_search,
             "search_cache": c.search_cache.copy(), "warping_count": int(c.warping_count), "iter": int(c.iter), "N": 0,
             "run_mean": [1.0], "run_cov": [1.0], "last_run_avg": 3.0}
    if c.temperature:
        state["temperature"] = c.temperature
    flog = SimpleNamespace(X=c.X.copy(), y=c.y.copy(), X_orig=c.X_orig, y_orig=c.y_orig, X_flag=c.X_flag,
                           parameter_transformer=pt)
    options = {"warp_rotoscaling": True, "warp_nonlinear": False, "warp_roto_corr_thresh": float(c.thresh),
               "warp_cov_reg": float(c.cov_reg)}
    gp = SimpleNamespace(covariance=_Count(lambda D: D + 1), noise=_Count(1), mean=globals()[c.mean](), X=c.gp_X,
                         posteriors=[SimpleNamespace(hyp=h.copy()) for h in c.hyp])
    return vp, state, flog, options, gp
