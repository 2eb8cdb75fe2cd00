"""A NumPy / SciPy restatement of ``kde_1d`` (reference stats/kde_1d.py:144) and ``VariationalPosterior.mtv``
(variational_posterior.py:921-1030), written from the algorithm, plus the sample recipes of
tests/golden/kde_mtv.npz (tools/make_mtv_golden.py imports the same recipes, so the fixture stores no samples).

kde_1d, after Botev, Grotowski and Kroese (2010): the samples are binned on a uniform mesh of n points
(n rounded up to a power of two; bounds min/max -+ 10 % of the range unless given), the normalised counts
go through a DCT-II, and the diffusion time t* is the smallest root of t - xi gamma^[7](t), found by
brentq on [0, tol] with tol doubled until a bracket is found (tol = 1e-12 + 0.01 (N - 50) / 1000, N the
number of distinct samples clamped to [50, 1050]).  Failing that, Scott's rule gives the bandwidth.  The
density is the DCT-III of the coefficients damped by exp(-k^2 pi^2 t* / 2), over 2 (upper - lower),
negatives set to 0.

mtv: per dimension, each side's density (mesh 2^13, bounds min/max -+ range/10 clipped to the
transformer's bounds) is normalised to unit trapezoid integral and interpolated by the not-a-knot cubic
spline (0 outside its mesh); half the trapezoid integral of |s1 - s2| over the three linspace(., ., 1e5)
segments between the sorted mesh ends is the distance.
"""
import numpy as np
from scipy.fft import dct, idct
from scipy.interpolate import make_interp_spline
from scipy.optimize import brentq

# ---- sample recipes (legacy RandomState streams) ---------------------------------------------------------


def kde_samples(name):
    """The samples of kde case ``name``."""
    r = np.random.RandomState(abs(hash_name(name)) % (2**31))
    if name == "three":
        return np.array([0.1, 0.7, 2.5])
    if name == "zeros_ones":
        return np.concatenate((np.zeros(500), np.ones(500)))
    if name == "bimodal":
        return np.concatenate((r.randn(3000), r.randn(2000) * 2 + 35, r.randn(1000) + 55))
    if name == "rounded":
        return np.round(r.randn(20000) * 3, 1)
    if name == "signed_zero":
        x = r.randn(4000)
        x[:200] = 0.0
        x[200:400] = -0.0
        return x
    if name in ("gauss", "gauss_n10", "gauss_n13", "gauss_odd", "bounded"):
        return r.randn(100000) * 1.5 + 0.3
    if name == "skewed":
        return r.standard_gamma(2.0, 50000)
    if name == "constant":
        return np.full(100, 3.25)
    raise KeyError(name)


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % 1000003
    return h


# name -> (n, lower_bound, upper_bound)
KDE_CASES = {
    "three": (2**14, None, None),
    "zeros_ones": (2**14, None, None),
    "bimodal": (2**14, None, None),
    "rounded": (2**14, None, None),
    "signed_zero": (2**13, None, None),
    "gauss": (2**14, None, None),
    "gauss_n10": (2**10, None, None),
    "gauss_n13": (2**13, None, None),
    "gauss_odd": (2**14 - 10, None, None),
    "bounded": (2**14, -2.0, 3.0),  # excludes samples on both sides
    "skewed": (2**12, 0.0, None),
}
FULL_DENSITY = ("three", "bimodal", "gauss_n10", "bounded")  # stored in full; the rest every 16th point


def mtv_case(name):
    """``(D, K, N, spec1, spec2, samples_rows)`` of mtv case ``name``; spec = (kind, seed) with kind
    "identity" / "bounded" / "roto"; samples_rows > 0: the second side is that many samples."""
    return {
        "d1": (1, 2, 100000, ("identity", 1), ("identity", 2), 0),
        "d2_bounded": (2, 3, 100000, ("bounded", 3), ("bounded", 3), 0),
        "d10": (10, 50, 100000, ("identity", 4), ("identity", 5), 0),
        "d10_xf": (10, 5, 100000, ("bounded", 6), ("roto", 7), 0),
        "d32": (32, 4, 20000, ("roto", 8), ("identity", 9), 0),
        "samples": (3, 4, 50000, ("bounded", 10), None, 30000),
    }[name]


MTV_CASES = ("d1", "d2_bounded", "d10", "d10_xf", "d32", "samples")


def mixture_params(D, K, seed):
    """mu (D x K), sigma (1 x K), lambd (D x 1), w (1 x K) of a test posterior."""
    r = np.random.RandomState(seed)
    mu = r.randn(D, K) * 1.5
    sigma = np.exp(r.randn(1, K) * 0.3 - 0.5)
    lambd = np.exp(r.randn(D, 1) * 0.2)
    lambd = lambd / np.sqrt(np.sum(lambd**2) / D)
    w = r.rand(1, K) + 0.2
    return mu, sigma, lambd, w / np.sum(w)


def transformer_spec(kind, D, seed):
    """Reference ``ParameterTransformer`` constructor arguments: (lb, ub, plb, pub, transform_type, rotoscale)."""
    r = np.random.RandomState(seed + 1000)
    if kind == "identity":
        return None
    lb = np.full(D, -np.inf)
    ub = np.full(D, np.inf)
    bnd = np.arange(D) % 2 == 0
    lb[bnd] = -4.0 - r.rand(bnd.sum())
    ub[bnd] = 4.0 + r.rand(bnd.sum())
    plb = np.where(bnd, lb + 1.0, -3.0)
    pub = np.where(bnd, ub - 1.0, 3.0)
    return lb, ub, plb, pub, ("probit" if kind == "roto" else "logit"), kind == "roto"


# ---- the restatement ---------------------------------------------------------------------------------------


def _mesh(lo, hi, n):
    return np.linspace(lo, hi, n)


def _counts(x, mesh):
    """Samples per mesh point (bins centred on the points), integers."""
    dx = mesh[1] - mesh[0]
    keep = x[(x >= mesh[0]) & (x <= mesh[-1])]
    b = np.floor((keep - (mesh[0] - 0.5 * dx)) / dx).astype(np.int64)
    return np.bincount(b, minlength=mesh.size).astype(np.float64)


def _gamma_l(t, nu, k2, a2):
    """t - xi gamma^[7](t): the functional of the 7th derivative, stepped down to the 2nd."""
    f = 2.0 * np.pi**14 * np.sum(k2**7 * a2 * np.exp(-k2 * np.pi**2 * t))
    if f <= 0:
        return -1.0
    for s in range(6, 1, -1):
        k0 = np.prod(np.arange(1.0, 2 * s, 2.0)) / np.sqrt(2 * np.pi)
        c = (1 + 0.5 ** (s + 0.5)) / 3
        tj = (2 * c * k0 / (nu * f)) ** (2 / (3 + 2 * s))
        f = 2.0 * np.pi ** (2 * s) * np.sum(k2**s * a2 * np.exp(-k2 * np.pi**2 * tj))
    return t - (2 * nu * np.sqrt(np.pi) * f) ** (-0.4)


def _smallest_root(nu, k2, a2):
    ncl = max(min(1050.0, nu), 50.0)
    tol = 1e-12 + 0.01 * (ncl - 50.0) / 1000.0
    while tol < 1:
        try:
            x, r = brentq(_gamma_l, 0, tol, args=(nu, k2, a2), full_output=True, disp=False)
        except ValueError:
            tol *= 2.0
            continue
        if r.converged and x > 0:
            return x
        return None  # (the reference would repeat this call forever)
    return None


def kde_1d_host(samples, n=2**14, lower_bound=None, upper_bound=None):
    """``(density, xmesh, bandwidth, scott, n_unique)``; bandwidth a float."""
    x = np.asarray(samples, dtype=np.float64).ravel()
    n = int(2 ** np.ceil(np.log2(n)))
    lo, hi = x.min(), x.max()
    lower = lo - 0.1 * (hi - lo) if lower_bound is None else float(np.ravel(lower_bound)[0])
    upper = hi + 0.1 * (hi - lo) if upper_bound is None else float(np.ravel(upper_bound)[0])
    width = upper - lower
    mesh = _mesh(lower, upper, n)
    nu = np.unique(x).size
    c = _counts(x, mesh)
    a = dct(c / c.sum(), type=2)
    k2 = np.arange(1, n, dtype=np.float64) ** 2
    t = _smallest_root(nu, k2, a[1:] ** 2 / 4)
    scott = t is None
    if scott:
        q75, q25 = np.quantile(x, 0.75), np.quantile(x, 0.25)
        bw = min(np.std(x, ddof=1), (q75 - q25) / 1.3489795003921634) * x.size ** (-0.2)
        t = (bw / width) ** 2
    else:
        bw = np.sqrt(t) * width
    k = np.arange(n, dtype=np.float64)
    # scipy.fft.idct scales by 1 / (2 n) (norm="backward"); the unnormalised DCT-III is 2 n times it
    dens = idct(a * np.exp(-(k**2) * np.pi**2 * t / 2), type=2) * (2 * n) / (2 * width)
    dens[dens < 0] = 0.0
    return dens, mesh, float(bw), scott, nu


def mtv_host(xx1, xx2, lb1, ub1, lb2, ub2, nkde=2**13):
    """The (D,) distances between the sample sets xx1 (n1 x D) and xx2 (n2 x D) with per-dimension bounds."""
    D = xx1.shape[1]
    out = np.zeros(D)

    def side(x, lb, ub):
        lo, hi = x.min(), x.max()
        r = hi - lo
        dens, mesh, _, _, _ = kde_1d_host(x, nkde, max(lo - r / 10, lb), min(hi + r / 10, ub))
        dx = mesh[1] - mesh[0]
        dens = dens / (np.sum((dens[1:] + dens[:-1]) / 2) * dx)
        return make_interp_spline(mesh, dens, k=3), mesh

    for d in range(D):
        s1, m1 = side(xx1[:, d], lb1[d], ub1[d])
        s2, m2 = side(xx2[:, d], lb2[d], ub2[d])

        def ev(s, m, p):
            return np.where((p >= m[0]) & (p <= m[-1]), s(p), 0.0)

        ends = np.sort([m1[0], m1[-1], m2[0], m2[-1]])
        for j in range(3):
            p = np.linspace(ends[j], ends[j + 1], 100000)
            f = np.abs(ev(s1, m1, p) - ev(s2, m2, p))
            out[d] += 0.5 * np.sum((f[1:] + f[:-1]) / 2) * (p[1] - p[0])
    return out
