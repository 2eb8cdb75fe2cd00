"""The cases and the raw calls of the fused GP fit's tests (``vbmc_gp_fit``, pyvbmc_amd/csrc/api_gp_fit.hip;
``GP.fit(optimizer="fused")``).  TEST INFRASTRUCTURE shared by tests/test_gp_fit_gpu.py, tests/test_gp_fit_host.py and
the train_gp tests.

The problems are tests/gp_opt_host.py's cases that straddle the 64-row block: 63 (N = 63, D = 3, constant mean, user
noise) and 130 (N = 130, D = 2, zero mean).  Case 65 is left out for the reason tests/test_gp_opt_host.py gives (several
optima).  The fit's shape: H = 3 rows of hyp0, 37 drawn candidates (40 in all: three chunks of 16 with a ragged last
one), 3 optimiser runs, 4 chains of thin 2 after 3 burn-in sweeps."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import gp_opt_host as goh

KEYS = (63, 130)
H, INIT_N, OPTS_N, N_SAMPLES, THIN, BURN = 3, 37, 3, 4, 2, 3
SEED = 0x5EED0F17
WIDTH = 0.6
CHUNK = 16


def design_box(cs):
    """A design box strictly inside the hard box: the middle half of every parameter's range."""
    q = 0.25 * (cs.ub - cs.lb)
    return cs.lb + q, cs.ub - q


def philox_bits53(c0, c1, c2, c3, seed):
    """Philox4x32-10 on counter (c0, c1, c2, c3) under the 64-bit key ``seed``; the upper 53 bits of words 0, 1: a
    restatement of its own, from the published constants."""
    m = 0xFFFFFFFF
    k0, k1 = seed & m, (seed >> 32) & m
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & m, (p0 >> 32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return ((c0 << 32) | c1) >> 11


def design_rows(init_N, dlb, dub, seed):
    """The drawn rows by the rule the header states: block (p, 0, j, 10), u = bits 2^-53, dlb + (dub - dlb) u, clipped."""
    out = np.empty((init_N, dlb.size))
    for j in range(init_N):
        for p in range(dlb.size):
            u = float(philox_bits53(p, 0, j, 10, seed)) * 2.0**-53
            out[j, p] = min(max(dlb[p] + (dub[p] - dlb[p]) * u, dlb[p]), dub[p])
    return out


def raw_fit(ctx, cs, *, hyp0=None, init_N=INIT_N, opts_N=OPTS_N, n_samples=N_SAMPLES, thin=THIN, burn=BURN, seed=SEED, lb=None,
            ub=None, dlb=None, dub=None, max_iter=None, m=None, tol_g=None, tol_f=None, widths=None, want_post=True, mean=None,
            no_s2=False):
    """The entry point itself on a case: a namespace of ``rc`` and every output."""
    from pyvbmc_amd import _lib

    X, y = _lib.f64(cs.X), _lib.f64(np.ravel(cs.y))
    N, D = X.shape
    P = cs.P
    hyp0 = cs.x0[:H] if hyp0 is None else hyp0
    hyp0 = _lib.f64(np.reshape(hyp0, (-1, P)))
    nH = hyp0.shape[0]
    B = max(nH + max(init_N, 0), 1)
    R, S = max(min(opts_N, B), 0), max(n_samples, 1)
    s2 = None if cs.s2 is None or no_s2 else _lib.f64(np.ravel(cs.s2))
    lb, ub = _lib.f64(cs.lb if lb is None else lb), _lib.f64(cs.ub if ub is None else ub)
    box = design_box(cs)
    dlb, dub = _lib.f64(box[0] if dlb is None else dlb), _lib.f64(box[1] if dub is None else dub)
    pri = [_lib.f64(cs.priors[k]) for k in ("mu", "sigma", "df")]
    widths = _lib.f64(np.full(P, WIDTH) if widths is None else widths)
    o = SimpleNamespace(
        cand=np.full((B, P), 7.0), score=np.full(B, 7.0), starts=np.full(R, 7, dtype=np.int32), o_hyp=np.full((R, P), 7.0),
        o_lp=np.full(R, 7.0), o_stats=np.full((R, 4), 7, dtype=np.int64), o_inv=np.full(R, 7, dtype=np.int32),
        best=np.full(P, 7.0), best_lp=np.full(1, 7.0), hyp=np.full((S, P), 7.0), lpost=np.full(S, 7.0), lprior=np.full(S, 7.0),
        stats=np.full((S, 4), 7, dtype=np.int64), noise=np.full(S, 7.0), status=np.full(1, 7, dtype=np.int32),
        alpha=np.full((S, N), 7.0) if want_post else None, L=np.full((S, N, N), 7.0) if want_post else None)
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    o.rc = ctx._lib.vbmc_gp_fit(
        ctx._h, N, D, P, cs.mean if mean is None else mean, _lib.ptr(X), _lib.ptr(y), _lib.ptr(s2), nH,
        _lib.ptr(hyp0) if nH else None, init_N, _lib.ptr(dlb), _lib.ptr(dub), _lib.ptr(lb), _lib.ptr(ub),
        *[_lib.ptr(a) for a in pri], opts_N, cs.max_iter if max_iter is None else max_iter, cs.m if m is None else m,
        cs.tol_g if tol_g is None else tol_g, cs.tol_f if tol_f is None else tol_f, n_samples, _lib.ptr(widths), thin, burn,
        C.c_uint64(seed), _lib.ptr(o.cand), _lib.ptr(o.score), o.starts.ctypes.data_as(i32), _lib.ptr(o.o_hyp), _lib.ptr(o.o_lp),
        o.o_stats.ctypes.data_as(i64), o.o_inv.ctypes.data_as(i32), _lib.ptr(o.best), _lib.ptr(o.best_lp), _lib.ptr(o.hyp),
        _lib.ptr(o.lpost), _lib.ptr(o.lprior), o.stats.ctypes.data_as(i64), _lib.ptr(o.noise), o.status.ctypes.data_as(i32),
        _lib.ptr(o.alpha), _lib.ptr(o.L))
    return o


OUTPUTS = ("cand", "score", "starts", "o_hyp", "o_lp", "o_stats", "o_inv", "best", "best_lp", "hyp", "lpost", "lprior", "stats",
           "noise", "status", "alpha", "L")


def same_fit(a, b):
    return a.rc == b.rc and all(np.array_equal(getattr(a, k), getattr(b, k)) for k in OUTPUTS)


def raw_sample(ctx, cs, x0, *, thin=THIN, burn=BURN, seed=SEED, widths=None):
    """vbmc_gp_hyp_sample on a case, n = 1: ``(rc, samples (C, P), log_post, log_prior, stats, invalid)``."""
    from pyvbmc_amd import _lib

    X, y = _lib.f64(cs.X), _lib.f64(np.ravel(cs.y))
    N, D = X.shape
    x0 = _lib.f64(np.atleast_2d(x0))
    Cn, P = x0.shape
    s2 = None if cs.s2 is None else _lib.f64(np.ravel(cs.s2))
    arr = [_lib.f64(np.full(P, WIDTH) if widths is None else widths), _lib.f64(cs.lb), _lib.f64(cs.ub)]
    arr += [_lib.f64(cs.priors[k]) for k in ("mu", "sigma", "df")]
    smp, lpost, lprior = np.full((Cn, 1, P), 7.0), np.full((Cn, 1), 7.0), np.full((Cn, 1), 7.0)
    stats, inv = np.full((Cn, 4), 7, dtype=np.int64), np.full(Cn, 7, dtype=np.int32)
    rc = ctx._lib.vbmc_gp_hyp_sample(ctx._h, N, D, P, cs.mean, _lib.ptr(X), _lib.ptr(y), _lib.ptr(s2), Cn, _lib.ptr(x0),
                                     *[_lib.ptr(a) for a in arr], 1, thin, burn, C.c_uint64(seed), _lib.ptr(smp),
                                     _lib.ptr(lpost), _lib.ptr(lprior), stats.ctypes.data_as(C.POINTER(C.c_int64)),
                                     inv.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, smp[:, 0, :], lpost[:, 0], lprior[:, 0], stats, inv


def raw_posterior(ctx, cs, hyp, noise):
    """vbmc_gp_posterior at ``hyp`` with the noise the fit reports: sn2 = noise + s2, sn2_div = noise + min s2."""
    from pyvbmc_amd import _lib

    X, y = _lib.f64(cs.X), _lib.f64(np.ravel(cs.y))
    N, D = X.shape
    hyp = _lib.f64(np.atleast_2d(hyp))
    S, P = hyp.shape
    s2 = np.zeros(N) if cs.s2 is None else np.ravel(cs.s2)
    sn2 = _lib.f64(noise[:, None] + s2[None, :]) if cs.s2 is not None else _lib.f64(np.repeat(noise[:, None], N, axis=1))
    div = _lib.f64(noise + (np.min(s2) if cs.s2 is not None else 0.0))
    alpha, L = np.full((S, N), 7.0), np.full((S, N, N), 7.0)
    rc = ctx._lib.vbmc_gp_posterior(ctx._h, N, D, S, P, cs.mean, _lib.ptr(X), _lib.ptr(y), _lib.ptr(sn2), _lib.ptr(div),
                                    _lib.ptr(hyp), _lib.ptr(alpha), _lib.ptr(L))
    return rc, alpha, L


def make_gp(ctx, cs):
    """The package's GP for a case, holding its data (``ctx`` None: no device)."""
    from oracle import gp_ref
    from pyvbmc_amd import gp as gpm

    cls = {gp_ref.MEAN_ZERO: gpm.ZeroMean, gp_ref.MEAN_CONST: gpm.ConstantMean, gp_ref.MEAN_NEGQUAD: gpm.NegativeQuadratic}
    gp = gpm.GP(cs.X.shape[1], gpm.SquaredExponential(), cls[cs.mean](),
                gpm.GaussianNoise(constant_add=True, user_provided_add=cs.s2 is not None))
    gp.ctx = ctx
    gp.X, gp.y = np.array(cs.X, dtype=np.float64), np.array(cs.y, dtype=np.float64).reshape(-1, 1)
    gp.s2 = None if cs.s2 is None else np.array(cs.s2, dtype=np.float64).reshape(-1, 1)
    return gp


def fit_package(ctx, cs, device, optimizer="fused", **options):
    """``GP.fit`` on a case through the package: ``(gp, hyp, optimize_result, sample_result)``."""
    opts = {"init_N": INIT_N, "opts_N": OPTS_N, "n_samples": N_SAMPLES, "thin": THIN, "burn": BURN, "widths": np.full(cs.P, WIDTH),
            "tol_opt": 1e-4}
    if optimizer == "fused":
        opts["design_lb"], opts["design_ub"] = design_box(cs)
    opts.update(options)
    gp = make_gp(ctx, cs)
    gp.set_bounds({"lb": cs.lb, "ub": cs.ub})
    gp.set_priors(cs.priors)
    return (gp,) + gp.fit(cs.X, cs.y, cs.s2, hyp0=cs.x0[:H], options=opts, device=device, seed=SEED, optimizer=optimizer)


def case(key):
    return goh.case(key)
