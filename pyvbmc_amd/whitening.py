"""Input warping (rotoscaling) with the point work on the device: the reference's ``pyvbmc/whitening``
(whitening/whitening.py: ``unscent_warp`` :7-77, ``warp_input`` :80-243, ``warp_gp_and_vp`` :246-375).

A warp is the composed map "old inference space -> original space -> new inference space", ``new(old.inverse(x))``.
Everything that applies it to points -- the sigma points of the unscented transform, the training set, the search cache,
the uniform draws that locate the plausible and search boxes -- is a call into csrc/warp.hip (``vbmc_warp_points``,
``vbmc_warp_unscent``, ``vbmc_warp_gp``, ``vbmc_warp_box``) with the old transformer in the context's slot 0 and the new
one in slot 1.  What stays on the host, in NumPy:

* the whitening transform itself (the D x D covariance, its threshold and regularisation, the SVD): D <= 32, and the
  singular vectors' signs and order must be LAPACK's own, as the reference gets them;
* the (K, D) algebra that turns the warped mixture scales into ``lambd``, ``sigma`` and ``w``.

The three functions keep the reference's signatures and return values; the extras are keyword-only.  ``device=False``
runs the same code over the transformers' own host methods.  A transformer that ``transformer.transformer_fields`` does
not recognise, or D > 32, raises ``_lib.UnsupportedShape`` before anything is drawn or launched, so under
``dropin.patch_whitening`` such a call goes back to the reference's function.
"""
import copy

import numpy as np

from . import _lib
from . import transformer as _xf

FROM_OLD, FROM_ORIG, IN_NEW = 0, 1, 2  # include/vbmc_hip.h VBMC_WARP_*


class Warp:
    """``x -> new(old.inverse(x))``: the ``fun`` that ``unscent_warp`` can evaluate on the device."""

    def __init__(self, old, new):
        self.old, self.new = old, new

    def __call__(self, x):
        return self.new(self.old.inverse(x))


def _rows(a):
    return np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64)


class _HostRoute:
    """The four operations over the transformers' own methods (``device=False``)."""

    def __init__(self, old, new):
        self.old, self.new = old, new

    def map(self, x, source):
        if source == FROM_OLD:
            return self.new(self.old.inverse(x))
        return self.new(x) if source == FROM_ORIG else x

    def points(self, x, source, want_y=True, want_new=False, want_old=False):
        x = _rows(x)
        if x.shape[0] == 0:
            return (x.copy() if want_y else None, np.empty(0) if want_new else None, np.empty(0) if want_old else None)
        y = np.atleast_2d(self.map(x, source))
        return (y if want_y else None,
                np.atleast_1d(self.new.log_abs_det_jacobian(y)) if want_new else None,
                np.atleast_1d(self.old.log_abs_det_jacobian(x)) if want_old else None)

    def unscent(self, x, sigma, want_pts=False):
        m, s, p = _unscent_host(lambda z: self.map(z, FROM_OLD), x, sigma)
        return m, s, (p if want_pts else None)

    def gp(self, X, hyp):
        X, hyp = _rows(X), _rows(hyp)
        D = X.shape[1]
        logell = np.stack([np.mean(np.log(self.unscent(X, np.exp(h[:D]))[1]), axis=0) for h in hyp])
        y, dy, dy_old = self.points(X, FROM_OLD, True, True, True)
        return logell, np.mean(dy, axis=0), np.mean(dy_old, axis=0)

    def box(self, u, lo, hi, source, mode, n=None, seed=None, want_sorted=False):
        if u is None:
            raise ValueError('rng="philox" draws on the device: it needs device=True')
        y = np.atleast_2d(self.map(u * (hi - lo) + lo, source))
        out = np.quantile(y, [0.05, 0.95], axis=0) if mode == 0 else np.stack([np.min(y, axis=0), np.max(y, axis=0)])
        return (out, np.sort(y, axis=0).T) if want_sorted else out


class _DeviceRoute:
    """The same four over csrc/warp.hip: slot 0 = old, slot 1 = new."""

    def __init__(self, old, new, ctx=None):
        self._ctx = ctx
        self.old, self.new = old, new
        f = _xf.transformer_fields(new) if _xf.enabled() else None
        if f is None or (old is not None and _xf.transformer_fields(old, f[0].size) is None):
            raise _lib.UnsupportedShape("input warping on the device needs reference-shaped parameter transformers")
        self.D = f[0].size
        if self.D > 32:
            raise _lib.UnsupportedShape(f"input warping: D={self.D} > 32 not supported")

    @property
    def ctx(self):  # (looked up at the first call: a refusal above needs no device)
        if self._ctx is None:
            self._ctx = _lib.default_context()
        return self._ctx

    def _set(self):
        # (every call: the library compares with what the slot holds, and other calls on this context use slot 0 too)
        if self.old is not None:
            _xf.upload(self.old, self.ctx, 0, self.D)
        _xf.upload(self.new, self.ctx, 1, self.D)

    def points(self, x, source, want_y=True, want_new=False, want_old=False):
        x = _rows(x)
        n = x.shape[0]
        y = np.empty((n, self.D)) if want_y else None
        lj_new = np.empty(n) if want_new else None
        lj_old = np.empty(n) if want_old else None
        if n:
            self._set()
        c = self.ctx
        c.check(c._lib.vbmc_warp_points(c._h, self.D, n, source, _lib.ptr(x), _lib.ptr(y), _lib.ptr(lj_new),
                                        _lib.ptr(lj_old)))
        return y, lj_new, lj_old

    def unscent(self, x, sigma, want_pts=False):
        x, sigma = _rows(x), _rows(sigma)
        n = max(x.shape[0], sigma.shape[0])
        if x.shape[0] != n:
            x = np.ascontiguousarray(np.tile(x, (n, 1)))
        mean, sd = np.empty((n, self.D)), np.empty((n, self.D))
        pts = np.empty((2 * self.D + 1, n, self.D)) if want_pts else None
        self._set()
        c = self.ctx
        c.check(c._lib.vbmc_warp_unscent(c._h, self.D, n, _lib.ptr(x), sigma.shape[0], _lib.ptr(sigma), _lib.ptr(mean),
                                         _lib.ptr(sd), _lib.ptr(pts)))
        return mean, sd, pts

    def gp(self, X, hyp):
        X, hyp = _rows(X), _rows(hyp)
        S, P = hyp.shape
        logell, dy, dy_old = np.empty((S, self.D)), np.empty(1), np.empty(1)
        self._set()
        c = self.ctx
        c.check(c._lib.vbmc_warp_gp(c._h, self.D, X.shape[0], S, P, _lib.ptr(X), _lib.ptr(hyp), _lib.ptr(logell),
                                    _lib.ptr(dy), _lib.ptr(dy_old)))
        return logell, dy[0], dy_old[0]

    def box(self, u, lo, hi, source, mode, n=None, seed=None, want_sorted=False):
        lo, hi = _lib.f64(np.ravel(lo)), _lib.f64(np.ravel(hi))
        if u is not None:
            u = _rows(u)
            n = u.shape[0]
        out = np.empty((2, self.D))
        srt = np.empty((self.D, n)) if want_sorted else None
        self._set()
        c = self.ctx
        c.check(c._lib.vbmc_warp_box(c._h, self.D, int(n), source, _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(u),
                                     int(seed or 0), mode, _lib.ptr(out), _lib.ptr(srt)))
        return (out, srt) if want_sorted else out


def _route(device, ctx, old, new):
    return _DeviceRoute(old, new, ctx) if device else _HostRoute(old, new)


def _check_unscent_shapes(x, sigma):
    n1, d1 = x.shape
    n2, d2 = sigma.shape
    n = max(n1, n2)
    if n1 not in (1, n) or n2 not in (1, n):
        raise ValueError("Mismatch between rows of X and SIGMA.")
    if d1 != d2:
        raise ValueError("Mismatch between columns of X and SIGMA.")
    return n, d1


def _unscent_host(fun, x, sigma):
    """The unscented transform of any warp ``fun``, in NumPy: 2 D + 1 sigma points per row, warped in one call."""
    x, sigma = np.atleast_2d(x), np.atleast_2d(sigma)
    n, D = _check_unscent_shapes(x, sigma)
    U = 2 * D + 1
    pts = np.tile(np.broadcast_to(x, (n, D)), (U, 1, 1)).astype(np.float64)
    step = np.sqrt(D) * np.broadcast_to(sigma, (n, D))
    for d in range(D):
        pts[2 * d + 1, :, d] = pts[2 * d + 1, :, d] + step[:, d]
        pts[2 * d + 2, :, d] = pts[2 * d + 2, :, d] - step[:, d]
    warped = np.reshape(fun(np.reshape(pts, (n * U, D))), (U, n, D))
    return np.mean(warped, axis=0), np.std(warped, axis=0, ddof=1), warped


def unscent_warp(fun, x, sigma, *, device=True, ctx=None):
    """The reference's ``unscent_warp`` (:7-77).  On the device ``fun`` is a ``Warp`` (its two transformers go to the
    context's slots); with ``device=False`` any callable is evaluated on the host."""
    shape = np.shape(x)
    x2, s2 = np.atleast_2d(x), np.atleast_2d(sigma)
    _check_unscent_shapes(x2, s2)
    if device:
        if not isinstance(fun, Warp):
            raise _lib.UnsupportedShape("unscent_warp on the device takes a whitening.Warp(old, new), not a bare callable")
        mean, sd, pts = _DeviceRoute(fun.old, fun.new, ctx).unscent(x2, s2, want_pts=True)
    else:
        mean, sd, pts = _unscent_host(fun, x2, s2)
    return mean.reshape(shape), sd.reshape(shape), pts


def _temperature(optim_state):
    return optim_state["temperature"] if optim_state.get("temperature") else 1


def _rotoscale(vp, pt, optim_state, options):
    """The whitening transform of the posterior's covariance (:126-163): R_mat and scale.  Host NumPy on a D x D matrix:
    the singular vectors' signs and order have to be the reference's own LAPACK result, so this does not go to the
    device."""
    D = vp.D
    _, cov = vp.moments(orig_flag=False, cov_flag=True)
    R = np.eye(D) if pt.R_mat is None else pt.R_mat
    scale = np.ones(D) if pt.scale is None else pt.scale
    # back to the unrotated, unscaled, uncentred coordinates
    cov = R @ np.diag(scale) @ cov @ np.diag(scale) @ R.T
    cov = np.diag(pt.delta) @ cov @ np.diag(pt.delta)
    thresh = options["warp_roto_corr_thresh"]
    if thresh > 0:
        corr = cov / np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
        cov[np.abs(corr) <= thresh] = 0
    reg = options["warp_cov_reg"]
    if not np.isscalar(reg):
        reg = reg[optim_state["N"]]
    reg = np.max([0, np.min([1, reg])])
    cov = (1 - reg) * cov + reg * np.diag(np.diag(cov))
    U, s, _ = np.linalg.svd(cov)
    if np.linalg.det(U) < 0:
        U[:, 0] = -U[:, 0]
    return U, np.sqrt(s + np.finfo(np.float64).eps)


def warp_input(vp, optim_state, function_logger, options, *, device=True, ctx=None, rng="numpy", seed=None,
               n_plausible=100000, n_search=1000):
    """The reference's ``warp_input`` (:80-243): the new transformer, and deep copies of ``optim_state`` and
    ``function_logger`` moved into its inference space.

    ``rng="numpy"`` takes the two box samples from ``np.random.rand`` exactly as the reference does (two calls, the same
    shapes and order, so a seeded global stream ends in the same state) and uploads them; ``rng="philox"`` draws them on
    the device under ``seed`` (drawn from ``np.random`` when None).  ``n_plausible`` / ``n_search`` are the reference's
    two hard-coded sample sizes."""
    if rng not in ("numpy", "philox"):
        raise ValueError(f"unknown rng {rng!r}")
    pt = copy.deepcopy(vp.parameter_transformer)
    optim_state = copy.deepcopy(optim_state)
    function_logger = copy.deepcopy(function_logger)
    if options.get("warp_nonlinear"):
        raise NotImplementedError("Non-linear warping is not supported.")
    D = vp.D
    route = _route(device, ctx, vp.parameter_transformer, pt)  # (refuses before anything is drawn)
    if options.get("warp_rotoscaling"):
        pt.R_mat, pt.scale = _rotoscale(vp, pt, optim_state, options)
    pt.mu = np.zeros(D)
    pt.delta = np.ones(D)
    if rng == "philox":
        seed = int(np.random.randint(0, 2**62, dtype=np.int64)) if seed is None else int(seed)

    # plausible bounds: the 0.05 / 0.95 quantiles of the plausible box's image, widened by a ninth of their span
    u = np.random.rand(n_plausible, D) if rng == "numpy" else None
    q = route.box(u, np.ravel(optim_state["plb_orig"]), np.ravel(optim_state["pub_orig"]), FROM_ORIG, 0, n=n_plausible,
                  seed=seed)
    span = q[1] - q[0]
    optim_state["plb_tran"] = (q[0] - span / 9).reshape((1, D))
    optim_state["pub_tran"] = (q[1] + span / 9).reshape((1, D))

    # the training set: new coordinates, and the log-Jacobian (tempered) onto the values
    T = _temperature(optim_state)
    flag = function_logger.X_flag
    y_orig = function_logger.y_orig[flag].T
    X, dy, _ = route.points(function_logger.X_orig[flag, :], FROM_ORIG, True, True, False)
    function_logger.X[flag, :] = X
    function_logger.y[flag] = (y_orig + dy / T).T
    function_logger.parameter_transformer = pt

    # search bounds: minimum and maximum of the search box's image, widened by 1 / n_search of their span
    u = np.random.rand(n_search, D) if rng == "numpy" else None
    mm = route.box(u, np.ravel(optim_state["lb_search"]), np.ravel(optim_state["ub_search"]), FROM_OLD, 1, n=n_search,
                   seed=None if seed is None else seed + 1)
    span = mm[1] - mm[0]
    optim_state["lb_search"] = np.atleast_2d(mm[0] - span / n_search)
    optim_state["ub_search"] = np.atleast_2d(mm[1] + span / n_search)

    # (a non-empty cache of any kind: the reference's truth test fails on an array of several rows)
    cache = optim_state.get("search_cache")
    if cache is not None and np.size(cache) > 0:
        optim_state["search_cache"] = route.points(cache, FROM_OLD)[0]

    optim_state["recompute_var_post"] = True
    optim_state["skip_active_sampling"] = True
    optim_state["warping_count"] += 1
    optim_state["last_warping"] = optim_state["iter"]
    optim_state["last_successful_warping"] = optim_state["iter"]
    optim_state["run_mean"] = []
    optim_state["run_cov"] = []
    optim_state["last_run_avg"] = np.nan
    return pt, optim_state, function_logger, "rotoscale"


def warp_gp_and_vp(parameter_transformer, gp_old, vp_old, vbmc, *, device=True, ctx=None):
    """The reference's ``warp_gp_and_vp`` (:246-375): the GP hyper-parameters (S, P) and a copy of the posterior pushed
    through the warp by the unscented transform.  One ``vbmc_warp_gp`` call serves all hyper-parameter samples."""
    vp_old = copy.deepcopy(vp_old)
    old = vp_old.parameter_transformer
    kind = type(gp_old.mean).__name__  # (by class name, as gp.mean_kind_of: ours, gpyreg's, a stand-in)
    if kind not in ("ConstantMean", "NegativeQuadratic"):
        raise ValueError("Unsupported GP mean function for input warping.")
    route = _route(device, ctx, old, parameter_transformer)
    T = _temperature(vbmc.optim_state)
    D = vbmc.D
    o = gp_old.covariance.hyperparameter_count(D) + gp_old.noise.hyperparameter_count()  # the mean's first entry

    hyp = np.array([np.ravel(p.hyp) for p in gp_old.posteriors], dtype=np.float64)
    hyp_warped = hyp.copy()
    logell, dy_mean, dy_old_mean = route.gp(gp_old.X, hyp)
    hyp_warped[:, :D] = logell
    if kind == "ConstantMean":
        hyp_warped[:, o] = hyp[:, o] + (dy_mean - dy_old_mean) / T
    else:
        xm, omega = hyp[:, o + 1:o + 1 + D], np.exp(hyp[:, o + 1 + D:o + 1 + 2 * D])
        xmw, omegaw, _ = route.unscent(xm, omega)
        dy_old = route.points(xm, FROM_OLD, False, False, True)[2]
        dy = route.points(xmw, IN_NEW, False, True, False)[1]
        hyp_warped[:, o] = hyp[:, o] + (dy - dy_old) / T
        hyp_warped[:, o + 1:o + 1 + D] = xmw
        hyp_warped[:, o + 1 + D:o + 1 + 2 * D] = np.log(omegaw)

    vp = copy.deepcopy(vp_old)
    vp.parameter_transformer = copy.deepcopy(parameter_transformer)
    mu = vp.mu.T
    muw, slw, _ = route.unscent(mu, (vp_old.lambd * vp_old.sigma).T)
    vp.mu = muw.T
    # (K, D) algebra, host: lambda from the per-dimension share of the squared scales, sigma as the geometric mean
    lambdaw = np.sqrt(D * np.mean((slw**2).T / np.sum(slw**2, axis=1), axis=1)).T
    vp.lambd[:, 0] = lambdaw
    vp.sigma[0, :] = np.exp(np.mean(np.log(slw / lambdaw), axis=1))
    dy_old = route.points(mu, FROM_OLD, False, False, True)[2]
    dy = route.points(muw, IN_NEW, False, True, False)[1]
    ww = vp_old.w * np.exp((dy - dy_old) / T)
    vp.w = ww / np.sum(ww)
    return vp, hyp_warped


__all__ = ["Warp", "unscent_warp", "warp_input", "warp_gp_and_vp", "FROM_OLD", "FROM_ORIG", "IN_NEW"]
