"""GP container for the ELBO path: the subset of ``gpyreg.GP`` PyVBMC touches on it.

gpyreg is a third-party dependency of the reference that is not part of its tree
(`gpyreg >= 0.1.0`, /root/reference/pyproject.toml:13).  What PyVBMC needs from it
on this path is (a) the posterior record per hyper-parameter
sample -- ``posteriors[s].{hyp, alpha, sW, L, sn2_mult, L_chol}`` -- and (b)
``predict``.  This module provides a duck-type with the same attribute/method
names so the hot-path functions accept either it or a real ``gpyreg.GP``:

* ``update(X_new, y_new, s2_new, hyp)`` builds the posterior records on the host.
  That is the O(N^3) Cholesky done ONCE per GP fit -- an input of the path
  (SURVEY 8a row a11), not part of it; hyper-parameter fitting itself (slice
  sampling) is out of scope.
* ``predict`` runs on the MI355X (vbmc_gp_predict).
* ``update(..., device=True)``, ``append`` and ``device_posterior`` build the same records on the device instead
  (vbmc_gp_posterior / vbmc_gp_append: batched FP64 Cholesky, one-point append) and leave them installed there, so
  the ``upload_gp`` that follows ships nothing.  Opt-in: the default path and its bits are unchanged.
* ``log_marginal_likelihood`` / ``GP.log_likelihood``: the objective of hyper-parameter fitting and its gradient for a
  batch of candidates on the device (vbmc_gp_lml), with a NumPy / SciPy host route of the same formulas.  The fitting
  loop itself (optimiser, slice sampler, priors) stays with the caller.
"""
import ctypes as C
import sys
from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla

from . import _lib


class SquaredExponential:
    """SE-ARD: k(a,b) = sf^2 exp(-1/2 sum_d ((a_d-b_d)/ell_d)^2); hyp = [log ell (D), log sf]."""

    def hyperparameter_count(self, D):
        return D + 1

    def compute(self, hyp, X, X_star=None):
        X = np.atleast_2d(X)
        Xs = X if X_star is None else np.atleast_2d(X_star)
        D = X.shape[1]
        ell = np.exp(hyp[:D])
        d2 = np.zeros((X.shape[0], Xs.shape[0]))
        for d in range(D):
            d2 += ((X[:, d] / ell[d])[:, None] - (Xs[:, d] / ell[d])[None, :]) ** 2
        return np.exp(2 * hyp[D]) * np.exp(-0.5 * d2)


class ZeroMean:
    kind = _lib.MEAN_ZERO

    def hyperparameter_count(self, D):
        return 0

    def compute(self, hyp, X):
        return np.zeros(X.shape[0])


class ConstantMean:
    kind = _lib.MEAN_CONST

    def hyperparameter_count(self, D):
        return 1

    def compute(self, hyp, X):
        return np.full(X.shape[0], hyp[0])


class NegativeQuadratic:
    """m(x) = m0 - 1/2 sum_d ((x_d - xm_d)/omega_d)^2; hyp = [m0, xm (D), log omega (D)]
    (layout used at variational_optimization.py:1383-1392)."""

    kind = _lib.MEAN_NEGQUAD

    def hyperparameter_count(self, D):
        return 1 + 2 * D

    def compute(self, hyp, X):
        D = X.shape[1]
        return hyp[0] - 0.5 * np.sum(((X - hyp[1 : 1 + D]) / np.exp(hyp[1 + D : 1 + 2 * D])) ** 2, 1)


class GaussianNoise:
    def __init__(self, constant_add=False, user_provided_add=False, scale_user_provided=False,
                 rectified_linear_output_dependent_add=False):
        if scale_user_provided or rectified_linear_output_dependent_add:
            raise NotImplementedError("only constant and user-provided additive noise are supported")
        self.constant_add = constant_add
        self.user_provided_add = user_provided_add

    def hyperparameter_count(self):
        return 1

    def compute(self, hyp, X, y=None, s2=None):
        sn2 = np.full((X.shape[0], 1), np.exp(2 * hyp[0]) if self.constant_add else np.spacing(1.0))
        if self.user_provided_add and s2 is not None:
            sn2 = sn2 + np.reshape(s2, (-1, 1))
        return sn2


_MEAN_KINDS = {"ZeroMean": _lib.MEAN_ZERO, "ConstantMean": _lib.MEAN_CONST,
               "NegativeQuadratic": _lib.MEAN_NEGQUAD}


def mean_kind_of(gp):
    """Mean-function kind of a GP duck type (ours or a real gpyreg.GP), by class name."""
    name = type(gp.mean).__name__
    if name not in _MEAN_KINDS:
        raise NotImplementedError(f"mean function {name} is not supported on the ELBO path")
    return _MEAN_KINDS[name]


class _ChecksumPlan:
    """The data pointers of every posterior's ``alpha`` and ``hyp`` (float64, contiguous), laid out
    for ONE library call that checksums all of them (vbmc_host_checksum).  Built when the identities
    of those arrays change and reused while they stay the same -- the objects are held, so an
    unchanged ``id`` is the same array with the same buffer."""

    __slots__ = ("ids", "held", "ptrs", "lens", "n", "out", "slow", "fn")

    def __init__(self, ids, held, arrays):
        self.ids, self.held = ids, held
        fast = [a for a in arrays if isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] and a.size > 0]
        self.slow = [a for a in arrays if not any(a is f for f in fast)]  # other dtypes / layouts: hashed through a copy
        self.n = len(fast)
        self.ptrs = (C.c_void_p * max(self.n, 1))(*[a.ctypes.data for a in fast])
        self.lens = (C.c_int64 * max(self.n, 1))(*[a.size for a in fast])
        self.out = C.c_uint64()
        self.fn = _lib.load().vbmc_host_checksum

    def checksum(self):
        self.fn(self.ptrs, self.lens, self.n, self.out)
        v = self.out.value
        for a in self.slow:
            v ^= hash(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        return v


def _gp_ids(gp):
    """The identity half of the GP key: ids of X, of the posteriors array, of every record and of its
    alpha / L / hyp arrays, and the end elements of X and L."""
    ps, X = gp.posteriors, gp.X
    ids = [id(ps), id(X), X.shape[0]]
    tail = [X.item(0), X.item(-1)]
    for p in ps:
        L = p.L
        ids += (id(p), id(p.alpha), id(L), id(p.hyp))
        # (L = None: a record whose factor stayed on the device -- ``device_posterior(fetch=False)``; its identity,
        # already in ``ids``, is the key)
        tail += (L.item(-1) if L is not None else None, p.L_chol)
    return ids, tail


def _gp_plan(gp, ctx, ids):
    plan = getattr(ctx, "_gp_ck", None) if ctx is not None else None
    if plan is None or plan.ids != ids:
        ps = gp.posteriors
        held, arrays = [ps, gp.X], []
        for p in ps:
            held += (p, p.alpha, p.L, p.hyp)
            arrays += (p.alpha, p.hyp)
        plan = _ChecksumPlan(ids, held, arrays)
        if ctx is not None:
            ctx._gp_ck = plan
    return plan


def _gp_fingerprint(gp, ctx=None):
    """State key of a GP duck type: identities of X, of the posteriors array, of every posterior
    record and of its alpha / L / hyp arrays, the end elements of X and L, and a checksum of EVERY
    element of every alpha and hyp.  It catches what the reference does to a GP between two calls
    -- ``gp.posteriors[s] = ...`` (active_importance_sampling.py:207-209), attribute re-binding,
    ``gp.X`` replaced or extended by ``gp.update`` (active_sample.py:584) -- and any in-place edit
    of alpha or hyp (alpha = (K + Sigma)^-1 (y - m) changes whenever anything about the GP does).
    An in-place edit of X or of the interior of L that leaves alpha untouched still needs
    ``invalidate_gp``.  ~2 us at S = 1, ~5 us at S = 8, N = 800 (one library call checksums all
    the arrays: 55 KB there); the optimiser's inner loop does not pay it up front (``upload_gp``
    with ``lazy``)."""
    ids, tail = _gp_ids(gp)
    plan = _gp_plan(gp, ctx, ids)
    return ids + tail + [plan.checksum()], plan.held


def invalidate_gp(ctx=None):
    """Forget the GP the context holds: the next call uploads it again.  Only needed after
    editing GP arrays in place in a way the fingerprint cannot see (see ``_gp_fingerprint``)."""
    ctx = _lib.default_context() if ctx is None else ctx
    ctx._gp_key = ctx._gp_ref = ctx._gp_ck = ctx._gp_quick = ctx._gp_dev = None
    vo = sys.modules.get(__package__ + ".variational_optimization")
    if vo is not None:
        vo.clear_fast_path()


def upload_gp(gp, ctx, lazy=False):
    """Ship X and the posterior records of ``gp`` to the context (skipped while the GP's
    fingerprint is the one already uploaded).

    ``lazy`` (the fused objective only): when identities and end elements are unchanged the
    checksum of the arrays' contents is NOT taken here -- ``vbmc_neg_elcbo`` takes it itself after it
    has released its launches, while the device works (vbmc_set_gp_watch), and answers
    ``W_GP_CHANGED`` if an array was edited in place; the caller then uploads and evaluates again.
    The test stays complete, its cost moves off the path between two evaluations."""
    if lazy:
        # identities of what the watch covers (alpha, hyp of every record) and of the containers; L and the
        # end elements are part of the full key only -- L never changes without alpha changing
        ps, X = gp.posteriors, gp.X
        quick = [id(ps), id(X), X.shape[0]]
        for p in ps:
            quick += (id(p), id(p.alpha), id(p.hyp))
        if quick == getattr(ctx, "_gp_quick", None):
            return
    ids, tail = _gp_ids(gp)
    plan = _gp_plan(gp, ctx, ids)
    key = ids + tail + [plan.checksum()]
    if getattr(ctx, "_gp_key", None) == key:
        return
    ctx._gp_quick = None
    posts = list(gp.posteriors)
    if any(p.L is None for p in posts):
        # records of a device-built posterior whose L was not fetched, and the context holds something else by now:
        # built again on the device from X, y, hyp (bit-reproducible: the records' alpha stays what it is)
        if _device_build(gp, np.stack([np.ravel(p.hyp) for p in posts]), ctx, want_L=False) is None:
            raise ValueError("upload_gp: posterior records without L that the device cannot rebuild")
        _adopt(gp, ctx, dev=True)
        return
    X = _lib.f64(gp.X)
    N, D = X.shape
    S = len(posts)
    hyp = _lib.f64(np.stack([np.ravel(p.hyp) for p in posts]))
    alpha = _lib.f64(np.stack([np.ravel(p.alpha) for p in posts]))
    L = _lib.f64(np.stack([np.asarray(p.L) for p in posts]))
    sW = _lib.f64(np.stack([np.ravel(p.sW) * np.ones(N) for p in posts]))
    chol = np.ascontiguousarray([1 if p.L_chol else 0 for p in posts], dtype=np.int32)
    mult = _lib.f64([float(getattr(p, "sn2_mult", 1.0)) for p in posts])
    ctx._gp_key = ctx._gp_quick = None
    ctx.check(
        ctx._lib.vbmc_set_gp(
            ctx._h, N, D, S, hyp.shape[1], mean_kind_of(gp), _lib.ptr(X), _lib.ptr(hyp),
            _lib.ptr(alpha), _lib.ptr(L), chol.ctypes.data_as(C.POINTER(C.c_int32)), _lib.ptr(sW),
            _lib.ptr(mult),
        )
    )
    # the held references keep every fingerprinted object alive, so an id cannot be recycled (and the
    # watched buffers stay allocated)
    ctx._gp_dev = None
    _keyed(gp, ctx, key, plan)


def _keyed(gp, ctx, key, plan):
    """Record that the context holds ``gp`` under ``key`` and have the library watch the arrays' contents."""
    ctx._gp_key, ctx._gp_ref = key, plan.held
    if not plan.slow and plan.n > 0:
        ctx.check(ctx._lib.vbmc_set_gp_watch(ctx._h, plan.ptrs, plan.lens, plan.n, C.c_uint64(key[-1])))
        quick = [id(gp.posteriors), id(gp.X), gp.X.shape[0]]
        for p in gp.posteriors:
            quick += (id(p), id(p.alpha), id(p.hyp))
        ctx._gp_quick = quick  # (set only while the library watches the arrays' contents)


def _adopt(gp, ctx, dev):
    """Key the context to ``gp`` as it stands, after a call that installed its posterior there itself; ``dev``: the
    state was built on the device (``GP.append`` may extend it)."""
    ctx._gp_key = ctx._gp_quick = None
    ids, tail = _gp_ids(gp)
    plan = _gp_plan(gp, ctx, ids)
    key = ids + tail + [plan.checksum()]
    _keyed(gp, ctx, key, plan)
    ctx._gp_dev = key if dev else None


def _noise_var(gp, hyp_noise):
    """Noise variance per training point for one sample, as ``GP._posterior`` takes it: the GP's own noise function
    where it has one, else constant noise exp(2 hyp) plus the user-provided ``s2`` where the GP carries it."""
    X = np.atleast_2d(gp.X)
    s2 = getattr(gp, "s2", None)
    noise = getattr(gp, "noise", None)
    if noise is not None and hasattr(noise, "compute"):
        return np.asarray(noise.compute(hyp_noise, X, gp.y, s2), dtype=np.float64).ravel() * np.ones(X.shape[0])
    sn2 = np.full(X.shape[0], np.exp(2 * hyp_noise[0]))
    if s2 is not None and np.size(s2):
        sn2 = sn2 + np.reshape(s2, -1)
    return sn2


def _device_build(gp, hyp, ctx, want_L):
    """vbmc_gp_posterior for a GP duck type: ``(alpha (S, N), L (S, N, N) or None, sn2_div (S))``, or None when the
    device route does not apply (a sample on the non-Cholesky branch, VBMC_E_UNSUP) and the caller takes the host path.
    Raises ``numpy.linalg.LinAlgError`` when a sample is not positive definite (the context's GP is then unchanged)."""
    X = _lib.f64(np.atleast_2d(gp.X))
    y = _lib.f64(np.ravel(gp.y))
    N, D = X.shape
    hyp = _lib.f64(np.atleast_2d(hyp))
    S, P = hyp.shape
    sn2 = _lib.f64(np.stack([_noise_var(gp, h[D + 1 : D + 2]) for h in hyp]))
    sn2_div = _lib.f64(np.min(sn2, axis=1))
    sn2_mult = 1.0
    if not np.all(sn2_div * sn2_mult >= 1e-6):
        return None
    alpha = np.empty((S, N))
    L = np.empty((S, N, N)) if want_L else None
    rc = ctx._lib.vbmc_gp_posterior(ctx._h, N, D, S, P, mean_kind_of(gp), _lib.ptr(X), _lib.ptr(y), _lib.ptr(sn2),
                                    _lib.ptr(sn2_div), _lib.ptr(hyp), _lib.ptr(alpha), _lib.ptr(L))
    if rc == _lib.E_UNSUP:
        return None
    ctx.check(rc)
    return alpha, L, sn2_div


def _records(hyp, alpha, L, sW0):
    posts = np.empty(len(hyp), dtype=object)
    N = alpha.shape[1]
    for s in range(len(hyp)):
        posts[s] = SimpleNamespace(hyp=np.array(hyp[s], dtype=np.float64), alpha=alpha[s].reshape(-1, 1).copy(),
                                   sW=np.ones(N) * sW0[s], L=None if L is None else L[s], sn2_mult=1.0, L_chol=True)
    return posts


def device_posterior(gp, hyp=None, *, ctx=None, fetch=True):
    """Build the posterior records of ``gp`` on the device and leave them installed there.

    ``gp``: this package's ``GP``, an attribute-only stand-in or a real ``gpyreg.GP``; read are ``X``, ``y``, ``s2``,
    ``mean`` and ``noise``.  Noise rule: where ``gp.noise`` has a ``compute`` method it decides the noise variance per
    point; a stand-in WITHOUT a noise object gets constant noise exp(2 hyp_noise) plus ``gp.s2`` whenever ``s2`` is
    present and not empty -- so a stand-in whose records were built without user noise must not carry an ``s2``.  ``hyp`` (S, P): the hyper-parameter samples (default: those of the present records).  The
    noise scalars ``sn2``, ``sn2_div`` are computed here with ``GP._posterior``'s arithmetic; covariance, Cholesky
    factor, its inverse and ``alpha`` on the device (vbmc_gp_posterior).  Sets ``gp.posteriors`` to records
    ``hyp, alpha, sW, L, sn2_mult, L_chol`` and keys the context to them: the next ``upload_gp(gp, ctx)`` ships nothing.

    ``fetch=False``: ``alpha`` still comes back (S N doubles) but ``L`` stays on the device and the records carry
    ``L = None``; ``fetch_posteriors`` fills it in later.

    Returns True, or False -- with ``gp`` untouched -- when the device route does not apply (a sample takes the
    non-Cholesky branch): the caller then uses the host path.  ``numpy.linalg.LinAlgError`` when a sample is not
    positive definite, as ``scipy.linalg.cholesky`` raises on the host path."""
    ctx = (getattr(gp, "ctx", None) or _lib.default_context()) if ctx is None else ctx
    if hyp is None:
        hyp = np.stack([np.ravel(p.hyp) for p in gp.posteriors])
    hyp = np.atleast_2d(np.asarray(hyp, dtype=np.float64))
    out = _device_build(gp, hyp, ctx, want_L=fetch)
    if out is None:
        return False
    alpha, L, sn2_div = out
    gp.posteriors = _records(hyp, alpha, L, 1.0 / np.sqrt(sn2_div * 1.0))
    _adopt(gp, ctx, dev=True)
    return True


def fetch_posteriors(gp, ctx=None):
    """Fill in the ``L`` of records built with ``fetch=False`` from the device (vbmc_gp_fetch); the context stays keyed
    to ``gp``.  Returns ``gp.posteriors``."""
    ctx = (getattr(gp, "ctx", None) or _lib.default_context()) if ctx is None else ctx
    posts = gp.posteriors
    if all(p.L is not None for p in posts):
        return posts
    upload_gp(gp, ctx)  # (rebuilds on the device if the context holds something else by now)
    dev = getattr(ctx, "_gp_dev", None) is not None
    N = gp.X.shape[0]
    L = np.empty((len(posts), N, N))
    ctx.check(ctx._lib.vbmc_gp_fetch(ctx._h, None, _lib.ptr(L)))
    for s, p in enumerate(posts):
        if p.L is None:
            p.L = L[s]
    _adopt(gp, ctx, dev=dev)
    return posts


def _mean_and_grad(kind, hm, X):
    """m(X) (N) and dm/dtheta (mean parameters, N) of the three mean kinds."""
    N, D = X.shape
    if kind == _lib.MEAN_ZERO:
        return np.zeros(N), np.zeros((0, N))
    if kind == _lib.MEAN_CONST:
        return np.full(N, hm[0]), np.ones((1, N))
    om = np.exp(hm[1 + D : 1 + 2 * D])
    u = X - hm[1 : 1 + D]
    m = hm[0] - 0.5 * np.sum((u / om) ** 2, axis=1)
    return m, np.vstack([np.ones((1, N)), (u / om**2).T, ((u / om) ** 2).T])


def _host_lml(X, y, kind, h, sn2, sn2_div, dsn2, grad):
    """One candidate on the host with vbmc_gp_lml's formulas: ``(lml, dlml or None)``; -inf and a NaN gradient when the
    covariance does not factorise or a result is not finite.  ``sn2_div < 1e-6`` (the posterior's non-Cholesky branch):
    the factor of C = K + diag(sn2) itself, sl = 1."""
    N, D = X.shape
    P = h.size
    bad = (-np.inf, np.full(P, np.nan) if grad else None)
    with np.errstate(all="ignore"):
        ell = np.exp(h[:D])
        Xs = X / ell
        d2 = np.zeros((N, N))
        for d in range(D):
            d2 += (Xs[:, d][:, None] - Xs[:, d][None, :]) ** 2
        K = np.exp(2 * h[D]) * np.exp(-0.5 * d2)
        sl = sn2_div if sn2_div >= 1e-6 else 1.0
        A = K / sl + np.diag(sn2 / sl)
        m, dm = _mean_and_grad(kind, h[D + 2 :], X)
        r = y - m
        if not (np.all(np.isfinite(A)) and np.all(np.isfinite(r))):
            return bad
        try:
            U = sla.cholesky(A, lower=False)
        except (np.linalg.LinAlgError, ValueError):
            return bad
        alpha = sla.cho_solve((U, False), r) / sl
        lml = -0.5 * (r @ alpha) - np.sum(np.log(np.diag(U))) - 0.5 * N * np.log(2 * np.pi * sl)
        if not np.isfinite(lml):
            return bad
        if not grad:
            return lml, None
        Ui = sla.solve_triangular(U, np.eye(N), lower=False)
        W = (Ui @ Ui.T) / sl - np.outer(alpha, alpha)
        WK = W * K
        g = np.empty(P)
        for d in range(D):
            g[d] = -0.5 * np.sum(WK * (Xs[:, d][:, None] - Xs[:, d][None, :]) ** 2)
        g[D] = -np.sum(WK)
        g[D + 1] = -0.5 * dsn2 * np.trace(W)
        g[D + 2 :] = dm @ alpha
        if not np.all(np.isfinite(g)):
            return bad
    return lml, g


def log_marginal_likelihood(gp, hyp, *, grad=False, device=True, ctx=None):
    """Log marginal likelihood of ``gp``'s training data under each row of ``hyp`` (B, P): ``lml`` (B,), or
    ``(lml, dlml (B, P))`` with ``grad=True`` -- the objective of hyper-parameter fitting, without priors.

    ``gp`` is read as ``device_posterior`` reads it (``X``, ``y``, ``s2``, ``mean``, ``noise``; the same noise rule).  The
    derivative with respect to the noise parameter is that of constant additive noise (d sn2 / d log sn =
    2 exp(2 hyp_noise)) where the GP has it -- a noise object's ``constant_add``; a stand-in without a noise object
    always has -- and 0 otherwise.
    ``device=True``: batched on the device (vbmc_gp_lml: the factorisation of ``vbmc_gp_posterior`` in chunks, the
    gradient's trace on the FP64 matrix cores); the posterior the context holds is untouched.  Rows with
    ``sn2_div < 1e-6`` and shapes the device does not take (D > 32) are computed on the host, row by row, as
    ``device=False`` computes every row (NumPy / SciPy, the same formulas).  A row that is not positive definite gives
    ``-inf`` and a NaN gradient row on both routes; it never raises."""
    X = _lib.f64(np.atleast_2d(gp.X))
    y = _lib.f64(np.ravel(gp.y))
    N, D = X.shape
    hyp = _lib.f64(np.atleast_2d(hyp))
    B, P = hyp.shape
    kind = mean_kind_of(gp)
    if P != D + 2 + (0, 1, 1 + 2 * D)[kind]:
        raise ValueError(f"log_marginal_likelihood: hyp has {P} columns, the GP takes {D + 2 + (0, 1, 1 + 2 * D)[kind]}")
    with np.errstate(all="ignore"):
        sn2 = _lib.f64(np.stack([_noise_var(gp, h[D + 1 : D + 2]) for h in hyp]))
        sn2_div = _lib.f64(np.min(sn2, axis=1))
        noise = getattr(gp, "noise", None)
        const_add = True if noise is None or not hasattr(noise, "compute") else bool(getattr(noise, "constant_add", False))
        dsn2 = _lib.f64(2.0 * np.exp(2 * hyp[:, D + 1]) if const_add else np.zeros(B))
    lml = np.empty(B)
    dlml = np.empty((B, P)) if grad else None
    host_rows = np.ones(B, dtype=bool)
    if device:
        ctx = (getattr(gp, "ctx", None) or _lib.default_context()) if ctx is None else ctx
        dev = np.flatnonzero(sn2_div >= 1e-6)
        if dev.size:
            h_d, sn2_d, div_d, ds_d = (_lib.f64(a[dev]) for a in (hyp, sn2, sn2_div, dsn2))
            lml_d = np.empty(dev.size)
            dl_d = np.empty((dev.size, P)) if grad else None
            status = np.zeros(dev.size, dtype=np.int32)
            rc = ctx._lib.vbmc_gp_lml(ctx._h, N, D, dev.size, P, kind, _lib.ptr(X), _lib.ptr(y), _lib.ptr(sn2_d),
                                      _lib.ptr(div_d), _lib.ptr(ds_d), _lib.ptr(h_d), int(bool(grad)), _lib.ptr(lml_d),
                                      _lib.ptr(dl_d), status.ctypes.data_as(C.POINTER(C.c_int32)))
            if rc != _lib.E_UNSUP:
                ctx.check(rc)
                lml[dev] = lml_d
                if grad:
                    dlml[dev] = dl_d
                host_rows[dev] = False
    for b in np.flatnonzero(host_rows):
        lml[b], g = _host_lml(X, y, kind, hyp[b], sn2[b], sn2_div[b], dsn2[b], grad)
        if grad:
            dlml[b] = g
    return (lml, dlml) if grad else lml


class GP:
    def __init__(self, D, covariance, mean, noise):
        if not isinstance(covariance, SquaredExponential):
            raise NotImplementedError("only the squared-exponential ARD kernel is on the ELBO path")
        self.D = D
        self.covariance = covariance
        self.mean = mean
        self.noise = noise
        self.X = None
        self.y = None
        self.s2 = None
        self.posteriors = None
        self.temporary_data = {}
        self._ctx = None

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.default_context()
        return self._ctx

    @ctx.setter
    def ctx(self, v):
        self._ctx = v

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_ctx"] = None
        return st

    def _posterior(self, hyp):
        """alpha, L, sW for one hyper-parameter vector (SURVEY Appendix A 'Posterior')."""
        X, y = self.X, self.y
        N, D = X.shape
        cov_n = self.covariance.hyperparameter_count(D)
        noise_n = self.noise.hyperparameter_count()
        Kxx = self.covariance.compute(hyp[:cov_n], X)
        m = self.mean.compute(hyp[cov_n + noise_n :], X)
        sn2 = self.noise.compute(hyp[cov_n : cov_n + noise_n], X, y, self.s2).ravel()
        sn2_div = np.min(sn2)
        sn2_mult = 1.0
        resid = y.ravel() - m
        if sn2_div * sn2_mult >= 1e-6:
            sl = sn2_div * sn2_mult
            L = sla.cholesky(Kxx / sl + np.diag(sn2 / sn2_div), lower=False)
            alpha = sla.cho_solve((L, False), resid) / sl
            L_chol = True
        else:
            L_chol = False
            L = -np.linalg.inv(Kxx + sn2_mult * np.diag(sn2))
            alpha = -L @ resid
        return SimpleNamespace(
            hyp=np.array(hyp, dtype=np.float64), alpha=alpha.reshape(-1, 1),
            sW=np.ones(N) / np.sqrt(sn2_div * sn2_mult), L=L, sn2_mult=sn2_mult, L_chol=L_chol,
        )

    def update(self, X_new=None, y_new=None, s2_new=None, hyp=None, compute_posterior=True, *, device=False,
               fetch=True):
        """REPLACE the training data (when given) and rebuild the posterior records.  ``device=True``: the records are
        built on the device and stay installed there (``device_posterior``; ``fetch`` as there); where that route does
        not apply the call takes the host path below, with its bits."""
        if X_new is not None:
            self.X = np.atleast_2d(np.asarray(X_new, dtype=np.float64))
            self.y = np.asarray(y_new, dtype=np.float64).reshape(-1, 1)
            self.s2 = None if s2_new is None else np.asarray(s2_new, dtype=np.float64).reshape(-1, 1)
        if hyp is None:
            hyp = np.stack([p.hyp for p in self.posteriors])
        hyp = np.atleast_2d(np.asarray(hyp, dtype=np.float64))
        if device and device_posterior(self, hyp, ctx=self.ctx, fetch=fetch):
            return
        posts = np.empty(hyp.shape[0], dtype=object)
        for i, h in enumerate(hyp):
            posts[i] = self._posterior(h)
        self.posteriors = posts

    def append(self, x_new, y_new, *, device=True, fetch=True):
        """Add ONE training point: ``X``, ``y`` grow by a row and the posterior records follow.

        This class's ``update(X_new, y_new)`` REPLACES the training data; gpyreg's ``update(xnew, ynew)`` -- what the
        reference calls after every acquired point (vbmc/active_sample.py:584) -- APPENDS to it.  ``append`` is that
        call for this class.  With ``device=True`` and the context holding this GP's posterior as the device built it
        (``update(device=True)``, ``device_posterior`` or an earlier ``append``) under constant noise, the factor, its
        inverse and ``alpha`` are extended on the device in O(S N^2) (vbmc_gp_append); otherwise the call is
        ``update`` on the extended data.  ``fetch`` as in ``device_posterior``."""
        x = _lib.f64(np.ravel(x_new))
        if x.size != self.X.shape[1]:
            raise ValueError("append: x_new must be one point of the GP's dimension")
        if self.s2 is not None:
            raise NotImplementedError("append under user-provided noise: call update with the extended X, y, s2")
        y = float(np.ravel(y_new)[0])
        X1 = np.vstack([self.X, x[None, :]])
        y1 = np.vstack([self.y, [[y]]])
        ctx = self.ctx
        posts = self.posteriors
        hyp = np.stack([p.hyp for p in posts])
        dev_key = getattr(ctx, "_gp_dev", None)
        if device and dev_key is not None and dev_key == _gp_fingerprint(self, ctx)[0]:
            S, N1 = len(posts), X1.shape[0]
            alpha = np.empty((S, N1))
            L = np.empty((S, N1, N1)) if fetch else None
            rc = ctx._lib.vbmc_gp_append(ctx._h, _lib.ptr(x), y, _lib.ptr(alpha), _lib.ptr(L))
            if rc != _lib.E_UNSUP:
                ctx.check(rc)
                self.X, self.y = X1, y1
                self.posteriors = _records(hyp, alpha, L, [p.sW[0] for p in posts])
                _adopt(self, ctx, dev=True)
                return
        self.update(X1, y1, None, hyp, device=device, fetch=fetch)

    def log_likelihood(self, hyp=None, grad=False, *, device=True):
        """``log_marginal_likelihood`` of this GP: ``hyp`` (B, P), default the present records' samples."""
        if hyp is None:
            hyp = np.stack([np.ravel(p.hyp) for p in self.posteriors])
        return log_marginal_likelihood(self, hyp, grad=grad, device=device, ctx=self.ctx if device else None)

    def get_hyperparameters(self, as_array=True):
        return np.stack([p.hyp for p in self.posteriors])

    def predict(self, x_star, y_star=None, s2_star=0, add_noise=False, separate_samples=False, *,
                ctx=None):
        """Posterior predictive mean/variance at ``x_star`` (M, D) on the MI355X.
        Returns (M, S) arrays when ``separate_samples`` else (M, 1)."""
        if self.noise.user_provided_add and add_noise and np.any(np.asarray(s2_star) != 0):
            raise NotImplementedError("add_noise with user-provided s2_star is not supported")
        ctx = self.ctx if ctx is None else ctx
        upload_gp(self, ctx)
        xs = _lib.f64(np.atleast_2d(x_star))
        M = xs.shape[0]
        S = len(self.posteriors)
        shape = (M, S) if separate_samples else (M, 1)
        fmu, fs2 = np.empty(shape), np.empty(shape)
        ctx.check(
            ctx._lib.vbmc_gp_predict(
                ctx._h, M, _lib.ptr(xs), int(bool(add_noise)), int(bool(separate_samples)),
                _lib.ptr(fmu), _lib.ptr(fs2),
            )
        )
        return fmu, fs2
