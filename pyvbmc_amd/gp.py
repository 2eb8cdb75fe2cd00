"""GP container for the ELBO path: the subset of ``gpyreg.GP`` PyVBMC touches on it.

gpyreg is a third-party dependency of the reference that is not part of its tree
(`gpyreg >= 0.1.0`, /root/reference/pyproject.toml:13).  What PyVBMC needs from it
on this path is (a) the posterior record per hyper-parameter
sample -- ``posteriors[s].{hyp, alpha, sW, L, sn2_mult, L_chol}`` -- and (b)
``predict``.  This module provides a duck-type with the same attribute/method
names so the hot-path functions accept either it or a real ``gpyreg.GP``:

* ``update(X_new, y_new, s2_new, hyp)`` builds the posterior records on the host.
  That is the O(N^3) Cholesky done ONCE per GP fit -- an input of the path
  (SURVEY 8a row a11), not part of it.
* ``predict`` runs on the MI355X (vbmc_gp_predict).
* ``update(..., device=True)``, ``append`` and ``device_posterior`` build the same records on the device instead
  (vbmc_gp_posterior / vbmc_gp_append: batched FP64 Cholesky, one-point append) and leave them installed there, so
  the ``upload_gp`` that follows ships nothing.  Opt-in: the default path and its bits are unchanged.
* ``append_point`` / ``reupdate``: the one-point append and the mirror of the reference's ``reupdate_gp`` for any GP duck
  type ``device_posterior`` accepts, under user-provided noise too (vbmc_gp_append_noisy); what the active-sampling loop
  (active_sample.py) calls after every acquired point.
* ``log_marginal_likelihood`` / ``GP.log_likelihood``: the objective of hyper-parameter fitting and its gradient for a
  batch of candidates on the device (vbmc_gp_lml), with a NumPy / SciPy host route of the same formulas.
* ``optimize_hyperparameters``: R box-constrained limited-memory BFGS runs over lml + log prior in lockstep on the device
  (vbmc_gp_hyp_optimize), one batch of R trial points per evaluation round, with a NumPy host route of the same
  algorithm; ``GP.fit(optimizer="lockstep")`` uses it for the optimiser stage.
* ``hyper_log_prior``, ``sample_hyperparameters`` and ``GP.fit`` / ``set_bounds`` / ``set_priors``: hyper-parameter
  fitting.  The sampler runs C slice chains over lml + log prior in lockstep on the device (vbmc_gp_hyp_sample), one
  batch of C candidates per evaluation round, with a NumPy host route on the same draws.  The sampler, the priors and
  ``fit``'s stages are this package's own: gpyreg's are not in the reference tree, and neither its stream nor its
  default bounds are reproduced.
* ``GP.fit(optimizer="fused")``: those stages as ONE device call (vbmc_gp_fit) -- the candidates drawn, scored and ranked,
  the lockstep optimiser, the optimum selected, the lockstep chains and the posterior build, with kernels doing the
  hand-overs and the posterior left installed; ``fit_design`` / ``fit_rank`` / ``fit_select`` and the ``device=False`` route
  state it in NumPy.  ``get_bounds_info`` of the covariance, mean and noise classes is the package's own rule for bounds
  from the data.  pyvbmc_amd/gaussian_process_train.py builds the reference's ``train_gp`` on it.
"""
import logging
import math
import ctypes as C
import sys
from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla

from . import _lib


# ``get_bounds_info(X, y) -> dict(LB, UB, PLB, PUB, x0)`` of the covariance, mean and noise classes below: hard bounds,
# plausible bounds and a starting point per hyper-parameter of the block, from the data's ranges.  gpyreg has methods of
# this name, but gpyreg is not part of the reference tree: the numbers here are THIS PACKAGE'S OWN RULE,
# not gpyreg's defaults.  w_d = max X_d - min X_d, h = max y - min y; a zero range counts as 1.
def _range(v, axis=None):
    r = np.max(v, axis=axis) - np.min(v, axis=axis)
    return np.where(r > 0, r, 1.0)


def _spread(v, axis=None):
    """std, and 1 where the range is zero (the std of a constant column is rounding noise, not a scale)"""
    return np.where(np.max(v, axis=axis) - np.min(v, axis=axis) > 0, np.std(v, axis=axis), 1.0)


def _log_scale_info(width, spread, lo=1e-6):
    """log-scale block: LB log(lo w), UB log(10 w), PLB log(1e-3 w), PUB log w, x0 log spread"""
    return dict(LB=np.log(lo * width), UB=np.log(10 * width), PLB=np.log(1e-3 * width), PUB=np.log(width), x0=np.log(spread))


class SquaredExponential:
    """SE-ARD: k(a,b) = sf^2 exp(-1/2 sum_d ((a_d-b_d)/ell_d)^2); hyp = [log ell (D), log sf]."""

    def hyperparameter_count(self, D):
        return D + 1

    def get_bounds_info(self, X, y):
        """log length scales from w_d and std(X_d), log output scale from h and std(y) (the package's own rule)."""
        X, y = np.atleast_2d(X), np.ravel(y)
        ell = _log_scale_info(_range(X, 0), _spread(X, 0))
        sf = _log_scale_info(np.atleast_1d(_range(y)), np.atleast_1d(_spread(y)))
        return {k: np.concatenate([ell[k], sf[k]]) for k in ell}

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

    def get_bounds_info(self, X, y):
        return {k: np.zeros(0) for k in ("LB", "UB", "PLB", "PUB", "x0")}


def _mean_const_info(y):
    """constant of a mean: LB min y - h/2, UB max y + h/2, PLB / PUB the 0.1 / 0.9 quantiles of y, x0 median y"""
    y = np.ravel(y)
    h = float(_range(y))
    return dict(LB=np.array([np.min(y) - 0.5 * h]), UB=np.array([np.max(y) + 0.5 * h]), PLB=np.array([np.quantile(y, 0.1)]),
                PUB=np.array([np.quantile(y, 0.9)]), x0=np.array([np.median(y)]))


class ConstantMean:
    kind = _lib.MEAN_CONST

    def hyperparameter_count(self, D):
        return 1

    def compute(self, hyp, X):
        return np.full(X.shape[0], hyp[0])

    def get_bounds_info(self, X, y):
        return _mean_const_info(y)


class NegativeQuadratic:
    """m(x) = m0 - 1/2 sum_d ((x_d - xm_d)/omega_d)^2; hyp = [m0, xm (D), log omega (D)]
    (layout used at variational_optimization.py:1383-1392)."""

    kind = _lib.MEAN_NEGQUAD

    def hyperparameter_count(self, D):
        return 1 + 2 * D

    def compute(self, hyp, X):
        D = X.shape[1]
        return hyp[0] - 0.5 * np.sum(((X - hyp[1 : 1 + D]) / np.exp(hyp[1 + D : 1 + 2 * D])) ** 2, 1)

    def get_bounds_info(self, X, y):
        """the constant as ``ConstantMean``; location: LB / UB min X - w/2 ... max X + w/2, PLB / PUB min X ... max X, x0
        median X; log scale: LB log(1e-3 w), UB log(10 w), PLB log(1e-2 w), PUB log w, x0 log std(X)."""
        X = np.atleast_2d(X)
        w, lo, hi = _range(X, 0), np.min(X, axis=0), np.max(X, axis=0)
        c = _mean_const_info(y)
        loc = dict(LB=lo - 0.5 * w, UB=hi + 0.5 * w, PLB=lo, PUB=hi, x0=np.median(X, axis=0))
        om = dict(LB=np.log(1e-3 * w), UB=np.log(10 * w), PLB=np.log(1e-2 * w), PUB=np.log(w), x0=np.log(_spread(X, 0)))
        return {k: np.concatenate([c[k], loc[k], om[k]]) for k in c}


class GaussianNoise:
    def __init__(self, constant_add=False, user_provided_add=False, scale_user_provided=False,
                 rectified_linear_output_dependent_add=False):
        if scale_user_provided or rectified_linear_output_dependent_add:
            raise NotImplementedError("only constant and user-provided additive noise are supported")
        self.constant_add = constant_add
        self.user_provided_add = user_provided_add

    def hyperparameter_count(self):
        return 1

    def get_bounds_info(self, X, y):
        """log noise scale: LB log 1e-3, UB log max(h, 1), PLB log 1e-3, PUB log max(std(y), 1e-2), x0 log 1e-3."""
        y = np.ravel(y)
        lo = math.log(1e-3)
        return dict(LB=np.array([lo]), UB=np.array([math.log(max(float(_range(y)), 1.0))]), PLB=np.array([lo]),
                    PUB=np.array([math.log(max(float(np.std(y)), 1e-2))]), x0=np.array([lo]))

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


def _records(hyp, alpha, L, sW0, sn2_div=None, sn2_const=None):
    """Records of a device build.  ``sn2_div`` (S): the scale the build used, kept exactly (``sW`` = 1 / sqrt of it does
    not give it back); ``sn2_const`` (S): the constant noise term where the DEVICE formed it (``vbmc_gp_fit``), absent
    where the host's noise rule gave the build its ``sn2``.  Both are what ``reinstall`` needs; the fingerprint and
    ``upload_gp`` do not read them."""
    posts = np.empty(len(hyp), dtype=object)
    N = alpha.shape[1]
    for s in range(len(hyp)):
        posts[s] = SimpleNamespace(hyp=np.array(hyp[s], dtype=np.float64), alpha=alpha[s].reshape(-1, 1).copy(),
                                   sW=np.ones(N) * sW0[s], L=None if L is None else L[s], sn2_mult=1.0, L_chol=True)
        if sn2_div is not None:
            posts[s].sn2_div = float(sn2_div[s])
        if sn2_const is not None:
            posts[s].sn2_const = float(sn2_const[s])
    return posts


def _carried(posts, name):
    """The field ``name`` of every record, or None when one of them has none (records of another maker)."""
    vals = [getattr(p, name, None) for p in posts]
    return None if any(v is None for v in vals) else vals


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
    gp.posteriors = _records(hyp, alpha, L, 1.0 / np.sqrt(sn2_div * 1.0), sn2_div)
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


def reinstall(gp, *, ctx=None):
    """Put the posterior of a GP that comes from a pickle (or from another context) back on the device AS THE DEVICE
    BUILT IT, so that ``append_point`` extends it with the arithmetic it would have used in the process that built it.

    The records of this package carry the build's inputs: ``sn2_div``, the scale, and -- where ``vbmc_gp_fit`` formed the
    constant noise term on the device -- ``sn2_const``.  ``vbmc_gp_posterior`` is called with them (``sn2`` = ``sn2_const``
    + ``s2``, else the host's noise rule at the records' samples, which is what ``device_posterior`` passed) and the
    ``alpha`` and ``L`` it returns must be ``np.array_equal`` to the records'.  Then the state is adopted as device-built,
    the records' arrays stay the objects they are, and the call returns True.

    Otherwise -- a record without ``sn2_div`` or without ``L``, the non-Cholesky branch, a shape the device refuses, a
    build that does not reproduce the records (host-built records; a per-point-noise state extended by
    ``vbmc_gp_append_noisy`` after a fit) -- the records are uploaded as they are (``upload_gp``: correct, but the next
    append rebuilds), one warning says that a resumed run will not be bit-exact, and the call returns False.  Without a
    device nothing is installed and the call returns False."""
    ctx = _device_ctx(gp, ctx, True)
    if ctx is None:
        return False
    posts = list(gp.posteriors)
    sn2_div, sn2_const = _carried(posts, "sn2_div"), _carried(posts, "sn2_const")
    if sn2_div is not None and all(p.L is not None and p.L_chol for p in posts):
        X, y = _lib.f64(np.atleast_2d(gp.X)), _lib.f64(np.ravel(gp.y))
        N, D = X.shape
        hyp = _lib.f64(np.stack([np.ravel(p.hyp) for p in posts]))
        s2 = _s2_column(gp)
        if sn2_const is None:
            sn2 = np.stack([_noise_var(gp, h[D + 1 : D + 2]) for h in hyp])
        else:
            sn2 = np.stack([np.full(N, c) if s2 is None else c + s2.ravel() for c in sn2_const])
        sn2, div = _lib.f64(sn2), _lib.f64(sn2_div)
        alpha, L = np.empty((len(posts), N)), np.empty((len(posts), N, N))
        invalidate_gp(ctx)
        rc = ctx._lib.vbmc_gp_posterior(ctx._h, N, D, len(posts), hyp.shape[1], mean_kind_of(gp), _lib.ptr(X), _lib.ptr(y),
                                        _lib.ptr(sn2), _lib.ptr(div), _lib.ptr(hyp), _lib.ptr(alpha), _lib.ptr(L))
        if rc == 0 and all(np.array_equal(alpha[s], np.ravel(p.alpha)) and np.array_equal(L[s], p.L)
                           for s, p in enumerate(posts)):
            _adopt(gp, ctx, dev=True)
            return True
    invalidate_gp(ctx)
    upload_gp(gp, ctx)
    logging.getLogger("GP").warning("reinstall: the device build does not reproduce the saved posterior records; they were "
                                    "uploaded as saved, and a run resumed from them will not be bit-exact")
    return False


def _host_records(gp, hyp):
    """The posterior records of a GP duck type on the host: ``GP._posterior``'s arithmetic, with the noise rule of
    ``_noise_var`` and the mean by its kind.  For the ducks that have no ``_posterior`` of their own."""
    X = np.atleast_2d(np.asarray(gp.X, dtype=np.float64))
    y = np.ravel(gp.y)
    N, D = X.shape
    kind = mean_kind_of(gp)
    posts = np.empty(len(hyp), dtype=object)
    for i, h in enumerate(hyp):
        Kxx = SquaredExponential().compute(h[: D + 1], X)
        sn2 = _noise_var(gp, h[D + 1 : D + 2])
        sn2_div = np.min(sn2)
        resid = y - _mean_and_grad(kind, h[D + 2 :], X)[0]
        if sn2_div >= 1e-6:
            L = sla.cholesky(Kxx / sn2_div + np.diag(sn2 / sn2_div), lower=False)
            alpha = sla.cho_solve((L, False), resid) / sn2_div
            L_chol = True
        else:
            L_chol = False
            L = -np.linalg.inv(Kxx + np.diag(sn2))
            alpha = -L @ resid
        posts[i] = SimpleNamespace(hyp=np.array(h, dtype=np.float64), alpha=alpha.reshape(-1, 1),
                                   sW=np.ones(N) / np.sqrt(sn2_div), L=L, sn2_mult=1.0, L_chol=L_chol,
                                   sn2_div=float(sn2_div))
    return posts


def _rebuild(gp, hyp, ctx, device, fetch):
    """The posterior records of ``gp`` from its present ``X``, ``y``, ``s2`` at the samples ``hyp``: on the device where
    that route applies, else on the host (the GP's own ``_posterior`` where it has one)."""
    if device and ctx is not None and device_posterior(gp, hyp, ctx=ctx, fetch=fetch):
        return
    if hasattr(gp, "_posterior"):
        posts = np.empty(len(hyp), dtype=object)
        for i, h in enumerate(hyp):
            posts[i] = gp._posterior(h)
        gp.posteriors = posts
    else:
        gp.posteriors = _host_records(gp, hyp)


def _device_ctx(gp, ctx, device):
    """The context of the device route, or None when ``device`` is off or there is no device."""
    if not device:
        return None
    if ctx is None:
        ctx = getattr(gp, "_ctx", None)
    if ctx is None:
        if _lib.device_count() <= 0:
            return None
        ctx = gp.ctx if isinstance(gp, GP) else _lib.default_context()
    return ctx if ctx.device >= 0 else None


def _s2_column(gp):
    s2 = getattr(gp, "s2", None)
    return None if s2 is None or not np.size(s2) else np.asarray(s2, dtype=np.float64).reshape(-1, 1)


def append_point(gp, x_new, y_new, s2_new=None, *, ctx=None, device=True, fetch=True):
    """Add ONE training point to a GP duck type (this package's ``GP``, an attribute-only stand-in or a real
    ``gpyreg.GP`` -- whatever ``device_posterior`` accepts): ``gp.X``, ``gp.y`` and, under user-provided noise, ``gp.s2``
    grow by a row and the posterior records follow at the present hyper-parameter samples.  This is gpyreg's
    ``update(xnew, ynew)`` after an acquired point (vbmc/active_sample.py:584).

    With ``device`` set and the context holding this GP's posterior as the device built it (``device_posterior``,
    ``GP.update(device=True)`` or an earlier append), the factor, its inverse and ``alpha`` are extended on the device in
    O(S N^2): ``vbmc_gp_append`` without ``s2``, ``vbmc_gp_append_noisy`` with it (the new point's noise variance per
    sample from the GP's noise rule).  Where the entry refuses (the new point's noise is below the sample's ``sn2_div``,
    the resident state is another GP's) and without a device, the records are rebuilt from the extended data.
    ``s2_new`` is required exactly when the GP carries ``s2``.  ``fetch`` as in ``device_posterior``.  Returns ``gp``."""
    X0 = np.atleast_2d(np.asarray(gp.X, dtype=np.float64))
    x = _lib.f64(np.ravel(x_new))
    if x.size != X0.shape[1]:
        raise ValueError("append: x_new must be one point of the GP's dimension")
    s2_old = _s2_column(gp)
    if (s2_old is None) != (s2_new is None):
        raise ValueError("append: s2_new is given exactly when the GP carries user-provided noise (gp.s2)")
    y = float(np.ravel(y_new)[0])
    X1 = np.vstack([X0, x[None, :]])
    y1 = np.vstack([np.asarray(gp.y, dtype=np.float64).reshape(-1, 1), [[y]]])
    s2_1 = None if s2_new is None else np.vstack([s2_old, [[float(np.ravel(s2_new)[0])]]])
    posts = gp.posteriors
    hyp = np.stack([np.ravel(p.hyp) for p in posts])
    ctx = _device_ctx(gp, ctx, device)
    dev_key = getattr(ctx, "_gp_dev", None) if ctx is not None else None
    if dev_key is not None and dev_key == _gp_fingerprint(gp, ctx)[0]:
        S, N1, D = len(posts), X1.shape[0], X1.shape[1]
        alpha = np.empty((S, N1))
        L = np.empty((S, N1, N1)) if fetch else None
        if s2_1 is None:
            rc = ctx._lib.vbmc_gp_append(ctx._h, _lib.ptr(x), y, _lib.ptr(alpha), _lib.ptr(L))
        else:
            probe = SimpleNamespace(X=x[None, :], y=np.array([[y]]), s2=s2_1[-1:], noise=getattr(gp, "noise", None))
            sn2_new = _lib.f64([_noise_var(probe, h[D + 1 : D + 2])[0] for h in hyp])
            rc = ctx._lib.vbmc_gp_append_noisy(ctx._h, _lib.ptr(x), y, _lib.ptr(sn2_new), _lib.ptr(alpha), _lib.ptr(L))
        if rc != _lib.E_UNSUP:
            ctx.check(rc)
            gp.X, gp.y = X1, y1
            if s2_1 is not None:
                gp.s2 = s2_1
            # (an append leaves the scale as it is: ``sn2_div`` and ``sn2_const`` go through unchanged)
            gp.posteriors = _records(hyp, alpha, L, [np.ravel(p.sW)[0] for p in posts], _carried(posts, "sn2_div"),
                                     _carried(posts, "sn2_const"))
            _adopt(gp, ctx, dev=True)
            return gp
    gp.X, gp.y, gp.s2 = X1, y1, s2_1
    _rebuild(gp, hyp, ctx, device, fetch)
    return gp


def training_data(function_logger):
    """``(X, y, s2)`` of the evaluated points of a function logger (reference gaussian_process_train.py
    ``_get_training_data``, :739-772): ``s2 = S^2`` where the logger's ``noise_flag`` is set, else None."""
    flag = function_logger.X_flag
    X = np.array(function_logger.X[flag], dtype=np.float64)
    y = np.array(function_logger.y[flag], dtype=np.float64).reshape(-1, 1)
    S = getattr(function_logger, "S", None)
    if S is None or not getattr(function_logger, "noise_flag", True):
        return X, y, None
    return X, y, (np.asarray(S[flag], dtype=np.float64) ** 2).reshape(-1, 1)


def reupdate(function_logger, gp, *, ctx=None, device=True, fetch=True):
    """Mirror of ``reupdate_gp`` (reference gaussian_process_train.py:817-842): the GP takes the logger's training data
    and its posterior records are rebuilt at the present hyper-parameter samples (``device_posterior``, else the host).
    Where the logger holds exactly the GP's data plus ONE new row evaluated once, the call is ``append_point`` instead
    (O(S N^2), under per-point noise too).  Returns ``gp``."""
    X, y, s2 = training_data(function_logger)
    X0 = np.atleast_2d(np.asarray(gp.X, dtype=np.float64))
    N = X0.shape[0]
    s2_old = _s2_column(gp)
    one_more = (X.shape[0] == N + 1 and (s2 is None) == (s2_old is None) and np.array_equal(X[:N], X0)
                and np.array_equal(y[:N], np.asarray(gp.y, dtype=np.float64).reshape(-1, 1))
                and (s2 is None or np.array_equal(s2[:N], s2_old))
                and np.ravel(function_logger.n_evals[function_logger.X_flag])[N] == 1)
    if one_more:
        return append_point(gp, X[N], y[N, 0], None if s2 is None else s2[N, 0], ctx=ctx, device=device, fetch=fetch)
    hyp = np.stack([np.ravel(p.hyp) for p in gp.posteriors])
    gp.X, gp.y, gp.s2 = X, y, s2
    _rebuild(gp, hyp, _device_ctx(gp, ctx, device), device, fetch)
    return gp


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
        dsn2 = _lib.f64(2.0 * np.exp(2 * hyp[:, D + 1]) if _const_noise_form(gp)[0] else np.zeros(B))
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


# ------------------------------------------------------------------------------------------ hyper-parameter sampling
def _prior_arrays(priors, P):
    """``(mu, sigma, df)`` of P entries from a prior dict (None: no prior anywhere, sigma NaN)."""
    if priors is None:
        return tuple(np.full(P, np.nan) for _ in range(3))
    mu, sigma, df = (np.array(np.broadcast_to(np.asarray(priors[k], dtype=np.float64), (P,))) for k in ("mu", "sigma", "df"))
    on = ~np.isnan(sigma)
    if np.any(on & ~((sigma > 0) & np.isfinite(sigma) & np.isfinite(mu) & (df > 0))):
        raise ValueError("hyper prior: a parameter with a prior needs finite mu, sigma > 0 and df > 0 (or +inf)")
    return mu, sigma, df


def hyper_log_prior(hyp, priors, grad=False):
    """Log prior of hyper-parameter vectors ``hyp`` (P,) or (B, P): ``sum_p t_p``, added with p ascending.

    ``priors``: dict of arrays ``mu``, ``sigma``, ``df`` (P entries each).  ``t_p = 0`` where ``sigma_p`` is NaN (no
    prior); else with z = (h_p - mu_p) / sigma_p it is the Gaussian's ``-1/2 log(2 pi) - log sigma - 1/2 z^2`` where
    ``df_p`` is +inf and the Student-t's ``lgamma((nu+1)/2) - lgamma(nu/2) - 1/2 log(pi nu) - log sigma - (nu+1)/2
    log1p(z^2/nu)`` otherwise -- what vbmc_gp_hyp_sample evaluates on the device.  ``grad=True``: ``(value, d/dhyp)``."""
    h = np.asarray(hyp, dtype=np.float64)
    one = h.ndim == 1
    h = np.atleast_2d(h)
    B, P = h.shape
    mu, sigma, df = _prior_arrays(priors, P)
    lp, g = np.zeros(B), np.zeros((B, P))
    for p in range(P):
        if np.isnan(sigma[p]):
            continue
        z = (h[:, p] - mu[p]) / sigma[p]
        if np.isinf(df[p]):
            c = -0.5 * math.log(2 * math.pi) - math.log(sigma[p])
            t = c - 0.5 * (z * z)
            g[:, p] = -z / sigma[p]
        else:
            nu = float(df[p])
            c = math.lgamma(0.5 * (nu + 1)) - math.lgamma(0.5 * nu) - 0.5 * math.log(math.pi * nu) - math.log(sigma[p])
            t = c - 0.5 * (nu + 1) * np.log1p(z * z / nu)
            g[:, p] = -(nu + 1) * z / (sigma[p] * (nu + z * z))
        lp = lp + t
    if one:
        return (float(lp[0]), g[0]) if grad else float(lp[0])
    return (lp, g) if grad else lp


_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_SLICE_OUT_CAP, _SLICE_SHRINK_CAP, _SLICE_STREAM = 32, 64, 6


def _philox_bits53(i, chain, seed, stream=_SLICE_STREAM):
    """The upper 53 bits of words 0, 1 of Philox4x32-10 block (i_lo, i_hi, chain, stream) under key ``seed``
    (csrc/philox.h).  Stream 6 (the default): draw i of chain ``chain`` of the slice samplers; stream 10: coordinate i of
    drawn candidate ``chain`` of the fit's design (csrc/sample.hip lists the streams)."""
    m = 0xFFFFFFFF
    c0, c1, c2, c3 = i & m, (i >> 32) & m, chain & m, stream
    k0, k1 = seed & m, (seed >> 32) & m
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & m, (p0 >> 32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + _PHILOX_W0) & m, (k1 + _PHILOX_W1) & m
    return ((c0 << 32) | c1) >> 11


def _slice_chain(log_p, x0, widths, lb, ub, n, thin, burn_in, seed, chain):
    """One chain of the package's coordinate-wise slice sampler (Neal 2003) on the host, the statement
    vbmc_gp_hyp_sample and vbmc_is_mcmc run on the device: level ``f(x) + log u`` (u in (0, 1]), an interval of width
    ``widths_d`` placed around x_d and clipped to the bounds, stepping out (at most 32 evaluations a side) while f at an
    end that is inside the bounds lies above the level, shrinkage (at most 64 proposals; x_d stays when the cap is
    reached), x0 clipped into the bounds, ``burn_in + n thin`` sweeps over the coordinates in order, a sample kept after
    every thin-th sweep past burn_in.  Returns ``(samples (n, P), f (n,), stats)`` with stats = [evaluations, draws,
    step-out caps, shrink caps]; ``ValueError("Invalid value.")`` when f(x0) is not finite."""
    x = np.maximum(np.minimum(np.array(x0, dtype=np.float64).ravel(), ub), lb)
    P = x.size
    cnt = {"evals": 0, "draws": 0, "out": 0, "shrink": 0}

    def bits():
        cnt["draws"] += 1
        return _philox_bits53(cnt["draws"] - 1, chain, seed)

    def f(pt):
        cnt["evals"] += 1
        return float(log_p(pt))

    def at(d, v):
        pt = x.copy()
        pt[d] = v
        return f(pt)

    fx = f(x)
    if not np.isfinite(fx):
        raise ValueError("Invalid value.")
    samples, f_vals = np.empty((n, P)), np.empty(n)
    kept = 0
    for t in range(burn_in + n * thin):
        for d in range(P):
            xd, w, lo, hi = x[d], widths[d], lb[d], ub[d]
            ly = fx + np.log((bits() + 1) * 2.0**-53)
            L = xd - w * (bits() * 2.0**-53)
            R = L + w
            L, R = max(L, lo), min(R, hi)
            j = 0
            while L > lo:
                if j == _SLICE_OUT_CAP:
                    cnt["out"] += 1
                    break
                if at(d, L) <= ly:
                    break
                L, j = max(L - w, lo), j + 1
            j = 0
            while R < hi:
                if j == _SLICE_OUT_CAP:
                    cnt["out"] += 1
                    break
                if at(d, R) <= ly:
                    break
                R, j = min(R + w, hi), j + 1
            for j in range(_SLICE_SHRINK_CAP):
                xp = L + (bits() * 2.0**-53) * (R - L)
                fp = at(d, xp)
                if fp > ly:
                    x[d], fx = xp, fp
                    break
                if xp < xd:
                    L = xp
                else:
                    R = xp
            else:
                cnt["shrink"] += 1
        if t >= burn_in and (t - burn_in + 1) % thin == 0:
            samples[kept], f_vals[kept] = x, fx
            kept += 1
    return samples, f_vals, np.array([cnt["evals"], cnt["draws"], cnt["out"], cnt["shrink"]], dtype=np.int64)


def _const_noise_form(gp):
    """Whether the GP's noise is constant additive noise exp(2 hyp_noise) plus, optionally, the user-provided ``s2`` -- the
    forms vbmc_gp_hyp_sample evaluates itself -- and the ``s2`` (N,) that applies (None: none)."""
    noise = getattr(gp, "noise", None)
    s2 = getattr(gp, "s2", None)
    s2 = None if s2 is None or not np.size(s2) else _lib.f64(np.ravel(s2))
    if noise is None or not hasattr(noise, "compute"):
        return True, s2  # (a stand-in without a noise object: the rule of ``_noise_var``)
    if not getattr(noise, "constant_add", False):
        return False, None
    return True, s2 if getattr(noise, "user_provided_add", False) else None


def _hyper_problem(who, runs, gp, x0, lb, ub, priors, ctx, device):
    """The prologue ``sample_hyperparameters`` and ``optimize_hyperparameters`` share (``who``, ``runs``: the caller's name and its letter
    for the number of starts, for its error texts): the GP's data, the starts and the box as float64 arrays of the right shapes, the prior arrays, the noise
    form and the context of the device route (None: the host route runs)."""
    X = _lib.f64(np.atleast_2d(gp.X))
    y = _lib.f64(np.ravel(gp.y))
    D = X.shape[1]
    kind = mean_kind_of(gp)
    P = D + 2 + (0, 1, 1 + 2 * D)[kind]
    x0 = _lib.f64(np.atleast_2d(x0))
    if x0.ndim != 2 or x0.shape[1] != P or x0.shape[0] < 1:
        raise ValueError(f"{who}: x0 must be ({runs}, {P})")
    lb, ub = (_lib.f64(np.array(np.broadcast_to(np.asarray(a, dtype=np.float64), (P,)))) for a in (lb, ub))
    if not (np.all(np.isfinite(lb)) and np.all(np.isfinite(ub)) and np.all(lb <= ub)):
        raise ValueError(f"{who}: finite bounds with lb <= ub are required")
    mu, sigma, df = (_lib.f64(a) for a in _prior_arrays(priors, P))
    const_add, s2 = _const_noise_form(gp)
    ctx = None if not (device and const_add) else (getattr(gp, "ctx", None) or _lib.default_context()) if ctx is None else ctx
    return SimpleNamespace(X=X, y=y, N=X.shape[0], D=D, kind=kind, P=P, x0=x0, lb=lb, ub=ub, mu=mu, sigma=sigma, df=df,
                           pri={"mu": mu, "sigma": sigma, "df": df}, const_add=const_add, s2=s2, ctx=ctx)


def sample_hyperparameters(gp, x0, *, lb, ub, widths, priors=None, n=1, thin=1, burn_in=0, seed=None, device=True, ctx=None):
    """Slice-sample the hyper-parameters of ``gp`` from ``lml + log prior``: C chains, one per row of ``x0`` (C, P).

    ``gp`` is read as ``log_marginal_likelihood`` reads it.  ``lb``, ``ub`` (finite), ``widths`` (> 0): P entries each;
    ``priors``: as ``hyper_log_prior`` takes them (None: flat inside the bounds).  Chain c keeps ``n`` samples, one after
    every ``thin``-th of the sweeps that follow ``burn_in``; its draws are counter-based (Philox block (i, c, stream 6)
    under ``seed``; None: a fresh seed), so its samples depend on its own start alone, not on C.
    ``device=True``: the chains advance in lockstep on the device (vbmc_gp_hyp_sample), every evaluation round one batch
    of C candidates through vbmc_gp_lml's kernels; the posterior the context holds is untouched.  Shapes the device
    refuses (D > 32, a noise bound that allows sn2_div < 1e-6, noise that is not constant-additive) and ``device=False``
    run the same chains in NumPy over the host lml, with the same draws.
    Returns ``dict(samples (C, n, P), log_post (C, n), log_priors (C, n), stats (C, 4))``, stats = [evaluations, draws,
    step-out caps hit, shrink caps hit].  ``ValueError("Invalid value.")`` when a chain's start has no finite density."""
    q = _hyper_problem("sample_hyperparameters", "C", gp, x0, lb, ub, priors, ctx, device)
    X, y, N, D, kind, P, x0, lb, ub, pri = q.X, q.y, q.N, q.D, q.kind, q.P, q.x0, q.lb, q.ub, q.pri
    Cn = x0.shape[0]
    widths = _lib.f64(np.array(np.broadcast_to(np.asarray(widths, dtype=np.float64), (P,))))
    if not (np.all(widths > 0) and np.all(np.isfinite(widths))):
        raise ValueError("sample_hyperparameters: widths must be positive")
    n, thin, burn_in = int(n), int(thin), int(burn_in)
    if n < 1 or thin < 1 or burn_in < 0:
        raise ValueError("sample_hyperparameters: n >= 1, thin >= 1, burn_in >= 0")
    seed = int(np.random.SeedSequence().generate_state(2, np.uint32).view(np.uint64)[0]) if seed is None else int(seed)
    seed &= 0xFFFFFFFFFFFFFFFF
    if q.ctx is not None:
        samples, lpost, lprior = np.zeros((Cn, n, P)), np.zeros((Cn, n)), np.zeros((Cn, n))
        stats, invalid = np.zeros((Cn, 4), dtype=np.int64), np.zeros(Cn, dtype=np.int32)
        rc = q.ctx._lib.vbmc_gp_hyp_sample(
            q.ctx._h, N, D, P, kind, _lib.ptr(X), _lib.ptr(y), _lib.ptr(q.s2), Cn, _lib.ptr(x0), _lib.ptr(widths),
            _lib.ptr(lb), _lib.ptr(ub), _lib.ptr(q.mu), _lib.ptr(q.sigma), _lib.ptr(q.df), n, thin, burn_in, C.c_uint64(seed),
            _lib.ptr(samples), _lib.ptr(lpost), _lib.ptr(lprior), stats.ctypes.data_as(C.POINTER(C.c_int64)),
            invalid.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc != _lib.E_UNSUP:
            q.ctx.check(rc)
            if np.any(invalid):
                raise ValueError("Invalid value.")
            return dict(samples=samples, log_post=lpost, log_priors=lprior, stats=stats)

    def log_p(h):
        with np.errstate(all="ignore"):
            sn2 = _noise_var(gp, h[D + 1 : D + 2])
            lml = _host_lml(X, y, kind, h, sn2, np.min(sn2), 0.0, False)[0]
        return lml + hyper_log_prior(h, pri)

    out = [_slice_chain(log_p, x0[c], widths, lb, ub, n, thin, burn_in, seed, c) for c in range(Cn)]
    samples = np.stack([o[0] for o in out])
    return dict(samples=samples, log_post=np.stack([o[1] for o in out]),
                log_priors=np.stack([hyper_log_prior(o[0], pri) for o in out]), stats=np.stack([o[2] for o in out]))


# -------------------------------------------------------------------------------------- hyper-parameter optimisation
_OPT_ARMIJO, _OPT_CURV, _OPT_HALVINGS = 1e-4, 1e-10, 30
STOP_TOL_G, STOP_MAX_ITER, STOP_TOL_F, STOP_SEARCH = 1, 2, 3, 4


def _lbfgs_run(fun, x0, lb, ub, max_iter, m, tol_g, tol_f, trace=None):
    """One run of the package's box-constrained limited-memory BFGS on the host, the statement vbmc_gp_hyp_optimize runs
    on the device (csrc/gp_opt.hip's header has the algorithm).  ``fun(x) -> (phi, g)``, phi = +inf where the point has
    no finite value and gradient.  Returns ``(x, phi, g, stats)`` with stats = [iterations, evaluations, history
    resets, stop reason]; ``ValueError("Invalid value.")`` when phi(x0) is not finite.  ``trace``: a dict that receives
    the lists ``iters`` and ``evals`` (rows as vbmc_gp_hyp_optimize's traces)."""
    x = np.maximum(np.minimum(np.array(x0, dtype=np.float64).ravel(), ub), lb)
    P = x.size
    if not np.all(np.isfinite(x)):
        raise ValueError("Invalid value.")
    phi, g = fun(x)
    n_ev, n_it, n_reset = 1, 0, 0
    if not np.isfinite(phi):
        raise ValueError("Invalid value.")
    it_rows, ev_rows = [], [[0.0, 0.0, phi, 1.0]]
    S, Y, rho, gamma = [], [], [], 1.0  # the pairs, oldest first
    fixed = lb == ub

    def row(d, reset):
        it_rows.append(np.concatenate([x, [phi], g, d, [float(len(S)), float(reset)]]))

    while True:
        in_b = ((x <= lb) & (g > 0)) | ((x >= ub) & (g < 0)) | fixed
        pg = np.where(in_b, 0.0, g)
        if np.max(np.abs(pg)) <= tol_g:
            reason = STOP_TOL_G
            row(np.zeros(P), 0)
            break
        if n_it >= max_iter:
            reason = STOP_MAX_ITER
            row(np.zeros(P), 0)
            break
        steepest = not S
        if S:
            q, al = pg.copy(), [0.0] * len(S)
            for j in range(len(S) - 1, -1, -1):
                al[j] = rho[j] * float(S[j] @ q)
                q = q - al[j] * Y[j]
            q = q * gamma
            for j in range(len(S)):
                be = rho[j] * float(Y[j] @ q)
                q = q + S[j] * (al[j] - be)
            d = np.where(in_b, 0.0, -q)
            if not float(g @ d) < 0.0:
                steepest, S, Y, rho = True, [], [], []
                n_reset += 1
        if steepest:
            d = -pg
            t = min(1.0, 1.0 / float(np.sum(np.abs(pg))))
        else:
            t = 1.0
        row(d, int(steepest))
        accepted = False
        for _ in range(_OPT_HALVINGS + 1):
            xt = np.maximum(np.minimum(x + t * d, ub), lb)
            phit, gt = fun(xt)
            n_ev += 1
            accepted = bool(np.isfinite(phit) and phit <= phi + _OPT_ARMIJO * float(g @ (xt - x)))
            ev_rows.append([float(n_it), t, phit, float(accepted)])
            if accepted:
                break
            t *= 0.5
        if not accepted:
            reason = STOP_SEARCH
            break
        s, yv = xt - x, gt - g
        sy, ss, yy = float(s @ yv), float(s @ s), float(yv @ yv)
        if sy > _OPT_CURV * (math.sqrt(ss) * math.sqrt(yy)):
            if len(S) == m:
                S, Y, rho = S[1:], Y[1:], rho[1:]
            S, Y, rho, gamma = S + [s], Y + [yv], rho + [1.0 / sy], sy / yy
        phi_old, x, g, phi = phi, xt, gt, phit
        n_it += 1
        if phi_old - phi <= tol_f * max(1.0, abs(phi)):
            reason = STOP_TOL_F
            row(np.zeros(P), 0)
            break
    if trace is not None:
        trace["iters"], trace["evals"] = np.array(it_rows), np.array(ev_rows)
    return x, phi, g, np.array([n_it, n_ev, n_reset, reason], dtype=np.int64)


def optimize_hyperparameters(gp, x0, *, lb, ub, priors=None, max_iter=200, history=8, tol_g=1e-5, tol_f=1e-9, device=True,
                             ctx=None, trace=False):
    """Maximise ``lml + log prior`` over the hyper-parameters of ``gp`` inside ``[lb, ub]``: R quasi-Newton runs, one per
    row of ``x0`` (R, P), each independent of the others.

    ``gp`` is read as ``log_marginal_likelihood`` reads it; ``lb``, ``ub`` finite (``lb == ub`` fixes a parameter);
    ``priors`` as ``hyper_log_prior`` takes them.  The optimiser is the package's own box-constrained limited-memory BFGS
    (``history`` pairs, 1 to 16; projected gradient; backtracking Armijo search of at most 30 halvings; csrc/gp_opt.hip's
    header states it), not SciPy's L-BFGS-B.  A run stops on max |projected gradient| <= ``tol_g`` (reason 1), on
    ``max_iter`` iterations (2), on a decrease of at most ``tol_f`` max(1, |value|) after an accepted step (3), or on an
    exhausted line search (4).
    ``device=True``: the runs advance in lockstep on the device (vbmc_gp_hyp_optimize), every evaluation round one batch
    of R trial points through vbmc_gp_lml's factorisation and gradient kernels; the posterior the context holds is
    untouched.  Shapes the device refuses (D > 32, a noise bound that allows sn2_div < 1e-6, noise that is not
    constant-additive) and ``device=False`` run the same algorithm in NumPy over the host lml, run by run.
    Returns ``dict(hyp (R, P), log_post (R,), grad (R, P), stats (R, 4))``: the final points, ``lml + log prior`` and its
    gradient there, and [iterations, evaluations, history resets, stop reason]; with ``trace=True`` also ``trace``, a dict
    ``iters`` (R, max_iter + 1, 3 P + 3), rows [x, phi, g, d, pairs held, reset flag], and ``evals`` (R, 1 + 31 (max_iter
    + 1), 4), rows [iteration, t, phi_trial, accepted]; rows not reached are zeros.  ``ValueError("Invalid value.")`` when
    a start has no finite value."""
    q = _hyper_problem("optimize_hyperparameters", "R", gp, x0, lb, ub, priors, ctx, device)
    X, y, N, D, kind, P, x0, lb, ub, pri = q.X, q.y, q.N, q.D, q.kind, q.P, q.x0, q.lb, q.ub, q.pri
    R = x0.shape[0]
    max_iter, m, tol_g, tol_f = int(max_iter), int(history), float(tol_g), float(tol_f)
    if max_iter < 0 or not 1 <= m <= 16 or not tol_g >= 0 or not tol_f >= 0:
        raise ValueError("optimize_hyperparameters: max_iter >= 0, 1 <= history <= 16, tol_g >= 0, tol_f >= 0")
    cap = max_iter + 1
    n_evr = 1 + 31 * cap
    if q.ctx is not None:
        hyp, lpost, grad = np.zeros((R, P)), np.zeros(R), np.zeros((R, P))
        stats, invalid = np.zeros((R, 4), dtype=np.int64), np.zeros(R, dtype=np.int32)
        t_it = np.zeros((R, cap, 3 * P + 3)) if trace else None
        t_ev = np.zeros((R, n_evr, 4)) if trace else None
        rc = q.ctx._lib.vbmc_gp_hyp_optimize(
            q.ctx._h, N, D, P, kind, _lib.ptr(X), _lib.ptr(y), _lib.ptr(q.s2), R, _lib.ptr(x0), _lib.ptr(lb), _lib.ptr(ub),
            _lib.ptr(q.mu), _lib.ptr(q.sigma), _lib.ptr(q.df), max_iter, m, tol_g, tol_f, cap if trace else 0, _lib.ptr(hyp),
            _lib.ptr(lpost), _lib.ptr(grad), stats.ctypes.data_as(C.POINTER(C.c_int64)),
            invalid.ctypes.data_as(C.POINTER(C.c_int32)), _lib.ptr(t_it), _lib.ptr(t_ev))
        if rc != _lib.E_UNSUP:
            q.ctx.check(rc)
            if np.any(invalid):
                raise ValueError("Invalid value.")
            out = dict(hyp=hyp, log_post=lpost, grad=grad, stats=stats)
            if trace:
                out["trace"] = dict(iters=t_it, evals=t_ev)
            return out

    def fun(h):
        with np.errstate(all="ignore"):
            sn2 = _noise_var(gp, h[D + 1 : D + 2])
            dsn2 = 2.0 * np.exp(2 * h[D + 1]) if q.const_add else 0.0
            lml, dl = _host_lml(X, y, kind, h, sn2, np.min(sn2), dsn2, True)
            lp, dp = hyper_log_prior(h, pri, grad=True)
            phi, g = -(lml + lp), -(dl + dp)
        if not (np.isfinite(phi) and np.all(np.isfinite(g))):
            return np.inf, np.zeros(P)
        return float(phi), g

    hyp, lpost, grad = np.zeros((R, P)), np.zeros(R), np.zeros((R, P))
    stats = np.zeros((R, 4), dtype=np.int64)
    t_it, t_ev = np.zeros((R, cap, 3 * P + 3)), np.zeros((R, n_evr, 4))
    for r in range(R):
        tr = {}
        x, phi, g, stats[r] = _lbfgs_run(fun, x0[r], lb, ub, max_iter, m, tol_g, tol_f, trace=tr)
        hyp[r], lpost[r], grad[r] = x, -phi, -g
        t_it[r, : len(tr["iters"])] = tr["iters"]
        t_ev[r, : len(tr["evals"])] = tr["evals"]
    out = dict(hyp=hyp, log_post=lpost, grad=grad, stats=stats)
    if trace:
        out["trace"] = dict(iters=t_it, evals=t_ev)
    return out


# ------------------------------------------------------------------------------------- the fused fit's own stages
_FIT_STREAM = 10


def fit_design(init_N, dlb, dub, seed):
    """The drawn candidates of ``GP.fit(optimizer="fused")`` (init_N, P), the statement of csrc/gp_fit.hip's design kernel:
    coordinate p of row j is ``clip(dlb_p + (dub_p - dlb_p) u, dlb_p, dub_p)`` with u = bits * 2^-53, bits the upper 53
    bits of words 0, 1 of Philox block (p, 0, j, stream 10) under ``seed``.  One product and one sum, each rounded, so
    the device's rows are these bits."""
    dlb, dub = np.asarray(dlb, dtype=np.float64), np.asarray(dub, dtype=np.float64)
    P = dlb.size
    out = np.empty((max(int(init_N), 0), P))
    for j in range(out.shape[0]):
        u = np.array([_philox_bits53(p, j, seed, _FIT_STREAM) for p in range(P)], dtype=np.float64) * 2.0**-53
        out[j] = np.maximum(np.minimum(dlb + (dub - dlb) * u, dub), dlb)
    return out


def fit_rank(score):
    """``(score with NaN and +inf as -inf, order)``: the candidates by score descending, ties to the lower index -- the
    stable ``argsort(-score)`` of ``GP.fit``, what csrc/gp_fit.hip's counting rank produces."""
    score = np.array(score, dtype=np.float64)
    score[~np.isfinite(score)] = -np.inf
    return score, np.argsort(-score, kind="stable")


def fit_select(best_f, run_log_post, run_invalid):
    """The optimum of the fused fit by ``GP.fit``'s lockstep-branch rule: ``(k, f)`` with k the first run of greatest
    finite log posterior among the valid ones where that is strictly greater than the best candidate's score
    ``best_f``, else ``(-1, best_f)``: the best candidate stays."""
    k, bl = -1, -np.inf
    for r, (lp, inv) in enumerate(zip(np.ravel(run_log_post), np.ravel(run_invalid))):
        if not inv and np.isfinite(lp) and lp > bl:
            k, bl = r, float(lp)
    return (k, bl) if k >= 0 and bl > best_f else (-1, float(best_f))


# hyper-parameter blocks by gpyreg's names, in the layout of hyp: (name, first index, length) for a GP of dimension D
def _hyp_blocks(D, mean_n):
    blocks = [("covariance_log_lengthscale", 0, D), ("covariance_log_outputscale", D, 1), ("noise_log_scale", D + 1, 1)]
    if mean_n >= 1:
        blocks.append(("mean_const", D + 2, 1))
    if mean_n == 1 + 2 * D:
        blocks += [("mean_location", D + 3, D), ("mean_log_scale", 2 * D + 3, D)]
    return blocks


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
        P = D + 2 + mean.hyperparameter_count(D)
        self._bounds = {"lb": np.full(P, -np.inf), "ub": np.full(P, np.inf)}
        # the priors of hyper-parameter fitting, one entry per parameter: sigma NaN = no prior, df +inf = Gaussian
        self.hyper_priors = {"mu": np.full(P, np.nan), "sigma": np.full(P, np.nan), "df": np.full(P, np.nan)}

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
            sn2_div=float(sn2_div),
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

    def append(self, x_new, y_new, s2_new=None, *, device=True, fetch=True):
        """Add ONE training point: ``X``, ``y`` (and ``s2``) grow by a row and the posterior records follow.

        This class's ``update(X_new, y_new)`` REPLACES the training data; gpyreg's ``update(xnew, ynew)`` -- what the
        reference calls after every acquired point (vbmc/active_sample.py:584) -- APPENDS to it.  ``append`` is that
        call for this class: ``append_point(self, ...)``.  With ``device=True`` and the context holding this GP's
        posterior as the device built it (``update(device=True)``, ``device_posterior`` or an earlier ``append``), the
        factor, its inverse and ``alpha`` are extended on the device in O(S N^2) (vbmc_gp_append; under user-provided
        noise, with ``s2_new``, vbmc_gp_append_noisy); otherwise the call is ``update`` on the extended data.  ``fetch``
        as in ``device_posterior``."""
        append_point(self, x_new, y_new, s2_new, ctx=self.ctx if device else None, device=device, fetch=fetch)

    def log_likelihood(self, hyp=None, grad=False, *, device=True):
        """``log_marginal_likelihood`` of this GP: ``hyp`` (B, P), default the present records' samples."""
        if hyp is None:
            hyp = np.stack([np.ravel(p.hyp) for p in self.posteriors])
        return log_marginal_likelihood(self, hyp, grad=grad, device=device, ctx=self.ctx if device else None)

    def get_hyperparameters(self, as_array=True):
        return np.stack([p.hyp for p in self.posteriors])

    # ------------------------------------------------------------------------------------ hyper-parameter fitting
    def _blocks(self):
        return _hyp_blocks(self.D, self.mean.hyperparameter_count(self.D))

    def _block_of(self, name):
        for nm, first, length in self._blocks():
            if nm == name:
                return slice(first, first + length)
        raise ValueError(f"this GP has no hyper-parameter block '{name}'")

    @staticmethod
    def _fill(dst, sl, values):
        """dst[sl] = values (a scalar or the block's length), NaN entries leaving a slot as it was"""
        v = np.array(np.broadcast_to(np.asarray(values, dtype=np.float64), dst[sl].shape))
        keep = np.isnan(v)
        v[keep] = dst[sl][keep]
        dst[sl] = v

    def set_bounds(self, bounds):
        """Bounds of the hyper-parameters: the array form ``{"lb": (P,), "ub": (P,)}`` or gpyreg's name-keyed form
        ``{"noise_log_scale": (lb, ub), ...}`` (the blocks of ``get_bounds``; scalars or the block's length).  NaN entries
        leave a slot as it was."""
        if set(bounds) <= {"lb", "ub"}:
            for k, v in bounds.items():
                self._fill(self._bounds[k], slice(None), v)
            return
        for name, pair in bounds.items():
            if pair is None:
                continue
            sl = self._block_of(name)
            self._fill(self._bounds["lb"], sl, pair[0])
            self._fill(self._bounds["ub"], sl, pair[1])

    def get_bounds(self, as_array=False):
        """``{name: (lb, ub)}`` per block (``covariance_log_lengthscale`` (D), ``covariance_log_outputscale``,
        ``noise_log_scale``, ``mean_const``, ``mean_location`` (D), ``mean_log_scale`` (D), as far as the mean has them), or
        copies of the arrays ``{"lb", "ub"}`` with ``as_array``."""
        if as_array:
            return {k: v.copy() for k, v in self._bounds.items()}
        return {nm: (self._bounds["lb"][f : f + n].copy(), self._bounds["ub"][f : f + n].copy()) for nm, f, n in self._blocks()}

    def set_priors(self, priors):
        """Priors of the hyper-parameters: the array form ``{"mu", "sigma", "df"}`` (P entries each; sigma NaN = no prior, df
        +inf = Gaussian) or gpyreg's name-keyed form ``{"noise_log_scale": ("student_t", (mu, sigma, df)), ...}`` with
        ``("gaussian", (mu, sigma))`` and None (no prior) as the other kinds.  NaN entries leave a slot as it was."""
        hp = self.hyper_priors
        if set(priors) <= {"mu", "sigma", "df"}:
            for k, v in priors.items():
                self._fill(hp[k], slice(None), v)
            return
        for name, spec in priors.items():
            sl = self._block_of(name)
            if spec is None:
                for k in ("mu", "sigma", "df"):
                    hp[k][sl] = np.nan
                continue
            kind, par = spec
            if kind == "student_t":
                mu, sigma, df = par
            elif kind == "gaussian":
                (mu, sigma), df = par, np.inf
            else:
                raise NotImplementedError(f"hyper prior '{kind}': only 'gaussian' and 'student_t' are supported")
            self._fill(hp["mu"], sl, mu)
            self._fill(hp["sigma"], sl, sigma)
            self._fill(hp["df"], sl, df)

    def get_priors(self, as_array=False):
        """``{name: spec}`` per block in ``set_priors``' name-keyed form (None: no prior on the whole block), or copies of
        the arrays with ``as_array``."""
        hp = self.hyper_priors
        if as_array:
            return {k: v.copy() for k, v in hp.items()}
        out = {}
        for nm, f, n in self._blocks():
            mu, sigma, df = (hp[k][f : f + n].copy() for k in ("mu", "sigma", "df"))
            if np.all(np.isnan(sigma)):
                out[nm] = None
            elif np.all(np.isinf(df[~np.isnan(sigma)])):
                out[nm] = ("gaussian", (mu, sigma))
            else:
                out[nm] = ("student_t", (mu, sigma, df))
        return out

    def fit(self, X=None, y=None, s2=None, hyp0=None, options=None, *, device=True, seed=None, optimizer="scipy"):
        """Fit the hyper-parameters to the training data (``X``, ``y``, ``s2`` REPLACE the GP's when given) inside the
        bounds of ``set_bounds`` (finite ones are required) under the priors of ``set_priors``:

        1. candidates: the rows of ``hyp0`` (default: the present records' samples, else the middle of the box) clipped
           into the bounds, plus ``init_N`` uniform draws in the box from ``np.random.default_rng(seed)``; all of them are
           scored in ONE ``log_marginal_likelihood`` batch, plus the prior;
        2. SciPy L-BFGS-B inside the bounds from the best ``opts_N`` of them on -(lml + log prior) with its gradient
           (tolerance ``tol_opt``); the best point seen is the optimum.  ``optimizer="lockstep"``: the best ``opts_N``
           candidates with a finite score go to ONE ``optimize_hyperparameters`` call instead (``tol_g = tol_opt``; on the
           device every evaluation round is one batch of ``opts_N`` trial points), and the best result is the optimum;
           ``n_iterations`` is the sum over the runs;
        3. ``n_samples`` > 0: that many slice chains from the optimum, one kept sample each after ``burn`` sweeps and
           ``thin`` more (``sample_hyperparameters``; ``widths`` as given, else (ub - lb) / 8);
        4. ``update(hyp=samples, device=device)``: with the device route the posterior stays installed.

        ``options``: a dict with ``init_N`` (0), ``opts_N`` (1), ``n_samples`` (0), ``thin`` (1), ``burn`` (0), ``widths``
        (None), ``tol_opt`` (1e-5) -- the keys the reference's ``_get_gp_training_options`` fills.  Returns ``(hyp (S, P),
        optimize_result, sample_result)``: ``optimize_result`` a dict ``hyp``, ``log_post``, ``candidates``,
        ``candidate_log_post``, ``n_iterations``; ``sample_result`` (None without sampling) a dict ``samples`` (S, P),
        ``log_priors`` (S,), ``log_post`` (S,), ``stats`` (S, 4).  gpyreg's own design of starting points, its default
        bounds and its random stream are not reproduced.

        ``optimizer="fused"`` (opt-in; the two routes above and their results are unchanged): the same stages as one
        device call with a counter-based design in its own box and the chains under the same ``seed`` -- ``_fit_fused``
        states them; it also reads the option keys ``design_lb`` / ``design_ub``."""
        import scipy.optimize as sopt

        opts = {"init_N": 0, "opts_N": 1, "n_samples": 0, "thin": 1, "burn": 0, "widths": None, "tol_opt": 1e-5}
        opts.update({k: v for k, v in (options or {}).items() if k in opts and v is not None})
        if X is not None:
            self.X = np.atleast_2d(np.asarray(X, dtype=np.float64))
            self.y = np.asarray(y, dtype=np.float64).reshape(-1, 1)
            self.s2 = None if s2 is None else np.asarray(s2, dtype=np.float64).reshape(-1, 1)
        lb, ub = self._bounds["lb"].copy(), self._bounds["ub"].copy()
        if not (np.all(np.isfinite(lb)) and np.all(np.isfinite(ub)) and np.all(lb <= ub)):
            raise ValueError("GP.fit: finite bounds with lb <= ub are required (set_bounds)")
        P = lb.size
        pri = self.hyper_priors
        ctx = self.ctx if device else None
        if hyp0 is None:
            hyp0 = np.stack([np.ravel(p.hyp) for p in self.posteriors]) if self.posteriors is not None else 0.5 * (lb + ub)
        hyp0 = np.atleast_2d(np.asarray(hyp0, dtype=np.float64))
        if hyp0.shape[1] != P:
            raise ValueError(f"GP.fit: hyp0 has {hyp0.shape[1]} columns, the GP takes {P}")
        if optimizer == "fused":
            return self._fit_fused(hyp0, opts, options or {}, lb, ub, device, seed)
        rng = np.random.default_rng(seed)
        cand = np.clip(hyp0, lb, ub)
        if int(opts["init_N"]) > 0:
            cand = np.vstack([cand, lb + (ub - lb) * rng.random((int(opts["init_N"]), P))])
        score = log_marginal_likelihood(self, cand, device=device, ctx=ctx) + hyper_log_prior(cand, pri)
        score = np.where(np.isnan(score), -np.inf, score)
        if not np.any(np.isfinite(score)):
            raise ValueError("GP.fit: no candidate has a finite log posterior")

        def neg(h):
            lml, dl = log_marginal_likelihood(self, h[None, :], grad=True, device=device, ctx=ctx)
            lp, dp = hyper_log_prior(h, pri, grad=True)
            if not (np.isfinite(lml[0]) and np.all(np.isfinite(dl[0]))):
                return 1e100, np.zeros(P)
            return -(lml[0] + lp), -(dl[0] + dp)

        if optimizer not in ("scipy", "lockstep"):
            raise ValueError(f"GP.fit: optimizer '{optimizer}' is not 'scipy', 'lockstep' or 'fused'")
        order = np.argsort(-score, kind="stable")
        best_h, best_f, n_it = cand[order[0]].copy(), float(score[order[0]]), 0
        if optimizer == "lockstep":
            starts = [i for i in order[: max(int(opts["opts_N"]), 0)] if np.isfinite(score[i])]
            if starts:
                res = optimize_hyperparameters(self, cand[starts], lb=lb, ub=ub, priors=pri, tol_g=float(opts["tol_opt"]),
                                               device=device, ctx=ctx)
                n_it = int(np.sum(res["stats"][:, 0]))
                k = int(np.argmax(res["log_post"]))
                if np.isfinite(res["log_post"][k]) and res["log_post"][k] > best_f:
                    best_h, best_f = res["hyp"][k].copy(), float(res["log_post"][k])
        for i in order[: max(int(opts["opts_N"]), 0) if optimizer == "scipy" else 0]:
            if not np.isfinite(score[i]):
                continue
            res = sopt.minimize(neg, cand[i], jac=True, method="L-BFGS-B", bounds=list(zip(lb, ub)), tol=float(opts["tol_opt"]))
            n_it += int(res.nit)
            h = np.clip(res.x, lb, ub)
            f = float(log_marginal_likelihood(self, h[None, :], device=device, ctx=ctx)[0] + hyper_log_prior(h, pri))
            if np.isfinite(f) and f > best_f:
                best_h, best_f = h, f
        opt_res = dict(hyp=best_h, log_post=best_f, candidates=cand, candidate_log_post=score, n_iterations=n_it)
        S = int(opts["n_samples"])
        if S <= 0:
            hyp, smp_res = best_h[None, :], None
        else:
            widths = (ub - lb) / 8 if opts["widths"] is None else np.asarray(opts["widths"], dtype=np.float64)
            sub = None if seed is None else int(rng.integers(0, 2**63))
            r = sample_hyperparameters(self, np.tile(best_h, (S, 1)), lb=lb, ub=ub, widths=widths, priors=pri, n=1,
                                       thin=int(opts["thin"]), burn_in=int(opts["burn"]), seed=sub, device=device, ctx=ctx)
            hyp = r["samples"][:, 0, :]
            smp_res = dict(samples=hyp, log_priors=r["log_priors"][:, 0], log_post=r["log_post"][:, 0], stats=r["stats"])
        self.update(hyp=hyp, device=device)
        return hyp, opt_res, smp_res

    def _fit_fused(self, hyp0, opts, options, lb, ub, device, seed):
        """``fit(optimizer="fused")``: the stages of ``fit`` as ONE device call (vbmc_gp_fit, csrc/api_gp_fit.hip) with
        the hand-overs done by kernels, or -- ``device=False``, and the shapes the device refuses (D > 32, a noise bound
        that allows sn2_div < 1e-6, noise that is not constant-additive) -- the same stages in NumPy, which is the
        statement of the algorithm:

        1. candidates: ``hyp0`` clipped into the bounds, then ``init_N`` rows of ``fit_design`` in the design box
           ``design_lb`` / ``design_ub`` (option keys; default the hard box) -- counter-based draws under ``seed``, the
           same bits on both routes;
        2. score = lml + log prior, NaN / not positive definite = -inf; ``fit_rank`` orders them; the first ``opts_N`` are
           the optimiser's starts (``optimize_result["starts"]``), one without a finite score an invalid run;
        3. ``optimize_hyperparameters`` from the starts; ``fit_select`` forms the optimum;
        4. ``n_samples`` chains of ``sample_hyperparameters`` from the optimum under the same ``seed``, one kept sample
           each after ``burn`` sweeps and ``thin`` more;
        5. the posterior at the samples (the optimum without sampling), left installed on the device route.

        Returns ``fit``'s triple; ``optimize_result`` also has ``starts`` and ``runs`` (the optimiser's ``hyp``,
        ``log_post``, ``stats``, ``invalid`` per start)."""
        P, pri = lb.size, self.hyper_priors
        dlb = lb.copy() if options.get("design_lb") is None else np.array(np.broadcast_to(np.asarray(options["design_lb"], dtype=np.float64), (P,)))
        dub = ub.copy() if options.get("design_ub") is None else np.array(np.broadcast_to(np.asarray(options["design_ub"], dtype=np.float64), (P,)))
        if not (np.all(dlb >= lb) and np.all(dub <= ub) and np.all(dlb <= dub)):
            raise ValueError("GP.fit: the design box must lie inside the bounds, with design_lb <= design_ub")
        init_N, opts_N, S = (max(int(opts[k]), 0) for k in ("init_N", "opts_N", "n_samples"))
        thin, burn, tol = int(opts["thin"]), int(opts["burn"]), float(opts["tol_opt"])
        H = hyp0.shape[0]
        B = H + init_N
        if B < 1:
            raise ValueError("GP.fit: no candidate (hyp0 is empty and init_N = 0)")
        widths = (ub - lb) / 8 if opts["widths"] is None else np.asarray(opts["widths"], dtype=np.float64)
        widths = _lib.f64(np.array(np.broadcast_to(widths, (P,))))
        if S > 0 and not (np.all(widths > 0) and np.all(np.isfinite(widths)) and thin >= 1 and burn >= 0):
            raise ValueError("GP.fit: widths must be positive, thin >= 1, burn >= 0")
        seed = int(np.random.SeedSequence().generate_state(2, np.uint32).view(np.uint64)[0]) if seed is None else int(seed)
        seed &= 0xFFFFFFFFFFFFFFFF
        q = _hyper_problem("GP.fit", "H", self, lb[None, :], lb, ub, pri, self.ctx if device else None, device)
        X, y, N, D = q.X, q.y, q.N, q.D
        R, Sn = min(opts_N, B), max(S, 1)
        max_iter, m, tol_f = 200, 8, 1e-9  # optimize_hyperparameters' defaults, as fit(optimizer="lockstep") runs it
        if q.ctx is not None:
            h0, dl, du = _lib.f64(hyp0), _lib.f64(dlb), _lib.f64(dub)
            cand, score, starts = np.zeros((B, P)), np.zeros(B), np.zeros(R, dtype=np.int32)
            o_hyp, o_lp = np.zeros((R, P)), np.zeros(R)
            o_stats, o_inv = np.zeros((R, 4), dtype=np.int64), np.zeros(R, dtype=np.int32)
            best, best_lp = np.zeros(P), np.zeros(1)
            hyp, lpost, lprior = np.zeros((Sn, P)), np.zeros(Sn), np.zeros(Sn)
            stats, noise, status = np.zeros((Sn, 4), dtype=np.int64), np.zeros(Sn), np.zeros(1, dtype=np.int32)
            alpha, L = np.empty((Sn, N)), np.empty((Sn, N, N))
            i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
            rc = q.ctx._lib.vbmc_gp_fit(
                q.ctx._h, N, D, P, q.kind, _lib.ptr(X), _lib.ptr(y), _lib.ptr(q.s2), H, _lib.ptr(h0) if H else None, init_N,
                _lib.ptr(dl), _lib.ptr(du), _lib.ptr(q.lb), _lib.ptr(q.ub), _lib.ptr(q.mu), _lib.ptr(q.sigma),
                _lib.ptr(q.df), opts_N, max_iter, m, tol, tol_f, S, _lib.ptr(widths), thin, burn, C.c_uint64(seed),
                _lib.ptr(cand), _lib.ptr(score), starts.ctypes.data_as(i32), _lib.ptr(o_hyp), _lib.ptr(o_lp),
                o_stats.ctypes.data_as(i64), o_inv.ctypes.data_as(i32), _lib.ptr(best), _lib.ptr(best_lp), _lib.ptr(hyp),
                _lib.ptr(lpost), _lib.ptr(lprior), stats.ctypes.data_as(i64), _lib.ptr(noise), status.ctypes.data_as(i32),
                _lib.ptr(alpha), _lib.ptr(L))
            if rc != _lib.E_UNSUP:
                q.ctx.check(rc)
                if status[0] & 1:
                    raise ValueError("GP.fit: no candidate has a finite log posterior")
                runs = dict(hyp=o_hyp, log_post=o_lp, stats=o_stats, invalid=o_inv)
                opt_res = dict(hyp=best, log_post=float(best_lp[0]), candidates=cand, candidate_log_post=score,
                               n_iterations=int(np.sum(o_stats[:, 0])), starts=starts.astype(np.int64), runs=runs)
                smp_res = dict(samples=hyp, log_priors=lprior, log_post=lpost, stats=stats) if S > 0 else None
                sn2_div = noise + (0.0 if q.s2 is None else float(np.min(q.s2)))
                self.posteriors = _records(hyp, alpha, L, 1.0 / np.sqrt(sn2_div * 1.0), sn2_div, noise)
                _adopt(self, q.ctx, dev=True)
                return hyp, opt_res, smp_res

        # ---- the host route: the statement of the stages
        cand = np.vstack([np.clip(hyp0, lb, ub), fit_design(init_N, dlb, dub, seed)])
        finite_rows = np.all(np.isfinite(cand), axis=1)
        score = np.full(B, -np.inf)
        if np.any(finite_rows):
            rows = cand[finite_rows]
            with np.errstate(all="ignore"):
                score[finite_rows] = log_marginal_likelihood(self, rows, device=False) + hyper_log_prior(rows, pri)
        score, order = fit_rank(score)
        if not np.any(np.isfinite(score)):
            raise ValueError("GP.fit: no candidate has a finite log posterior")
        starts = order[:R].astype(np.int64)
        o_hyp, o_lp = np.zeros((R, P)), np.zeros(R)
        o_stats, o_inv = np.zeros((R, 4), dtype=np.int64), np.zeros(R, dtype=np.int32)
        for r, i in enumerate(starts):  # (the runs are independent of each other: one call each finds the invalid ones)
            try:
                if not np.isfinite(score[i]):
                    raise ValueError("Invalid value.")
                res = optimize_hyperparameters(self, cand[i][None, :], lb=lb, ub=ub, priors=pri, max_iter=max_iter, history=m,
                                               tol_g=tol, tol_f=tol_f, device=False)
                o_hyp[r], o_lp[r], o_stats[r] = res["hyp"][0], res["log_post"][0], res["stats"][0]
            except ValueError:
                o_inv[r] = 1
        k, best_f = fit_select(float(score[order[0]]), o_lp, o_inv)
        best_h = (o_hyp[k] if k >= 0 else cand[order[0]]).copy()
        runs = dict(hyp=o_hyp, log_post=o_lp, stats=o_stats, invalid=o_inv)
        opt_res = dict(hyp=best_h, log_post=best_f, candidates=cand, candidate_log_post=score,
                       n_iterations=int(np.sum(o_stats[:, 0])), starts=starts, runs=runs)
        if S <= 0:
            hyp, smp_res = best_h[None, :].copy(), None
        else:
            r = sample_hyperparameters(self, np.tile(best_h, (S, 1)), lb=lb, ub=ub, widths=widths, priors=pri, n=1, thin=thin,
                                       burn_in=burn, seed=seed, device=False)
            hyp = r["samples"][:, 0, :]
            smp_res = dict(samples=hyp, log_priors=r["log_priors"][:, 0], log_post=r["log_post"][:, 0], stats=r["stats"])
        self.update(hyp=hyp, device=False)
        return hyp, opt_res, smp_res

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
