"""``active_importance_sampling`` -- mirror of the reference's ``pyvbmc/vbmc/active_importance_sampling.py``: the
importance state ``AcqFcnVIQR`` / ``AcqFcnIMIQR`` consume, prepared on the MI355X.

Same names and signatures as the reference (``active_importance_sampling`` :10, ``active_sample_proposal_pdf``
:317, ``get_mcmc_opts`` :393, ``fess`` :426, ``renormalize_weights`` :481); ``vp``, ``gp``, the acquisition object and
``options`` are taken by duck typing -- the reference's own objects, this package's, or attribute-only stand-ins --
and ``options`` may be a plain ``dict`` or an object with ``.eval(key, env)``.

Where the work runs:

* the proposal weights (:317-390) -- separate-sample ``gp.predict``, the log density of the smoothed posterior, the
  box-uniform mixture around the training points and their log-sum-exp -- in one library call (``vbmc_is_proposal``,
  csrc/acq_is_prep.hip);
* step 3 (:264-308) -- ``K_Xa_X`` and ``C_tmp`` of every GP sample -- on the FP64 matrix cores against the ``L^-1`` the
  context already holds (``vbmc_acq_is_build``, csrc/api_acq_is.hip).  The result stays in the context as the state
  ``vbmc_acq_is_eval`` reads, so the mirror acquisition classes upload nothing when they receive the returned dict;
  ``products=False`` also keeps ``K_Xa_X`` / ``C_tmp`` (S N Na doubles each) off the bus and out of the dict;
* step 2, the optional MCMC (:195-262), is by default a host loop around a slice-sampler class with the reference's data
  flow; its ``log_p`` is the acquisition's ``is_log_full`` on the device ``gp.predict``, one point per call.  With
  ``sampler="device"`` (or ``VBMC_HIP_AIS_SAMPLER=device`` when ``sampler`` is None) the S chains run as ONE launch
  instead (``vbmc_is_mcmc``, csrc/acq_is_mcmc.hip): one batched ``predict`` on the old points, the resampling weights
  and one ``np.random.choice`` per GP sample exactly as in the host loop, then all chains at once; the launch also
  returns ``f_mu`` / ``f_s2`` at the kept points, so the second ``predict`` (:254) is not run.  The device sampler is
  this package's own -- Neal's coordinate-wise slice sampler with stepping out and shrinkage on the Philox stream 6,
  stated in NumPy by tests/slice_host.py -- and NOT gpyreg's: it targets the same density, but its draws are its own
  stream, neither ``np.random``'s nor gpyreg's.  ``seed`` is taken as for ``rng="philox"``.  Cap counters that are not
  zero come back under ``ais["mcmc_stats"]``.  Step 0's MCMC pass (VIQR with ``mcmc_importance_sampling``) hands a
  matrix of walkers to the sampler and stays on the class route: ``sampler="device"`` there raises
  ``NotImplementedError``.

Draws: by default (``rng="numpy"``) ``np.random`` is consumed exactly as the reference consumes it -- the same calls in
the same order -- so the same global state gives the reference's ``X``.  ``rng="philox"`` (or ``VBMC_HIP_RNG=philox``)
takes the smoothed-posterior samples from the device sampler and the box samples from its stream 5
(``vbmc_is_box_sample``); ``seed`` as for ``VariationalPosterior.sample``.

A shape the kernels do not cover (D > 32) raises ``_lib.UnsupportedShape`` before anything is drawn or changed.
"""
import ctypes as C
import os
import sys
from math import ceil

import numpy as np

from . import _lib
from ._duck import ctx_of, upload_vp
from .gp import upload_gp
from .variational_posterior import IdentityTransformer, VariationalPosterior, _mixture_args, _rng_mode, _seed_or_draw

SMOOTH_SCALES = (0.05, 0.2, 1.0)  # widths added to sigma in the smoothed posterior (:127)


# ------------------------------------------------------------------------------------------------ small helpers
def renormalize_weights(ln_w):
    """``ln_w`` minus the log of the sum of its exponentials (:481-483)."""
    top = np.amax(ln_w)
    return ln_w - (top + np.log(np.sum(np.exp(ln_w - top))))


def get_mcmc_opts(Ns, thin=1, burn_in=None):
    """``(sampler_opts, thin, burn_in)`` with the reference's defaults (:393-423): no display, no diagnostics,
    ``burn_in = ceil(thin Ns / 2)``."""
    if burn_in is None:
        burn_in = ceil(thin * Ns / 2)
    return {"display": "off", "diagnostics": False}, thin, burn_in


def _eval_option(options, key, env):
    """``options.eval(key, env)`` where the object has it; a plain dict's number as it is, its string evaluated in
    ``env`` (what the reference's ``Options.eval`` does with a string option)."""
    if hasattr(options, "eval"):
        return options.eval(key, env)
    v = options[key]
    if isinstance(v, str):
        return eval(v, {"np": np, "__builtins__": {}}, dict(env))  # noqa: S307 (the caller's own option string)
    return v


def _mirror_vp(vp, ctx, mu=None, sigma=None, w=None):
    """A ``VariationalPosterior`` of this package with the mixture attributes of ``vp`` (or the ones given), built
    without the constructor's ``np.random`` draw."""
    m = VariationalPosterior.__new__(VariationalPosterior)
    mu = np.array(vp.mu if mu is None else mu, dtype=np.float64)
    m.D, m.K = int(mu.shape[0]), int(mu.shape[1])
    m.mu = np.ascontiguousarray(mu)
    m.sigma = np.array(vp.sigma if sigma is None else sigma, dtype=np.float64).reshape(1, m.K)
    m.lambd = np.array(vp.lambd, dtype=np.float64).reshape(m.D, 1)
    m.w = np.array(vp.w if w is None else w, dtype=np.float64).reshape(1, m.K)
    with np.errstate(divide="ignore"):
        m.eta = np.log(m.w)
    m.optimize_mu = m.optimize_sigma = m.optimize_lambd = m.optimize_weights = True
    m.parameter_transformer = getattr(vp, "parameter_transformer", None) or IdentityTransformer(m.D)
    m.bounds = m.stats = m._mode = None
    m._ctx = ctx
    return m


def smoothed_posterior(vp, ctx=None):
    """The proposal's smoothed posterior (:126-137): the components of ``vp`` and three more copies of them with
    ``sigma' = sqrt(sigma^2 + s^2)``, s = 0.05, 0.2, 1, all weights renormalised -- 4 K components."""
    mu = np.asarray(vp.mu, dtype=np.float64).reshape(vp.D, vp.K)
    sg = np.asarray(vp.sigma, dtype=np.float64).reshape(1, vp.K)
    w = np.asarray(vp.w, dtype=np.float64).reshape(1, vp.K)
    mus, sgs, ws = [mu], [sg], [w]
    for s in SMOOTH_SCALES:
        mus.append(mu)
        sgs.append(np.sqrt(sg**2 + s**2))
        ws.append(w)
    w_all = np.hstack(ws)
    return _mirror_vp(vp, ctx, np.hstack(mus), np.hstack(sgs), w_all / np.sum(w_all))


class _DeviceGP:
    """The GP (or one hyper-parameter sample of it, :205-209) as the host-side callers of step 2 need it: the
    attributes ``upload_gp`` reads and ``predict`` on the device."""

    def __init__(self, gp, ctx, sample=None):
        self._gp, self._ctx = gp, ctx
        self.X, self.mean = gp.X, gp.mean
        self.D = gp.X.shape[1]
        if sample is None:
            self.posteriors = gp.posteriors
        else:
            self.posteriors = np.empty(1, dtype=object)
            self.posteriors[0] = gp.posteriors[sample]
        self.temporary_data = getattr(gp, "temporary_data", {})

    def predict(self, x_star, y_star=None, s2_star=0, add_noise=False, separate_samples=False):
        return _predict(self, self._ctx, x_star, add_noise=add_noise, separate_samples=separate_samples)


def _predict(gp, ctx, x, add_noise=False, separate_samples=False):
    """``gp.predict`` of any GP duck type on the device (vbmc_gp_predict)."""
    upload_gp(gp, ctx)
    xs = _lib.f64(np.atleast_2d(x))
    M, S = xs.shape[0], len(gp.posteriors)
    shape = (M, S) if separate_samples else (M, 1)
    fmu, fs2 = np.empty(shape), np.empty(shape)
    ctx.check(ctx._lib.vbmc_gp_predict(ctx._h, M, _lib.ptr(xs), int(bool(add_noise)), int(bool(separate_samples)),
                                       _lib.ptr(fmu), _lib.ptr(fs2)))
    return fmu, fs2


def _log_pdf(vp, ctx, x):
    """``vp.pdf(x, orig_flag=False, log_flag=True)`` of any VP duck type on the device, (n, 1)."""
    upload_vp(vp, ctx)
    xs = _lib.f64(np.atleast_2d(x))
    y = np.empty(xs.shape[0])
    ctx.check(ctx._lib.vbmc_mixture_pdf(ctx._h, xs.shape[0], _lib.ptr(xs), 1, 0, float("inf"), _lib.ptr(y), None))
    return y.reshape(-1, 1)


def _check_shape(D):
    if D > 32:
        raise _lib.UnsupportedShape(f"active_importance_sampling: D={D} > 32 not supported")


MCMC_DEVICE_MAX_N = 9984  # a device chain keeps k and the product's stripe sums in LDS: 2 N doubles in 156 KiB


def _check_mcmc_shape(N):
    if N > MCMC_DEVICE_MAX_N:
        raise _lib.UnsupportedShape(f"active_importance_sampling: sampler='device' with N={N} > {MCMC_DEVICE_MAX_N} "
                                    "training points not supported")


# ------------------------------------------------------------------------------------------------ the reference's names
def fess(vp, gp, X=100):
    """Fractional effective sample size by importance sampling (:426-478): ``gp`` is a GP (its averaged predictive
    mean at ``X`` is taken on the device) or an (N, Ns_gp) array of separate means; ``X`` the points, or how many to
    draw from ``vp``."""
    ctx = ctx_of(vp)
    if np.isscalar(X):
        N = X
        X = _mirror_vp(vp, ctx).sample(N, orig_flag=False)[0]
    else:
        X = np.atleast_2d(X)
        N = X.shape[0]
    if isinstance(gp, np.ndarray):
        f_bar = np.mean(gp, axis=1)
    else:
        _check_shape(gp.X.shape[1])
        f_bar = _predict(gp, ctx, X)[0].ravel()
    if f_bar.shape[0] != X.shape[0]:
        raise ValueError("Mismatch between number of samples from VP and GP.")
    v_ln_pdf = np.maximum(_log_pdf(vp, ctx, X), np.log(sys.float_info.min)).ravel()
    ln_weights = f_bar - np.atleast_2d(v_ln_pdf)
    weight = np.exp(ln_weights - np.amax(ln_weights))
    weight = weight / np.sum(weight)
    return (1 / np.sum(weight**2)) / N


def active_sample_proposal_pdf(Xa, gp, vp_is, w_vp, rect_delta, acq_fcn):
    """Log importance weights of the proposal points ``Xa`` and the GP's predictive variances there, both
    ``(Na, Ns_gp)`` (:317-390), in one device call.  ``ln_y`` is the acquisition's ``is_log_base``: the predictive mean
    (IMIQR), or zero when the acquisition sets ``variational_importance_sampling`` (VIQR)."""
    ctx = ctx_of(vp_is if vp_is is not None else gp)
    Xa = _lib.f64(np.atleast_2d(Xa))
    Na, D = Xa.shape
    _check_shape(gp.X.shape[1])
    if D != gp.X.shape[1]:
        raise ValueError(f"points have {D} columns, the GP D={gp.X.shape[1]}")
    upload_gp(gp, ctx)
    S = len(gp.posteriors)
    w_vp = float(w_vp)
    mix = _mixture_args(vp_is) if w_vp > 0 else (None,) * 4
    rect = _lib.f64(np.ravel(rect_delta)) if w_vp < 1 else None
    lnw, fs2 = np.empty((Na, S)), np.empty((Na, S))
    invalid = C.c_int(0)
    ln_y_fmu = 0 if acq_fcn.acq_info.get("variational_importance_sampling") else 1
    ctx.check(ctx._lib.vbmc_is_proposal(ctx._h, Na, _lib.ptr(Xa), int(vp_is.K) if w_vp > 0 else 0, _lib.ptr(mix[0]),
                                        _lib.ptr(mix[1]), _lib.ptr(mix[2]), _lib.ptr(mix[3]), w_vp, _lib.ptr(rect),
                                        ln_y_fmu, _lib.ptr(lnw), _lib.ptr(fs2), C.byref(invalid)))
    if invalid.value:
        raise ValueError("Invalid value.")
    return lnw, fs2


def _default_sampler():
    try:
        from gpyreg.slice_sample import SliceSampler
    except ImportError as e:
        raise ImportError("active_importance_sampling: the MCMC step needs gpyreg.slice_sample.SliceSampler "
                          "(gpyreg is not installed); pass sampler=<class with the same interface>") from e
    return SliceSampler


def _device_sampler(sampler):
    """Whether step 2 runs as the device launch: ``sampler="device"``, or the environment's switch when it is None."""
    if sampler is None:
        return os.environ.get("VBMC_HIP_AIS_SAMPLER", "") == "device"
    return isinstance(sampler, str) and sampler == "device"


def _mcmc_device(ctx, gp, acq_fcn, old, n_mcmc, thin, burn_in, widths, lb, ub, seed):
    """Step 2 (:195-262) with the chains on the device: ``(ais, stats)`` -- the new dict and the (S, 4) counters
    [evaluations, draws, step-out caps, shrink caps] of ``vbmc_is_mcmc``."""
    X = np.asarray(gp.X, dtype=np.float64)
    S, D = len(gp.posteriors), X.shape[1]
    # the resampling weights of every GP sample from one batched predict on the old points (:211-226)
    f_mu, f_s2 = _predict(gp, ctx, old["X"], separate_samples=True)
    x0 = np.empty((S, D))
    for s in range(S):
        ln_w = old["ln_weights"][s, :].reshape(-1, 1) + acq_fcn.is_log_added(f_mu=f_mu[:, s:s + 1], f_s2=f_s2[:, s:s + 1])
        ln_w_max = np.amax(ln_w, axis=1).reshape(-1, 1)
        if np.any(ln_w_max == -np.inf):
            raise ValueError("Invalid value.")
        weights = np.exp(ln_w - ln_w_max).ravel()
        weights = weights / np.sum(weights)
        index = np.random.choice(a=len(weights), p=weights, replace=False)
        x0[s] = np.maximum(np.minimum(old["X"][index, :], ub), lb)
    Xa, log_p = np.empty((S, n_mcmc, D)), np.empty((S, n_mcmc))
    c_mu, c_s2 = np.empty((n_mcmc, S)), np.empty((n_mcmc, S))
    stats = np.zeros((S, 4), dtype=np.int64)
    invalid = C.c_int(0)
    u_q = float(acq_fcn.u)
    ln_y_fmu = 0 if acq_fcn.acq_info.get("variational_importance_sampling") else 1
    ctx.check(ctx._lib.vbmc_is_mcmc(ctx._h, ln_y_fmu, u_q, _lib.ptr(_lib.f64(x0)), _lib.ptr(_lib.f64(widths)),
                                    _lib.ptr(_lib.f64(lb)), _lib.ptr(_lib.f64(ub)), int(n_mcmc), int(thin), int(burn_in),
                                    C.c_uint64(int(seed)), _lib.ptr(Xa), _lib.ptr(log_p), _lib.ptr(c_mu), _lib.ptr(c_s2),
                                    stats.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(invalid)))
    if invalid.value:
        raise ValueError("Invalid value.")
    ais = {"ln_weights": np.zeros((S, n_mcmc)), "X": Xa, "f_s2": c_s2}
    for s in range(S):
        ln_y = acq_fcn.is_log_base(Xa[s], f_mu=c_mu[:, s:s + 1], f_s2=c_s2[:, s:s + 1])
        ais["ln_weights"][s, :] = ln_y.T - log_p[s]
    return ais, stats


def _box_samples(gp, ctx, n_box, rect_delta, mode, seed):
    """Box-uniform proposals around random training points (:164-168)."""
    X = gp.X
    if mode == "philox":
        out = np.empty((n_box, X.shape[1]))
        rect = _lib.f64(np.ravel(rect_delta))
        ctx.check(ctx._lib.vbmc_is_box_sample(ctx._h, n_box, C.c_uint64(int(seed)), _lib.ptr(rect), _lib.ptr(out)))
        return out
    jj = np.random.randint(0, len(X), size=(n_box,))
    return X[jj, :] + (2 * np.random.rand(jj.size, X.shape[1]) - 1) * rect_delta


def _build_state(ctx, gp, acq_fcn, ais, products):
    """Step 3 (:264-308) on the device: the products go into the context's importance state; with ``products`` also
    into ``ais``.  Leaves the context keyed to ``ais`` (acquisition._QuantileAcq._upload_state)."""
    from .acquisition import _is_state_key

    upload_gp(gp, ctx)
    Xa = _lib.f64(ais["X"])
    Na, N, S = Xa.shape[-2], gp.X.shape[0], len(gp.posteriors)
    fs2 = _lib.f64(ais["f_s2"])
    lnw = None if acq_fcn.acq_info.get("variational_importance_sampling") else _lib.f64(ais["ln_weights"])
    K = np.empty((S, Na, N)) if products else None
    Ct = np.empty((S, N, Na)) if products else None
    ctx.__dict__["_acq_is_key"] = None
    ctx.check(ctx._lib.vbmc_acq_is_build(ctx._h, Na, _lib.ptr(Xa), int(Xa.ndim == 3), _lib.ptr(fs2), _lib.ptr(lnw),
                                         _lib.ptr(K), _lib.ptr(Ct)))
    if products:
        ais["K_Xa_X"], ais["C_tmp"] = K, Ct
    key, parts = _is_state_key(ais, ctx)
    ctx.__dict__["_acq_is_key"], ctx.__dict__["_acq_is_ref"] = key, (ais, gp.posteriors, parts)


def active_importance_sampling(vp, gp, acq_fcn, options, *, rng=None, seed=None, sampler=None, products=True):
    """The reference's function (:10-314): a dict with ``X`` (Na, D) -- (S, Na, D) after MCMC -- ``f_s2`` (Na, S),
    ``ln_weights`` (S, Na, renormalised), ``K_Xa_X`` (S, Na, N) and ``C_tmp`` (S, N, Na).

    Keyword-only extras: ``rng`` / ``seed`` (the draw source, module docstring), ``sampler`` (the slice-sampler class
    of the MCMC steps, default ``gpyreg.slice_sample.SliceSampler``; or ``"device"``: step 2's chains as one launch,
    module docstring) and ``products`` (False: ``K_Xa_X`` / ``C_tmp`` stay on the device, for callers that evaluate
    with this package's acquisition classes)."""
    X = np.asarray(gp.X, dtype=np.float64)
    N, D = X.shape
    _check_shape(D)
    mode = _rng_mode(rng)
    S = len(gp.posteriors)
    info = acq_fcn.acq_info

    # scales and bounds of the input space, for the MCMC (:48-53)
    widths = np.std(X, axis=0, ddof=1)
    diam = np.amax(X, axis=0) - np.amin(X, axis=0)
    lb_tran = np.amin(X, axis=0) - 0.5 * diam
    ub_tran = np.amax(X, axis=0) + 0.5 * diam

    ais = {"ln_weights": None, "X": None, "f_s2": None}
    on_device = _device_sampler(sampler)
    if info.get("variational_importance_sampling", False):
        # step 0: samples of the variational posterior itself (:60-114)
        if sampler is not None and on_device and info.get("mcmc_importance_sampling"):
            raise NotImplementedError("active_importance_sampling: sampler='device' runs the chains of step 2; step 0's "
                                      "MCMC pass hands a matrix of walkers to the sampler and needs a sampler class")
        if on_device:
            sampler = None  # (the environment's switch: step 0 keeps the class route)
        Na = ceil(_eval_option(options, "active_importance_sampling_mcmc_samples", {"K": vp.K, "n_vars": D, "D": D}))
        if not np.isfinite(Na) or not np.isscalar(Na) or Na <= 0:
            raise ValueError("options['active_importance_sampling_mcmc_samples']"
                             + "should evaluate to a positive integer.")
        ctx = ctx_of(vp)  # (after the options are known to be valid: a context needs a device)
        dgp = _DeviceGP(gp, ctx)
        if mode == "philox":
            seed = _seed_or_draw(seed)
        Xa, __ = _mirror_vp(vp, ctx).sample(Na, orig_flag=False, rng=mode, seed=seed)
        f_mu, f_s2 = _predict(gp, ctx, Xa, separate_samples=True)
        if info.get("mcmc_importance_sampling"):
            if fess(vp, f_mu, Xa) < options["active_importance_sampling_fess_thresh"]:
                n_mcmc = Na * options["active_importance_sampling_mcmc_thin"]
                sampler_opts, __, __ = get_mcmc_opts(n_mcmc)
                cls = _default_sampler() if sampler is None else sampler
                chain = cls(lambda x: acq_fcn.is_log_full(x, vp=vp, gp=dgp), Xa, widths, lb_tran, ub_tran, sampler_opts)
                Xa = chain.sample(n_mcmc, 1, 0)["samples"][-Na:, :]
                f_mu, f_s2 = _predict(gp, ctx, Xa, separate_samples=True)
        ln_y = acq_fcn.is_log_base(Xa, f_mu=f_mu, f_s2=f_s2)
        ais["f_s2"], ais["ln_weights"], ais["X"] = f_s2, ln_y.T, Xa
    else:
        # step 1: importance sampling-resampling from the smoothed posterior and the boxes (:116-191)
        n_vp = options["active_importance_sampling_vp_samples"]
        n_box = options["active_importance_sampling_box_samples"]
        n_mcmc = options["active_importance_sampling_mcmc_samples"]
        if n_mcmc > 0 and on_device:
            _check_mcmc_shape(N)  # (before anything is drawn)
        w_vp = n_vp / (n_vp + n_box)
        rect_delta = 2 * np.std(X, ddof=1, axis=0)
        ctx = ctx_of(vp)
        if mode == "philox":
            seed = _seed_or_draw(seed)
        vp_is = smoothed_posterior(vp, ctx) if n_vp > 0 else None
        parts = []
        if n_vp > 0:
            Xa_vp, __ = vp_is.sample(n_vp, orig_flag=False, rng=mode, seed=seed)
            parts.append((Xa_vp,) + active_sample_proposal_pdf(Xa_vp, gp, vp_is, w_vp, rect_delta, acq_fcn))
        if n_box > 0:
            Xa_box = _box_samples(gp, ctx, int(n_box), rect_delta, mode, seed)
            parts.append((Xa_box,) + active_sample_proposal_pdf(Xa_box, gp, vp_is, w_vp, rect_delta, acq_fcn))
        ais["X"] = np.concatenate([p[0] for p in parts], axis=0)
        ais["ln_weights"] = np.concatenate([p[1].T for p in parts], axis=1)
        ais["f_s2"] = np.concatenate([p[2] for p in parts], axis=0)
        ais["ln_weights"][~np.isfinite(ais["ln_weights"])] = -np.inf

        if n_mcmc > 0 and on_device:
            # step 2 as one launch: every GP sample's chain at once (:195-262)
            thin = options["active_importance_sampling_mcmc_thin"]
            if mode != "philox":
                seed = _seed_or_draw(seed)
            ais, stats = _mcmc_device(ctx, gp, acq_fcn, ais, int(n_mcmc), thin, ceil(thin * n_mcmc / 2), widths, lb_tran,
                                      ub_tran, seed)
            ctx.__dict__["_is_mcmc_stats"] = stats  # (the last launch's counters, for measurement tools)
            if np.any(stats[:, 2:]):
                ais["mcmc_stats"] = stats
        elif n_mcmc > 0:
            # step 2: one chain per GP sample, started from a resampled proposal (:195-262)
            old = ais
            ais = {"ln_weights": np.zeros((S, n_mcmc)), "X": np.zeros((S, n_mcmc, D)), "f_s2": np.zeros((n_mcmc, S))}
            cls = _default_sampler() if sampler is None else sampler
            for s in range(S):
                gp1 = _DeviceGP(gp, ctx, sample=s)
                thin = options["active_importance_sampling_mcmc_thin"]
                burn_in = ceil(thin * n_mcmc / 2)
                sampler_opts, __, __ = get_mcmc_opts(n_mcmc)
                f_mu, f_s2 = gp1.predict(old["X"], separate_samples=True)
                ln_w = old["ln_weights"][s, :].reshape(-1, 1) + acq_fcn.is_log_added(f_mu=f_mu, f_s2=f_s2)
                ln_w_max = np.amax(ln_w, axis=1).reshape(-1, 1)
                if np.any(ln_w_max == -np.inf):
                    raise ValueError("Invalid value.")
                weights = np.exp(ln_w - ln_w_max).ravel()
                weights = weights / np.sum(weights)
                index = np.random.choice(a=len(weights), p=weights, replace=False)
                x0 = np.maximum(np.minimum(old["X"][index, :], ub_tran), lb_tran)
                chain = cls(lambda x, g=gp1: acq_fcn.is_log_full(x, vp=vp, gp=g), x0, widths, lb_tran, ub_tran,
                            sampler_opts)
                res = chain.sample(n_mcmc, thin, burn_in)
                Xa, log_p = res["samples"], res["f_vals"]
                f_mu, f_s2 = gp1.predict(Xa, separate_samples=True)
                ln_y = acq_fcn.is_log_base(Xa, f_mu=f_mu, f_s2=f_s2)
                ais["f_s2"][:, s] = f_s2.ravel()
                ais["ln_weights"][s, :] = ln_y.T - log_p.T
                ais["X"][s, :, :] = Xa

    # step 3: the cross-kernel matrices and C_tmp, on the device (:264-308); weights renormalised (:313)
    ais["ln_weights"] = renormalize_weights(ais["ln_weights"])
    _build_state(ctx, gp, acq_fcn, ais, products)
    return ais
