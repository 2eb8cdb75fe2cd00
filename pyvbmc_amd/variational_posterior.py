"""``VariationalPosterior`` -- the reference's Gaussian-mixture class, hot-path subset,
with the density evaluated on the MI355X.

Mirrors /root/reference/pyvbmc/variational_posterior/variational_posterior.py
(class at :24): same constructor, attribute names/shapes (:106-138) and the
methods on the ELBO path -- ``get_bounds`` (:140-239), ``sample`` (:241-363),
``pdf`` (:365-564), ``log_pdf`` (:566-621), ``get_parameters`` (:623-678),
``set_parameters`` (:680-759), ``moments`` (:761-808) -- with the same mutation
side effects and exceptions -- plus ``kl_div`` (:1032-1127), the Monte-Carlo consumer
SURVEY.md 8f row 4 names, and ``mtv`` (:921-1030), the marginal total variation distance, whose
density estimates, splines and integrals run on the device (csrc/kde.hip, vbmc_mtv; kde_1d itself is
``pyvbmc_amd.stats.kde_1d``), and ``mode`` (:810-919), whose start selection and local searches run on the
device for all rounds at once (csrc/mode.hip, vbmc_mixture_mode), and ``save`` / ``load`` (:1287-1343), and ``plot``
(:1129-1285) over ``marginals``, the histograms, quantiles and density levels of a corner plot in one device call
(csrc/marginals.hip, vbmc_marginals; pyvbmc_amd/marginals.py).

Where the arithmetic runs: ``pdf``/``log_pdf`` -> HIP kernel (vbmc_mixture_pdf).
State bookkeeping (get/set_parameters, bounds) and the closed-form K*D^2 moments are
plain NumPy object state, as in the reference.  ``sample`` draws from NumPy's global
stream exactly like the reference by default; ``rng="philox"`` (keyword-only, or env
``VBMC_HIP_RNG=philox``) generates the samples on the device instead
(vbmc_mixture_sample), which is what ``moments(orig_flag=True)`` and ``kl_div`` then use;
with ``rng="philox"`` ``kl_div`` runs entirely on the device (vbmc_kl_div_mc).

Original space (``orig_flag=True``, the default of ``sample`` / ``pdf`` / ``moments``): a transformer
with the reference's fields (pyvbmc_amd/transformer.py) runs on the device -- fused into the sampling,
density, moments and KL entry points (vbmc_*_orig) -- and any other transformer object is called on
the host as the reference does.  ``VBMC_HIP_TRANSFORM=0`` keeps every transformer on the host.
"""
import ctypes as C
import os
import sys
import types

import numpy as np

from . import _lib
from . import transformer as _xf
from ._duck import upload_vp
from .entropy import _HOST_RANDN_MIN, host_randn


def _randn(n, d):
    """``np.random.randn(n, d)`` -- the same values and generator state; large requests through the
    library's multi-threaded restatement of NumPy's stream (csrc/host_randn.hip)."""
    if n * d >= _HOST_RANDN_MIN:
        flat = host_randn(n * d)
        if flat is not None:
            return flat.reshape(n, d)
    return np.random.randn(n, d)


def _rng_mode(rng, check=True):
    """``rng``, or the environment's default when it is None; an unknown name raises unless ``check`` is off."""
    mode = os.environ.get("VBMC_HIP_RNG", "numpy") if rng is None else rng
    if check and mode not in ("numpy", "philox"):
        raise ValueError(f"unknown rng {mode!r}")
    return mode


def _seed_or_draw(seed):
    """``seed`` of the device generator, drawn from NumPy's global stream when it is None."""
    return int(np.random.randint(0, 2**62, dtype=np.int64)) if seed is None else seed


def _mixture_args(vp):
    """``(mu.T, sigma, lambd, w)`` of ``vp`` as contiguous float64 arrays: a second mixture of the C ABI."""
    return (_lib.f64(np.asarray(vp.mu, dtype=np.float64).reshape(vp.D, vp.K).T), _lib.f64(np.ravel(vp.sigma)),
            _lib.f64(np.ravel(vp.lambd)), _lib.f64(np.ravel(vp.w)))


def _shape_pdf(y, dy, in_dims, grad_flag):
    """``pdf``'s result from y (n x 1) and dy: a pair with the gradient, raveled for a 1-D input."""
    out = (y, dy) if grad_flag else y
    if in_dims == 1:
        return tuple(o.ravel() for o in out) if grad_flag else out.ravel()
    return out


class IdentityTransformer:
    """Unbounded-space parameter transformer (the reference's default
    ``ParameterTransformer(D)`` with infinite bounds is the identity map).  Any
    object with the same five members may be passed instead, e.g. the
    reference's own ``ParameterTransformer``."""

    def __init__(self, D):
        self.lb_orig = np.full((1, D), -np.inf)
        self.ub_orig = np.full((1, D), np.inf)

    def __call__(self, x):
        return x

    def inverse(self, u):
        return u

    def log_abs_det_jacobian(self, u):
        return np.zeros(np.atleast_2d(u).shape[0])


class VariationalPosterior:
    def __init__(self, D, K=2, x0=None, parameter_transformer=None):
        self.D = D
        self.K = K
        if x0 is None:
            x0 = np.zeros((D, K))
        elif x0.size == D:
            x0 = np.tile(x0.reshape(-1), (K, 1)).T
        else:
            x0 = x0.T
            x0 = np.tile(x0, int(np.ceil(K / x0.shape[1])))[:, :K]
        self.w = np.ones((1, K)) / K
        self.eta = np.ones((1, K)) / K
        # the reference perturbs the means and consumes the global RNG here (:121)
        self.mu = x0 + 1e-6 * np.random.randn(D, K)
        self.sigma = 1e-3 * np.ones((1, K))
        self.lambd = np.ones((D, 1))
        self.optimize_weights = True
        self.optimize_mu = True
        self.optimize_sigma = True
        self.optimize_lambd = True
        self.parameter_transformer = (
            IdentityTransformer(D) if parameter_transformer is None else parameter_transformer
        )
        self.bounds = None
        self.stats = None
        self._mode = None
        self._ctx = None

    # -- device plumbing (never pickled) -----------------------------------------
    def __getstate__(self):
        st = self.__dict__.copy()
        st["_ctx"] = None
        return st

    def save(self, file, overwrite=False):
        """Write the posterior to ``file`` (:1287-1317): ``.pkl`` is appended to a name without a suffix,
        ``FileExistsError`` for an existing file unless ``overwrite``; the write is atomic (pyvbmc_amd/_persist.py).  The
        context is not part of the file."""
        from . import _persist

        _persist.save(self, file, overwrite)

    @classmethod
    def load(cls, file):
        """The posterior ``save`` wrote (:1319-1343); it has no context until it is used or given one.  Loading a pickle
        runs code: load only files you wrote yourself."""
        from . import _persist

        vp = _persist.load(file)
        if not isinstance(vp, cls):
            raise TypeError(f"{file}: holds a {type(vp).__name__}, not a {cls.__name__}")
        return vp

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.default_context()
        return self._ctx

    @ctx.setter
    def ctx(self, value):
        self._ctx = value

    def _upload(self, ctx=None):
        """Push the current attributes to the device context (pyvbmc_amd._duck.upload_vp;
        the hot-path functions call that helper directly, so they accept any object with
        the reference's public attributes, not just this class)."""
        return upload_vp(self, self.ctx if ctx is None else ctx)

    # -- bounds (:140-239) ------------------------------------------------------------
    def get_bounds(self, X, options, K=None):
        if K is None:
            K = self.K
        D = self.D
        if self.bounds is None:
            self.bounds = {
                "mu_lb": np.full((D,), np.inf),
                "mu_ub": np.full((D,), -np.inf),
                "lnscale_lb": np.full((D,), np.inf),
                "lnscale_ub": np.full((D,), -np.inf),
            }
        xmin, xmax = np.min(X, axis=0), np.max(X, axis=0)
        b = self.bounds
        b["mu_lb"] = np.minimum(xmin, b["mu_lb"])
        b["mu_ub"] = np.maximum(xmax, b["mu_ub"])
        ln_range = np.log(xmax - xmin)
        b["lnscale_lb"] = np.minimum(b["lnscale_lb"], ln_range + np.log(options["tol_length"]))
        b["lnscale_ub"] = np.maximum(b["lnscale_ub"], ln_range)
        if self.optimize_weights:
            b["eta_lb"] = -np.inf if options["tol_weight"] == 0 else np.log(0.5 * options["tol_weight"])
            b["eta_ub"] = 0
        lo, hi = [], []
        if self.optimize_mu:
            lo.append(np.tile(b["mu_lb"], (K,)))
            hi.append(np.tile(b["mu_ub"], (K,)))
        if self.optimize_sigma or self.optimize_lambd:
            lo.append(np.tile(b["lnscale_lb"], (K,)))
            hi.append(np.tile(b["lnscale_ub"], (K,)))
        if self.optimize_weights:
            lo.append(np.tile(b["eta_lb"], (K,)))
            hi.append(np.tile(b["eta_ub"], (K,)))
        theta_bnd = {"lb": np.concatenate(lo), "ub": np.concatenate(hi)}
        theta_bnd["tol_con"] = options["tol_con_loss"]
        if self.optimize_weights:
            theta_bnd["weight_threshold"] = max(1 / (4 * K), options["tol_weight"])
            theta_bnd["weight_penalty"] = options["weight_penalty"]
        return theta_bnd

    # -- sampling (:241-363): RNG-bound, consumes np.random in the reference's order ----
    def sample(self, N, orig_flag=True, balance_flag=False, df=np.inf, *, rng=None, seed=None,
               shuffle=True):
        """Reference signature; keyword-only extras: ``rng`` ("numpy": the reference's global
        MT19937 stream, the default; "philox": the device generator), ``seed`` of the device
        generator (drawn from ``np.random`` when omitted) and ``shuffle`` (the device returns
        balanced samples grouped by component; ``True`` permutes them like the reference)."""
        if N < 1:
            return np.zeros((0, self.D)), np.zeros((0, 1))
        mode = _rng_mode(rng, check=False)
        if mode == "philox" and not (np.isfinite(df) and df < 0):  # (df < 0: numpy's gamma raises, below)
            N = int(N)
            ctx = self._upload()
            seed = _seed_or_draw(seed)
            x = np.empty((N, self.D))
            i = np.empty(N, dtype=np.int32)
            tdf = float(df) if (np.isfinite(df) and df != 0) else float("inf")
            on_dev = orig_flag and _xf.upload(self.parameter_transformer, ctx, 0, self.D) is not None
            fn = ctx._lib.vbmc_mixture_sample_orig if on_dev else ctx._lib.vbmc_mixture_sample_t
            ctx.check(fn(ctx._h, N, int(seed), int(bool(balance_flag)), tdf, _lib.ptr(x),
                         i.ctypes.data_as(C.POINTER(C.c_int32))))
            if balance_flag and shuffle and self.K > 1:
                perm = np.random.permutation(N)
                x, i = x[perm], i[perm]
            if orig_flag and not on_dev:
                x = self.parameter_transformer.inverse(x)
            return x, (i.astype(np.int64) if self.K > 1 else np.zeros(N))
        _rng_mode(mode)  # (an unknown name raises here, after the device branch)
        lam = self.lambd.reshape(1, -1)
        heavy = np.isfinite(df) and df != 0
        if self.K > 1:
            if balance_flag:
                reps = np.floor(self.w * N).astype("int")
                i = np.repeat(range(self.K), reps.ravel())
                if N > i.shape[0]:
                    w_extra = self.w * N - reps
                    n_extra = np.ceil(np.sum(w_extra))
                    w_extra += self.w * (n_extra - sum(w_extra))
                    w_extra /= np.sum(w_extra)
                    i = np.append(
                        i, np.random.choice(range(self.K), size=n_extra.astype("int"), p=w_extra.ravel())
                    )
                np.random.shuffle(i)
                i = i[:N]
            else:
                i = np.random.choice(range(self.K), size=N, p=self.w.ravel())
            if heavy:
                t = df / 2 / np.sqrt(np.random.gamma(df / 2, df / 2, (N, 1)))
                x = self.mu.T[i] + lam * _randn(N, self.D) * t * self.sigma[:, i].T
            else:
                x = self.mu.T[i] + lam * _randn(N, self.D) * self.sigma[:, i].T
        else:
            if heavy:
                t = df / 2 / np.sqrt(np.random.gamma(df / 2, df / 2, (N, 1)))
                x = self.mu.T + lam * t * _randn(N, self.D) * self.sigma
            else:
                x = self.mu.T + lam * _randn(N, self.D) * self.sigma
            i = np.zeros(N)
        if orig_flag:
            x = self._inverse(x)
        return x, i

    def _inverse(self, u):
        """The transformer's inverse of the NumPy-stream draws: on the device when it is reference-shaped and
        there is a device, else its own method.  These draws never needed a GPU, and still do not: without one
        (none visible, or a host-only context) the transformer is called on the host as before."""
        pt = self.parameter_transformer
        ctx = self._device_ctx() if _xf.candidate(pt) else None
        D = _xf.upload(pt, ctx, 0, self.D) if ctx is not None else None
        if D is None:
            return pt.inverse(u)
        return _xf.transform_points(ctx, u, _xf.INVERSE, D)

    def _device_ctx(self):
        """The context to use when it has a device, else None (creates no context on a machine without one)."""
        if self._ctx is not None:
            return self._ctx if self._ctx.device >= 0 else None
        return self.ctx if _lib.device_count() > 0 else None

    # -- density (:365-621) ---------------------------------------------------------------
    def pdf(self, x, orig_flag=True, log_flag=False, grad_flag=False, df=np.inf):
        # 0-D / 1-D inputs are lifted to 2-D and 1-D results raveled, like the
        # reference's handle_0D_1D_input decorator (decorators/handle_0D_1D_input.py:46-58)
        in_dims = np.ndim(x)
        x = np.array(np.atleast_2d(x), dtype=np.float64)  # copy (:425)
        n, D = x.shape
        finite_df = np.isfinite(df) and df != 0
        if grad_flag and finite_df:
            raise NotImplementedError("Gradient of heavy-tailed pdf not supported yet.")
        if grad_flag and orig_flag and log_flag:
            raise NotImplementedError(
                "vbmc_pdf:NoOriginalGrad: Gradient computation in original space not supported yet."
            )
        if orig_flag:
            ctx = self._upload()
            if _xf.upload(self.parameter_transformer, ctx, 0, self.D) is not None:
                return self._pdf_orig_device(ctx, x, in_dims, log_flag, grad_flag, df)
            pt = self.parameter_transformer
            mask = np.logical_and(np.all(x > pt.lb_orig, axis=1), np.all(x < pt.ub_orig, axis=1))
            x[mask] = pt(x[mask])
        else:
            mask = np.full(n, True)
        ctx = self._upload()
        y = np.empty(n)
        dy = np.empty((n, D)) if grad_flag else None
        xin = np.ascontiguousarray(x)
        if not np.all(mask) and not np.all(np.isfinite(xin)):
            # rows outside the bounds stay in original coordinates and go through the density like
            # the reference's (their value is overwritten below, their gradient rows are returned
            # as computed, :464-469); only non-finite coordinates are kept off the device
            xin = np.where(np.isfinite(xin), xin, 0.0)
        ctx.check(
            ctx._lib.vbmc_mixture_pdf(
                ctx._h, n, _lib.ptr(xin), int(bool(log_flag)), int(bool(grad_flag)), float(df),
                _lib.ptr(y), _lib.ptr(dy),
            )
        )
        y = y.reshape(n, 1)
        if log_flag:
            y[~mask] = -np.inf
        else:
            y[~mask] = 0
        if orig_flag:
            ladj = self.parameter_transformer.log_abs_det_jacobian(x[mask])[:, np.newaxis]
            if log_flag:
                y[mask] -= ladj
            else:
                y[mask] /= np.exp(ladj)
        return _shape_pdf(y, dy, in_dims, grad_flag)

    def _pdf_orig_device(self, ctx, x, in_dims, log_flag, grad_flag, df):
        """pdf(orig_flag=True) in one device call (vbmc_mixture_pdf_orig): bound mask, transform, density,
        Jacobian; the host path's values, gradient rows included."""
        n, D = x.shape
        if D != self.D:
            raise ValueError(f"points have {D} columns, the posterior D={self.D}")
        y = np.empty(n)
        dy = np.empty((n, D)) if grad_flag else None
        ctx.check(ctx._lib.vbmc_mixture_pdf_orig(ctx._h, n, _lib.ptr(x), int(bool(log_flag)), int(bool(grad_flag)),
                                                 float(df), _lib.ptr(y), _lib.ptr(dy)))
        return _shape_pdf(y.reshape(n, 1), dy, in_dims, grad_flag)

    def log_pdf(self, *args, **kwargs):
        return self.pdf(*args, **kwargs, log_flag=True)

    # -- parameter vector (:623-759) ----------------------------------------------------------
    def _renormalise(self):
        nl = np.sqrt(np.sum(self.lambd**2) / self.D)
        self.lambd = self.lambd.reshape(-1, 1) / nl
        self.sigma = self.sigma.reshape(1, -1) * nl
        if self.optimize_weights:
            self.w = self.w.reshape(1, -1) / np.sum(self.w)

    def get_parameters(self, raw_flag=True):
        self._renormalise()
        theta = self.mu.ravel(order="F") if self.optimize_mu else np.array([])
        tail = [np.array([])]
        if self.optimize_sigma:
            tail.append(self.sigma.ravel())
        if self.optimize_lambd:
            tail.append(self.lambd.ravel())
        if self.optimize_weights:
            tail.append(self.w.ravel())
        tail = np.concatenate(tail)
        return np.concatenate((theta, np.log(tail) if raw_flag else tail))

    def set_parameters(self, theta, raw_flag=True):
        theta = np.array(theta, dtype=np.float64)
        D, K = self.D, self.K
        if not raw_flag:
            n_con = K * self.optimize_weights + D * self.optimize_lambd + K * self.optimize_sigma
            # same slice the reference checks (theta[-check_idx:] with check_idx = -n_con, :701-710)
            if np.any(theta[n_con:] < 0.0):
                raise ValueError("sigma, lambda and weights must be positive when raw_flag = False")
        pos = 0
        if self.optimize_mu:
            self.mu = np.reshape(theta[: D * K], (D, K), order="F")
            pos = D * K
        if self.optimize_sigma:
            s = theta[pos : pos + K]
            self.sigma = np.exp(s) if raw_flag else s
            pos += K
        if self.optimize_lambd:
            l = theta[pos : pos + D]
            self.lambd = np.exp(l) if raw_flag else l
        if self.optimize_weights:
            eta = theta[-K:]
            self.w = (np.exp(eta - np.amax(eta)) if raw_flag else eta)[np.newaxis, :]
        self._renormalise()
        self._mode = None

    # -- moments (:761-808) ----------------------------------------------------------------------
    def moments(self, N=int(1e6), orig_flag=True, cov_flag=False, *, rng=None, seed=None):
        mode = _rng_mode(rng, check=False)
        ctx = self._upload() if orig_flag and mode == "philox" else None
        if ctx is not None and _xf.upload(self.parameter_transformer, ctx, 0, self.D) is not None:
            # the balanced samples of sample(N, True, True, rng="philox", seed=seed), reduced where they are drawn
            N = int(N)
            seed = _seed_or_draw(seed)
            mubar = np.empty(self.D)
            cov = np.empty((self.D, self.D)) if cov_flag else None
            ctx.check(ctx._lib.vbmc_mixture_moments_orig(ctx._h, N, int(seed), int(bool(cov_flag)), _lib.ptr(mubar),
                                                         _lib.ptr(cov)))
            if cov_flag:
                cov = cov.squeeze()  # (np.cov's shape)
        elif orig_flag:
            # mean / covariance do not depend on the order: skip the shuffle on the device path
            x, _ = self.sample(int(N), orig_flag=True, balance_flag=True, rng=rng, seed=seed, shuffle=False)
            mubar = np.mean(x, axis=0)
            if cov_flag:
                cov = np.cov(x.T)
        else:
            mubar = np.sum(self.w * self.mu, axis=1)
            if cov_flag:
                cov = np.sum(self.w * self.sigma**2) * np.eye(len(self.lambd)) * self.lambd**2
                dev = self.mu - mubar[:, np.newaxis]
                cov = cov + (self.w * dev) @ dev.T
        return (mubar.reshape(1, -1), cov) if cov_flag else mubar.reshape(1, -1)

    # -- mode (:810-919) -------------------------------------------------------------------------
    def mode(self, orig_flag=True, n_opts=None, *, rng=None, seed=None):
        """The mode of the posterior, a ``(D,)`` array; reference signature.  ``n_opts`` rounds (default
        ``ceil(sqrt(K))``) each pick the best of 1e5 samples (plus the component centres in round 0) and run a
        local search from it; all rounds run in one device call (vbmc_mixture_mode, csrc/mode.hip).
        ``rng="numpy"`` (the default) draws ``self.sample(int(1e5), orig_flag)`` once per round from NumPy's
        global stream, as the reference does; ``rng="philox"`` draws round k on the device with ``seed + k``
        and never copies the candidates to the host.  The result for ``orig_flag=True`` is cached in
        ``_mode`` until ``set_parameters``.  ``mode_info`` keeps the last search's details: ``log_pdf`` at the
        result, per-round ``records`` (start index, start value, final value, iterations, status), the rounds'
        final ``points`` (and, from the device, ``search_points``, the same in the search's coordinates) and
        whether it ran on the ``device``.  With ``rng="numpy"`` the n_opts x 1e5 x D candidates are held and
        uploaded in one piece.

        Deviations from the reference: D = 1 with ``orig_flag=True`` returns the mode (the reference raises
        ``AxisError``), and the local search is a monotone ascent with analytic derivatives that stops at a
        step of 1e-12, so the result is a stationary point to a much tighter tolerance than SciPy's.  Without
        a device (or with a transformer that cannot go to one and ``orig_flag=True``) a NumPy / SciPy loop
        with the reference's structure runs around ``sample`` / ``pdf``."""
        mode = _rng_mode(rng)
        if n_opts is None:
            n_opts = int(np.ceil(np.sqrt(self.K)))
        n_opts = int(n_opts)
        if n_opts < 1:
            raise ValueError(f"n_opts={n_opts}: at least one optimization run is needed")
        if orig_flag and self._mode is not None:
            return self._mode
        x, self.mode_info = self._mode_search(bool(orig_flag), n_opts, mode, seed)
        if orig_flag:
            self._mode = x
        return x

    def _mode_search(self, orig_flag, n_opts, mode, seed):
        D, n = self.D, int(1e5)
        if D > 32:
            raise _lib.UnsupportedShape(f"mode: D={D} > 32 not supported")
        ctx = self._device_ctx()
        on_dev = ctx is not None
        if on_dev and orig_flag:
            pt = _device_pt(self)
            on_dev = _xf.upload(pt, self._upload(ctx), 0, D) is not None and _orthogonal(pt.R_mat)
        if not on_dev:
            return self._mode_host(orig_flag, n_opts, mode, seed, n)
        cand = None
        if mode == "numpy":
            cand = np.empty((n_opts, n, D))
            for k in range(n_opts):
                cand[k] = self.sample(n, orig_flag, rng="numpy")[0]
        else:
            seed = _seed_or_draw(seed)
        ctx = self._upload(ctx)
        if orig_flag:  # (sample may have put another transformer in the slot)
            _xf.upload(_device_pt(self), ctx, 0, D)
        x, f = np.empty(D), np.empty(1)
        rec, pts, ys = np.empty((n_opts, 5)), np.empty((n_opts, D)), np.empty((n_opts, D))
        ctx.check(ctx._lib.vbmc_mixture_mode(ctx._h, n_opts, int(orig_flag), n, _lib.ptr(cand), int(seed or 0), 200,
                                             1e-12, _lib.ptr(x), _lib.ptr(f), _lib.ptr(rec), _lib.ptr(pts), _lib.ptr(ys)))
        return x, {"log_pdf": float(f[0]), "records": rec, "points": pts, "search_points": ys, "device": True}

    def _log_pdf_host(self, x, orig_flag):
        """``pdf(x, orig_flag, log_flag=True)`` and, in the transformed space, its gradient, in NumPy (a 1-D
        point gives a scalar and a ``(D,)`` gradient)."""
        dims = np.ndim(x)
        x = np.array(np.atleast_2d(x), dtype=np.float64)
        pt, lj = self.parameter_transformer, 0.0
        mask = np.full(x.shape[0], True)
        if orig_flag:
            mask = np.all(x > pt.lb_orig, axis=1) & np.all(x < pt.ub_orig, axis=1)
            u = np.atleast_2d(pt(x[mask]))
            lj = np.ravel(pt.log_abs_det_jacobian(u))
        else:
            u = x
        lam, sig = self.lambd.reshape(1, 1, -1), np.ravel(self.sigma)
        z = (u[:, None, :] - self.mu.T[None, :, :]) / lam                         # n x K x D
        l = (np.log(np.ravel(self.w)) - self.D * np.log(sig) - 0.5 * self.D * np.log(2 * np.pi)
             - np.sum(np.log(lam)) - 0.5 * np.sum(z**2, axis=2) / sig**2)
        m = np.max(l, axis=1, keepdims=True)
        p = np.exp(l - m)
        y = np.full(x.shape[0], -np.inf)
        y[mask] = m[:, 0] + np.log(np.sum(p, axis=1)) - lj
        dy = None
        if not orig_flag:
            r = p / np.sum(p, axis=1, keepdims=True)
            dy = -np.sum((r / sig**2)[:, :, None] * z, axis=1) / lam[0]
        if dims == 1:
            return y[0], (None if dy is None else dy[0])
        return y, dy

    def _mode_host(self, orig_flag, n_opts, mode, seed, n):
        """The reference's loop (:863-914) around our own ``sample`` and a NumPy log-density: no device, or a
        transformer that stays on the host."""
        from scipy.optimize import minimize

        pt = self.parameter_transformer

        def neg_log_pdf(x0):
            y, dy = self._log_pdf_host(x0, orig_flag)
            return -y if orig_flag else (-y, -dy)

        rec, pts = np.empty((n_opts, 5)), np.empty((n_opts, self.D))
        for k in range(n_opts):
            x0_mat, _ = self.sample(n, orig_flag, rng=mode, seed=None if seed is None else seed + k)
            if k == 0:
                x0_mu = self.mu.T
                if orig_flag:
                    x0_mu = pt.inverse(x0_mu)
                x0_mat = np.concatenate([x0_mat, x0_mu])
            y0 = -self._log_pdf_host(x0_mat, orig_flag)[0]
            y0 = np.where(np.isnan(y0), np.inf, y0)  # a NaN value never wins (csrc/mode.hip)
            idx = int(np.argmin(y0))
            x0, bounds = x0_mat[idx], None
            if orig_flag:
                lb = np.broadcast_to(np.ravel(pt.lb_orig), (self.D,))  # (D = 1: the reference's np.stack raises)
                ub = np.broadcast_to(np.ravel(pt.ub_orig), (self.D,))
                bounds = np.stack((lb + np.sqrt(np.finfo(float).eps), ub - np.sqrt(np.finfo(float).eps)), axis=1)
                x0 = np.minimum(ub, np.maximum(x0, lb))
            res = minimize(fun=neg_log_pdf, x0=x0, bounds=bounds, jac=not orig_flag)
            pts[k] = res.x
            rec[k] = (idx, -y0[idx], -float(np.ravel(res.fun)[0]), res.nit, 0 if res.success else 2)
        best = int(np.argmin(np.where(np.isnan(rec[:, 2]), np.inf, -rec[:, 2])))
        return pts[best].copy(), {"log_pdf": rec[best, 2], "records": rec, "points": pts, "device": False}

    # -- Kullback-Leibler divergence (:1032-1127) ------------------------------------------------
    def kl_div(self, vp2=None, samples=None, N=int(1e5), gauss_flag=False, *, rng=None, seed=None):
        """Forward and reverse KL divergence between two posteriors, reference signature.
        With ``rng="philox"`` (or ``VBMC_HIP_RNG=philox``) and both posteriors sharing one
        parameter transformer the Monte-Carlo branch runs in one device call."""
        if samples is None and vp2 is None:
            raise ValueError("Either vp2 or samples have to be not None")
        if not gauss_flag and vp2 is None:
            raise ValueError("Unless the KL divergence is gaussianized, VP2 is required.")
        mode = _rng_mode(rng, check=False)
        if gauss_flag:
            if N == 0:
                raise ValueError("Analytical moments are available only for the transformed space.")
            q1mu, q1sigma = self.moments(N, True, True, rng=rng, seed=seed)
            if vp2 is not None:
                q2mu, q2sigma = vp2.moments(N, True, True, rng=rng, seed=None if seed is None else seed + 1)
            else:
                q2mu = np.mean(samples)  # sic (:1103)
                q2sigma = np.cov(samples.T)
            kls = kl_div_mvn(q1mu, q1sigma, q2mu, q2sigma)
        elif mode == "philox" and (fn := self._kl_device_fn(vp2)) is not None:
            ctx = self.ctx
            seed = _seed_or_draw(seed)
            mu2, sg2, lm2, w2 = _mixture_args(vp2)
            kls = np.empty(2)
            ctx.check(fn(ctx._h, int(N), int(seed), vp2.K, _lib.ptr(mu2), _lib.ptr(sg2), _lib.ptr(lm2), _lib.ptr(w2),
                         _lib.ptr(kls)))
        else:
            minp = sys.float_info.min
            xx1, _ = self.sample(N, True, True, rng=rng, seed=seed, shuffle=False)
            q1 = self.pdf(xx1, True)
            q2 = vp2.pdf(xx1, True)
            # the reference writes `q == 0 | np.isinf(q)`, which Python parses as
            # q == (0 | isinf(q)): true exactly where q == 0 (:1113-1114)
            q1[q1 == 0] = 1.0
            q2[q2 == 0] = minp
            kl1 = -np.mean(np.log(q2) - np.log(q1))
            xx2, _ = vp2.sample(N, True, True, rng=rng, seed=None if seed is None else seed + 1, shuffle=False)
            q1 = self.pdf(xx2, True)
            q2 = vp2.pdf(xx2, True)
            q1[q1 == 0] = minp
            q2[q2 == 0] = 1.0
            kl2 = -np.mean(np.log(q1) - np.log(q2))
            kls = np.concatenate((kl1, kl2), axis=None)
        return np.maximum(0, kls)  # correct for numerical errors (:1126)

    def _kl_device_fn(self, vp2):
        """The C function that runs kl_div's Monte-Carlo branch against ``vp2`` in one device call, with this
        mixture uploaded and the transformers it needs in their slots; None when there is none."""
        if _same_transformer(self, vp2) and vp2.D == self.D:
            return self._upload()._lib.vbmc_kl_div_mc
        if (vp2.D == self.D and _xf.upload(self.parameter_transformer, self._upload(), 0, self.D) is not None
                and _xf.upload(vp2.parameter_transformer, self.ctx, 1, vp2.D) is not None):
            # different transformers: both sides in original space (vbmc_kl_div_mc_orig)
            return self.ctx._lib.vbmc_kl_div_mc_orig
        return None

    # -- marginal total variation (:921-1030) ----------------------------------------------------------
    def mtv(self, vp2=None, samples=None, N=int(1e5), *, rng=None, seed=None):
        """Marginal total variation distances to ``vp2`` or to ``samples``, a ``(1, D)`` array; reference
        signature.  ``rng="numpy"`` (the default) draws ``self.sample(N, True, True)`` then
        ``vp2.sample(N, True, True)`` from NumPy's global stream, as the reference does, and uploads them
        once; ``rng="philox"`` draws both on the device (seeds ``seed`` and ``seed + 1``) and never copies
        them to the host.  Everything after the sampling is one device call (vbmc_mtv)."""
        if vp2 is None and samples is None:
            raise ValueError("Either vp2 or samples have to be not None")
        mode = _rng_mode(rng)
        D, N = self.D, int(N)
        if vp2 is not None and vp2.D != D:
            raise ValueError(f"vp2 has D={vp2.D}, this posterior D={D}")
        if samples is not None and vp2 is None:
            samples = np.ascontiguousarray(samples, dtype=np.float64)
            if samples.ndim != 2 or samples.shape[1] != D:
                raise ValueError(f"samples of shape {samples.shape}, the posterior D={D}")
        ctx = self._upload()
        if mode == "philox":
            seed = _seed_or_draw(seed)
        held = []  # arrays the sides point at, alive until the call returns

        def bounds(pt):
            lb = _lib.f64(np.broadcast_to(np.asarray(pt.lb_orig, dtype=np.float64).reshape(-1), (D,)))
            ub = _lib.f64(np.broadcast_to(np.asarray(pt.ub_orig, dtype=np.float64).reshape(-1), (D,)))
            held.extend((lb, ub))
            return lb, ub

        def host_side(x, lb, ub):
            x = _lib.f64(x)
            held.extend((x, lb, ub))
            return _lib.MtvSide(_lib.MTV_HOST, x.shape[0], _lib.ptr(x), 0, _lib.ptr(lb), _lib.ptr(ub))

        def draw_side(vp, slot, s):
            # sample(N, True, True, rng=mode, seed=s): on the device when its transformer can go to the slot
            lb, ub = bounds(vp.parameter_transformer)
            if mode == "philox" and _xf.upload(_device_pt(vp), ctx, slot, D) is not None:
                src = _lib.MTV_MIX1 if slot == 0 else _lib.MTV_MIX2
                return _lib.MtvSide(src, N, None, int(s), _lib.ptr(lb), _lib.ptr(ub))
            x, _ = vp.sample(N, True, True, rng=mode, seed=s, shuffle=False)
            return host_side(x, lb, ub)

        s1 = draw_side(self, 0, seed)
        if vp2 is not None:
            s2 = draw_side(vp2, 1, None if seed is None else seed + 1)
        else:
            s2 = host_side(samples, np.full(D, -np.inf), np.full(D, np.inf))  # (:974-975)
        if s1.source == _lib.MTV_MIX1:
            # (vp2.sample on the host path may have put vp2's mixture or transformer in this context)
            ctx = self._upload()
            _xf.upload(_device_pt(self), ctx, 0, D)
        K2, mix2 = 0, (None,) * 4
        if s2.source == _lib.MTV_MIX2:
            K2, mix2 = vp2.K, _mixture_args(vp2)
        out = np.empty(D)
        info = np.empty((2 * D, 2), dtype=np.int64)
        from .stats import _call_checked, _raise_degenerate
        rc = ctx._lib.vbmc_mtv(ctx._h, D, C.byref(s1), C.byref(s2), K2, *(_lib.ptr(a) for a in mix2), _lib.ptr(out),
                               info.ctypes.data_as(C.POINTER(C.c_int64)))
        _call_checked(ctx, rc, "mtv")
        if np.any(info[:, 1] & _lib.KDE_DEGENERATE):
            _raise_degenerate("mtv")
        return out.reshape(1, D)

    # -- marginals and the corner plot (:1129-1285) ----------------------------------------------------
    def marginals(self, N=int(1e6), bins=40, ranges=None, quantiles=(0.025, 0.16, 0.5, 0.84, 0.975), levels=(0.5, 0.9),
                  orig_flag=True, samples=None, kde=True, *, rng=None, seed=None, device=True, ctx=None):
        """The numbers of a corner plot as a ``Marginals`` object: the 1-D and pair histograms of ``N`` draws (or of
        ``samples``), the quantiles per dimension, the highest-density levels per pair and the kde_1d curve per
        dimension -- one device call (vbmc_marginals); ``device=False``: the same in NumPy.  The rules are stated in
        pyvbmc_amd/marginals.py."""
        from . import marginals as _mg

        return _mg.marginals(self, N, bins, ranges, quantiles, levels, orig_flag, samples, kde, rng=rng, seed=seed,
                             device=device, ctx=ctx)

    def plot(self, n_samples=int(1e5), title=None, plot_data=False, highlight_data=None, plot_vp_centres=False,
             plot_style=None, gp=None):
        """Reference signature: the corner plot of ``marginals(N=n_samples)`` drawn with matplotlib (imported here;
        ``ImportError`` without it, before any sampling).  Returns the figure."""
        from . import marginals as _mg

        return _mg.plot(self, n_samples, title, plot_data, highlight_data, plot_vp_centres, plot_style, gp)


_IDENTITY_PT = {}


def _device_pt(vp):
    """The transformer to put in a device slot: its own when reference-shaped, the identity's fields for
    ``IdentityTransformer`` (one object per D, so the slot's cached arguments are reused), else itself
    (not recognised: the caller samples through ``sample``)."""
    pt = vp.parameter_transformer
    if isinstance(pt, IdentityTransformer):
        D = vp.D
        if D not in _IDENTITY_PT:
            _IDENTITY_PT[D] = types.SimpleNamespace(type=np.zeros(D), lb_orig=np.full(D, -np.inf),
                                                    ub_orig=np.full(D, np.inf), mu=np.zeros(D), delta=np.ones(D),
                                                    R_mat=None, scale=None)
        return _IDENTITY_PT[D]
    return pt


def _orthogonal(R):
    """The mode search's original-space objective takes log|J| at the pre-rotation coordinates, which is what the
    transformer computes when R R^T = I (csrc/mode.hip)."""
    if R is None:
        return True
    R = np.asarray(R, dtype=np.float64)
    return R.ndim == 2 and bool(np.max(np.abs(R @ R.T - np.eye(R.shape[0]))) <= 1e-10)


def _same_transformer(a, b):
    ta, tb = a.parameter_transformer, b.parameter_transformer
    return (ta is tb or (isinstance(ta, IdentityTransformer) and isinstance(tb, IdentityTransformer))
            or (_xf.enabled() and _xf.same_by_value(ta, tb)))


def kl_div_mvn(mu1, sigma1, mu2, sigma2):
    """Analytical KL divergences between two multivariate normals, both directions
    (reference pyvbmc/stats/kl_div_mvn.py:10-47)."""
    D = mu1.size
    dmu = mu2.reshape(-1, 1) - mu1.reshape(-1, 1)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)  # (D = 1: np.cov's 0-D variance, lifted as there)
    det1, det2 = np.linalg.det(sigma1), np.linalg.det(sigma2)
    if det1 == 0 or det2 == 0:
        return np.array([np.inf, np.inf])
    lndet = np.log(det2 / det1)
    out = []
    for S_to, S_from, sign in ((sigma2, sigma1, 1.0), (sigma1, sigma2, -1.0)):
        a = np.linalg.lstsq(S_to, S_from, rcond=None)[0]
        b = np.linalg.lstsq(S_to, dmu, rcond=None)[0]
        out.append(0.5 * (np.trace(a) + dmu.T @ b - D + sign * lndet))
    return np.concatenate(out, axis=None)
