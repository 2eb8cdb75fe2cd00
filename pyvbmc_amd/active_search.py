"""The acquisition search of the reference's ``active_sample``: mirror of
``pyvbmc/vbmc/active_sample.py`` ``_get_search_points`` (:647-837) and of the search lines of ``active_sample`` itself
(:310-349).  Line numbers below cite that file.

``get_search_points`` draws the candidate set.  Two draw modes, chosen like everywhere in this package
(``variational_posterior._rng_mode``: the ``rng`` keyword, else ``VBMC_HIP_RNG``, else "numpy"):

``rng="numpy"``
    Every draw is the reference's own statement on NumPy's global stream, in the reference's order: after the same
    ``np.random.seed`` the result equals the reference's.  With ``device=False`` nothing touches a GPU; ``device=True``
    only moves the transform of the cache rows to the device where the transformer is reference-shaped.

``rng="philox"``
    Everything that scales with ``number_of_points`` is drawn on the device (``vbmc_search_fill``, csrc/api_search.hip).
    The host keeps the small statistics: the cache permutation and the four random HPD fractions from
    ``np.random.default_rng(seed)``, the HPD sets by ``get_hpd``'s rule (stats/get_hpd.py:34-37), the analytic moments of
    the posterior (``vp.moments(orig_flag=False, cov_flag=True)``), and each covariance factored the way
    ``np.random.multivariate_normal`` factors it (SVD, ``sqrt(s)[:, None] * v``), singular values at the SVD's rounding
    level set to zero first (``mvn_factor``): a rank-deficient covariance's draws then stay in its span.  Source j of ``SOURCES`` draws under
    the sub-seed ``sub_seed(seed, j)``; row n of a source depends only on (sub-seed, n).  The two mixture sources are
    the device sampler's balanced, unshuffled draws (``vbmc_mixture_sample_t``); the Gaussian and box sources take
    Philox stream 7 (csrc/sample.hip).

``search`` is the whole stage as one fused route: the points are generated (or, with ``rng="numpy"``, uploaded once),
rounded, scored, masked and ranked on the device (``vbmc_search_eval``) and come back once, with the values and the
order.  It works for the four closed-form acquisition classes and for ``AcqFcnVIQR`` / ``AcqFcnIMIQR``.
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np

from . import _lib
from . import transformer as _xf
from ._duck import ctx_of, upload_vp
from .acquisition import ACQ_LOG, ACQ_NOISY, ACQ_STD, AbstractAcqFcn, _QuantileAcq, string_to_acq
from .active_importance_sampling import active_importance_sampling
from .gp import upload_gp
from .variational_posterior import IdentityTransformer, VariationalPosterior, _rng_mode, _seed_or_draw

# the random sources in the order of the output (:724-830); their index is j of sub_seed
SOURCES = ("heavy", "mvn", "hpd0", "hpd1", "hpd2", "hpd3", "hpd4", "hpd5", "box", "vp")
_GOLDEN = 0x9E3779B97F4A7C15


def sub_seed(seed, j):
    """The key of source ``SOURCES[j]``: ``seed + (j + 1) * 0x9E3779B97F4A7C15`` modulo 2^64."""
    return (int(seed) + (j + 1) * _GOLDEN) % 2**64


def mvn_factor(cov):
    """``A`` with ``np.random.multivariate_normal(mean, cov) = z @ A + mean`` (numpy/random/mtrand.pyx: SVD of the
    covariance, ``sqrt(s)[:, None] * v``).  Singular values at the level of the SVD's own rounding -- below
    ``s.max() * D * eps``, the tolerance of ``np.linalg.matrix_rank`` -- count as zero: their square roots, ~1e-8 of the
    largest scale, would put every draw of a rank-deficient HPD set that far outside the set's span."""
    cov = np.atleast_2d(np.asarray(cov, dtype=np.float64))
    _, s, v = np.linalg.svd(cov)
    s = np.where(s > s.max() * len(s) * np.finfo(np.float64).eps, s, 0.0)
    return np.sqrt(s)[:, None] * v


def _sample_kw(vp):
    """The reference's own posterior (under the drop-in) has no ``rng`` keyword and draws from NumPy's stream anyway."""
    return {"rng": "numpy"} if isinstance(vp, VariationalPosterior) else {}


def _moments_tran(vp):
    """``vp.moments(orig_flag=False, cov_flag=True)`` (:735) in the reference's own order of operations
    (variational_posterior.py:793-804), from the public attributes: the covariance's last bits decide the last bits of
    every draw made with its factor."""
    D, K = int(vp.D), int(vp.K)
    mu = np.asarray(vp.mu, dtype=np.float64).reshape(D, K)
    w, sigma = np.reshape(vp.w, (1, K)), np.reshape(vp.sigma, (1, K))
    lambd = np.reshape(vp.lambd, (D, 1))
    mubar = np.sum(w * mu, axis=1)
    cov = np.sum(w * sigma**2) * np.eye(len(lambd)) * lambd**2
    for k in range(K):
        cov += w[:, k] * ((mu[:, k] - mubar)[:, np.newaxis]).dot((mu[:, k] - mubar)[:, np.newaxis].T)
    return mubar.reshape(1, -1), cov


def _hpd_plan(options, N_hpd, uniform4):
    """(:743-756) the six sorted fractions and the rows each gets."""
    hpd_min = options.get("hpd_frac") / 8
    hpd_max = options.get("hpd_frac")
    hpd_fracs = np.sort(np.concatenate((uniform4 * (hpd_max - hpd_min) + hpd_min, np.array([hpd_min, hpd_max]))))
    N_hpd_vec = np.diff(np.round(np.linspace(0, N_hpd, len(hpd_fracs) + 1)))
    return hpd_fracs, N_hpd_vec


def _hpd_moments(X, y, frac, D):
    """(:765-780) mean and covariance of the HPD set of ``frac`` (get_hpd.py:34-37), or the fallback when it is empty."""
    order = np.argsort(y, axis=None)[::-1]
    X_hpd = X[order[0:round(frac * X.shape[0])]]
    if X_hpd.size == 0:
        mubar = X[np.argmax(y)]  # :768-769
        sigmabar = np.cov(X, rowvar=False)  # :771
    else:
        mubar = np.mean(X_hpd, axis=0)  # :773
        sigmabar = np.cov(X_hpd, bias=True, rowvar=False)  # :776
    if sigmabar.shape != (D, D):  # :779-780
        sigmabar = np.ones((D, D)) * sigmabar
    return mubar, sigmabar


def _box(optim_state, X, lb_search, ub_search):
    """(:789-804) the box of the box source."""
    X_diam = np.amax(X, axis=0) - np.amin(X, axis=0)
    plb_tran = optim_state.get("plb_tran")
    pub_tran = optim_state.get("pub_tran")
    if np.all(np.isfinite(lb_search)) and np.all(np.isfinite(ub_search)):
        box_lb = lb_search
        box_ub = ub_search
    else:
        box_lb = plb_tran - 3 * (pub_tran - plb_tran)
        box_ub = pub_tran + 3 * (pub_tran - plb_tran)
    box_lb = np.maximum(np.amin(X, axis=0) - 0.5 * X_diam, box_lb)
    box_ub = np.minimum(np.amax(X, axis=0) + 0.5 * X_diam, box_ub)
    return box_lb, box_ub


def _too_many(N_random_points, n):
    return ValueError("A maximum of {} points ".format(N_random_points),
                      "should be randomly sampled but {} ".format(n),
                      "were sampled. Please validate the provided options.")  # :815-821


def _points_numpy(number_of_points, optim_state, function_logger, vp, options, transform):
    """``_get_search_points`` statement by statement on NumPy's global stream."""
    x0 = np.copy(optim_state["cache"]["x_orig"])  # :686
    lb_search = optim_state.get("lb_search")
    ub_search = optim_state.get("ub_search")
    D = ub_search.shape[1]  # :691
    search_X = np.full((0, D), np.nan)
    idx_cache = np.array([])
    if x0.size > 0:  # :697-706
        N_cache = math.ceil(number_of_points * options.get("cache_frac"))
        idx_cache = np.random.permutation(x0.shape[0])[: min(N_cache, x0.shape[0])]
        search_X = transform(x0[idx_cache])
    if x0.shape[0] < number_of_points:  # :709
        N_random_points = number_of_points - x0.shape[0]  # :710: the cache's size, not the rows taken from it
        random_Xs = np.full((0, D), np.nan)
        N_search_cache = round(options.get("search_cache_frac") * N_random_points)
        if N_search_cache > 0:  # :716-722
            search_cache = optim_state.get("search_cache")
            random_Xs = np.append(random_Xs, search_cache[: min(len(search_cache), N_search_cache)], axis=0)
        N_heavy = round(options.get("heavy_tail_search_frac") * N_random_points)
        if N_heavy > 0:  # :727-731
            heavy_Xs, _ = vp.sample(N=N_heavy, orig_flag=False, balance_flag=True, df=3, **_sample_kw(vp))
            random_Xs = np.append(random_Xs, heavy_Xs, axis=0)
        N_mvn = round(options.get("mvn_search_frac") * N_random_points)
        if N_mvn > 0:  # :734-739
            mubar, sigmabar = _moments_tran(vp)
            mvn_Xs = np.random.multivariate_normal(np.ravel(mubar), sigmabar, size=N_mvn)
            random_Xs = np.append(random_Xs, mvn_Xs, axis=0)
        N_hpd = round(options.get("hpd_search_frac") * N_random_points)
        if N_hpd > 0:  # :742-785
            hpd_fracs, N_hpd_vec = _hpd_plan(options, N_hpd, np.random.uniform(size=4))
            X = function_logger.X[function_logger.X_flag]
            y = function_logger.y[function_logger.X_flag]
            for idx in range(len(hpd_fracs)):
                if N_hpd_vec[idx] == 0:
                    continue
                mubar, sigmabar = _hpd_moments(X, y, hpd_fracs[idx], D)
                hpd_Xs = np.random.multivariate_normal(mubar, sigmabar, size=int(N_hpd_vec[idx]))
                random_Xs = np.append(random_Xs, hpd_Xs, axis=0)
        N_box = round(options.get("box_search_frac") * N_random_points)
        if N_box > 0:  # :788-811
            X = function_logger.X[function_logger.X_flag]
            box_lb, box_ub = _box(optim_state, X, lb_search, ub_search)
            box_Xs = np.random.standard_normal((N_box, D)) * (box_ub - box_lb) + box_lb  # :806-809: normal, not uniform
            random_Xs = np.append(random_Xs, box_Xs, axis=0)
        if N_random_points < random_Xs.shape[0]:  # :814
            raise _too_many(N_random_points, random_Xs.shape[0])
        N_vp = max(0, N_random_points - N_search_cache - N_heavy - N_mvn - N_box - N_hpd)  # :824-827
        if N_vp > 0:
            vp_Xs, _ = vp.sample(N=N_vp, orig_flag=False, balance_flag=True, **_sample_kw(vp))
            random_Xs = np.append(random_Xs, vp_Xs, axis=0)
        search_X = np.append(search_X, random_Xs, axis=0)
        idx_cache = np.append(idx_cache, np.full(N_random_points, np.nan))  # :833
    search_X = np.minimum((np.maximum(search_X, lb_search)), ub_search)  # :836
    return search_X, idx_cache


def philox_plan(number_of_points, optim_state, function_logger, vp, options, seed):
    """The philox mode's host part: ``(sources, idx_cache)`` with ``sources`` a list of ``(kind, rows, data, df, key)``
    in output order -- kind one of ``_lib.SRC_*``; data the rows (copy / transform), ``(mean, A)`` (affine), ``(lb, ub)``
    (box) or None (mixture).  Raises the reference's ``ValueError`` before anything is drawn on the device."""
    g = np.random.default_rng(seed)
    x0 = np.copy(optim_state["cache"]["x_orig"])
    lb_search = optim_state.get("lb_search")
    ub_search = optim_state.get("ub_search")
    D = ub_search.shape[1]
    sources = []
    idx_cache = np.array([])
    if x0.size > 0:  # :697-706
        N_cache = math.ceil(number_of_points * options.get("cache_frac"))
        idx_cache = g.permutation(x0.shape[0])[: min(N_cache, x0.shape[0])]
        sources.append((_lib.SRC_TRANSFORM, len(idx_cache), x0[idx_cache].reshape(-1, D), 0.0, 0))
    if x0.shape[0] < number_of_points:
        N_random_points = number_of_points - x0.shape[0]  # :710
        n_random = 0
        N_search_cache = round(options.get("search_cache_frac") * N_random_points)
        if N_search_cache > 0:  # :716-722
            search_cache = np.asarray(optim_state.get("search_cache"), dtype=np.float64)
            rows = search_cache[: min(len(search_cache), N_search_cache)].reshape(-1, D)
            sources.append((_lib.SRC_COPY, rows.shape[0], rows, 0.0, 0))
            n_random += rows.shape[0]
        N_heavy = round(options.get("heavy_tail_search_frac") * N_random_points)
        if N_heavy > 0:  # :727-731
            sources.append((_lib.SRC_MIXTURE, N_heavy, None, 3.0, sub_seed(seed, 0)))
        N_mvn = round(options.get("mvn_search_frac") * N_random_points)
        if N_mvn > 0:  # :734-739
            mubar, sigmabar = _moments_tran(vp)
            sources.append((_lib.SRC_AFFINE, N_mvn, (np.ravel(mubar), mvn_factor(sigmabar)), 0.0, sub_seed(seed, 1)))
        N_hpd = round(options.get("hpd_search_frac") * N_random_points)
        if N_hpd > 0:  # :742-785
            hpd_fracs, N_hpd_vec = _hpd_plan(options, N_hpd, g.uniform(size=4))
            X = function_logger.X[function_logger.X_flag]
            y = function_logger.y[function_logger.X_flag]
            for idx in range(len(hpd_fracs)):
                if N_hpd_vec[idx] == 0:
                    continue
                mubar, sigmabar = _hpd_moments(X, y, hpd_fracs[idx], D)
                sources.append((_lib.SRC_AFFINE, int(N_hpd_vec[idx]), (np.ravel(mubar), mvn_factor(sigmabar)), 0.0,
                                sub_seed(seed, 2 + idx)))
        N_box = round(options.get("box_search_frac") * N_random_points)
        if N_box > 0:  # :788-811
            X = function_logger.X[function_logger.X_flag]
            box_lb, box_ub = _box(optim_state, X, lb_search, ub_search)
            sources.append((_lib.SRC_BOX, N_box, (np.ravel(box_lb), np.ravel(box_ub)), 0.0, sub_seed(seed, 8)))
        n_random += N_heavy + N_mvn + N_hpd + N_box
        if N_random_points < n_random:  # :814
            raise _too_many(N_random_points, n_random)
        N_vp = max(0, N_random_points - N_search_cache - N_heavy - N_mvn - N_box - N_hpd)  # :824-827
        if N_vp > 0:
            sources.append((_lib.SRC_MIXTURE, N_vp, None, np.inf, sub_seed(seed, 9)))
        idx_cache = np.append(idx_cache, np.full(N_random_points, np.nan))  # :833
    return sources, idx_cache


def _check_D(D):
    if D > 32:
        raise _lib.UnsupportedShape(f"acquisition search: D={D} > 32 not supported")


def _xf_flag(pt, ctx, D):
    """1: ``pt`` is in the context's slot 0; 0: it is the identity.  Any other transformer cannot run on the device."""
    if _xf.upload(pt, ctx, 0, D) is not None:
        return 1
    if pt is None or isinstance(pt, IdentityTransformer):
        return 0
    raise _lib.UnsupportedShape("acquisition search: the parameter transformer is not one the device runs "
                                "(pyvbmc_amd/transformer.py)")


def _int_bits(integer_vars, D):
    if integer_vars is None or not np.any(integer_vars):
        return 0
    iv = np.asarray(integer_vars)
    dims = np.flatnonzero(iv) if iv.dtype == bool else np.unique(iv.astype(np.int64) % D)
    return int(sum(1 << int(d) for d in dims))


def _fill(ctx, D, sources, lb_search, ub_search, int_bits, use_xf, fetch):
    """``vbmc_search_fill`` for the sources of ``philox_plan``; returns the set when ``fetch``."""
    arr = (_lib.SearchSource * max(1, len(sources)))()
    keep = []
    M = 0
    for e, (kind, rows, data, df, key) in zip(arr, sources):
        if kind in (_lib.SRC_AFFINE, _lib.SRC_BOX):  # (mean, A) or (lb, ub): one block
            block = _lib.f64(np.concatenate((np.ravel(data[0]), np.ravel(data[1]))))
        else:
            block = None if data is None else _lib.f64(data)
        keep.append(block)
        e.kind, e.rows, e.data, e.df, e.seed = kind, int(rows), _lib.ptr(block), float(df), int(key)
        M += int(rows)
    lb = _lib.f64(np.ravel(lb_search))
    ub = _lib.f64(np.ravel(ub_search))
    out = np.empty((M, D)) if fetch else None
    ctx.check(ctx._lib.vbmc_search_fill(ctx._h, D, len(sources), arr, _lib.ptr(lb), _lib.ptr(ub), int_bits, use_xf,
                                        _lib.ptr(out)))
    return out


def _philox_sources(sources, pt, use_xf):
    """Cache rows of a transformer the device does not run are transformed here and go in as copies."""
    if use_xf:
        return sources
    return [(_lib.SRC_COPY, rows, np.asarray(pt(data) if pt is not None else data, dtype=np.float64), df, key)
            if kind == _lib.SRC_TRANSFORM and rows > 0 else (kind, rows, data, df, key)
            for kind, rows, data, df, key in sources]


def put_points(ctx, X, int_bits=0, use_xf=0):
    """``vbmc_search_put``: the rows of ``X`` become the context's resident search set, integer columns rounded."""
    X = _lib.f64(np.atleast_2d(X))
    ctx.check(ctx._lib.vbmc_search_put(ctx._h, X.shape[0], X.shape[1], _lib.ptr(X), int_bits, use_xf))


def evaluate_resident(ctx, M, D, kind, y_max, tol_var, u, noise, use_xf, lb_eps_orig, ub_eps_orig):
    """``vbmc_search_eval`` on the resident set of M rows: ``(acq, order, X_sorted)``.  ``noise``: ``(X_rescaled,
    sn2_new, gp_length_scale)`` for the kinds that need the per-point noise, else ``(None, None, None)``."""
    lb_eps, ub_eps = _lib.f64(np.ravel(lb_eps_orig)), _lib.f64(np.ravel(ub_eps_orig))
    acq = np.empty(M)
    order = np.empty(M, dtype=np.int64)
    X_sorted = np.empty((M, D))
    ctx.check(ctx._lib.vbmc_search_eval(ctx._h, kind, y_max, tol_var, u, 0 if noise[0] is None else noise[0].shape[0],
                                        _lib.ptr(noise[0]), _lib.ptr(noise[1]), _lib.ptr(noise[2]), use_xf, _lib.ptr(lb_eps),
                                        _lib.ptr(ub_eps), _lib.ptr(acq), order.ctypes.data_as(C.POINTER(C.c_int64)),
                                        _lib.ptr(X_sorted)))
    return acq, order, X_sorted


def get_search_points(number_of_points, optim_state, function_logger, vp, options, *, rng=None, seed=None, device=True,
                      ctx=None):
    """``_get_search_points`` (:647-837): ``(search_X, idx_cache)``, the reference's arguments, return values and
    ``ValueError``.  ``options``: anything with ``.get``; ``function_logger`` needs ``X``, ``y``, ``X_flag`` and
    ``parameter_transformer``.  ``rng`` / ``seed`` / ``device``: the module docstring."""
    mode = _rng_mode(rng)
    pt = function_logger.parameter_transformer
    D = optim_state.get("ub_search").shape[1]
    if mode == "numpy":
        transform = pt
        if device and _xf.candidate(pt):
            dctx = ctx if ctx is not None else getattr(vp, "_ctx", None)
            if dctx is None and _lib.device_count() > 0:
                dctx = _lib.default_context()
            if dctx is not None and dctx.device >= 0 and D <= 32 and _xf.upload(pt, dctx, 0, D) is not None:
                transform = lambda x: _xf.transform_points(dctx, np.atleast_2d(x), _xf.FORWARD, D)  # noqa: E731
        return _points_numpy(number_of_points, optim_state, function_logger, vp, options, transform)
    _check_D(D)
    ctx = ctx_of(vp, ctx)
    seed = _seed_or_draw(seed)
    sources, idx_cache = philox_plan(number_of_points, optim_state, function_logger, vp, options, seed)
    upload_vp(vp, ctx)
    use_xf = 1 if _xf.upload(pt, ctx, 0, D) is not None else 0
    X = _fill(ctx, D, _philox_sources(sources, pt, use_xf), optim_state.get("lb_search"),
              optim_state.get("ub_search"), 0, use_xf, True)
    return X, idx_cache


def search(acq_fcn, gp, vp, function_logger, optim_state, options, *, number_of_points=None, rng=None, seed=None,
           ctx=None):
    """The search lines of ``active_sample`` (:310-349) through the device: draw (or upload) the points, round the
    integer variables, prepare the importance state, evaluate the acquisition with the hard-bound mask, rank.

    Returns an object with ``X_acq`` (1, D), ``idx_cache_acq``, ``acq_fast`` (M), ``order`` (M: the stable ascending
    order of ``acq_fast``, NaN last), and ``X_search`` / ``idx_cache`` with the chosen row removed.  As the reference,
    it stores ``optim_state["search_cache"]`` when ``options["search_cache_frac"] > 0`` (and then takes the first of
    the order, else ``np.argmin``), ``optim_state["active_importance_sampling"]`` for the importance-sampled kinds and
    ``optim_state["var_log_joint_samples"]`` when the acquisition asks for it."""
    mode = _rng_mode(rng)
    D = optim_state.get("ub_search").shape[1]
    _check_D(D)
    ctx = ctx_of(vp, ctx)
    if ctx.device < 0:
        raise _lib.NoDeviceError(_lib.E_NODEV, "search needs a gfx950 device (pyvbmc_amd has no CPU fallback)")
    if number_of_points is None:
        number_of_points = options["ns_search"]
    acq_eval = string_to_acq(acq_fcn) if isinstance(acq_fcn, str) else acq_fcn  # :318-321
    if not isinstance(acq_eval, AbstractAcqFcn) or acq_eval._kind is None:
        raise TypeError("search: acq_fcn must be one of pyvbmc_amd.acquisition's classes (or its constructor string)")
    pt = function_logger.parameter_transformer
    int_bits = _int_bits(optim_state.get("integer_vars"), D)
    upload_vp(vp, ctx)

    # :310-316: the points and their rounding; they stay on the device
    if mode == "philox":
        seed = _seed_or_draw(seed)
        sources, idx_cache = philox_plan(number_of_points, optim_state, function_logger, vp, options, seed)
        use_xf = _xf_flag(pt, ctx, D)
        _fill(ctx, D, _philox_sources(sources, pt, use_xf), optim_state.get("lb_search"),
              optim_state.get("ub_search"), int_bits, use_xf, False)
    else:
        X, idx_cache = get_search_points(number_of_points, optim_state, function_logger, vp, options, rng="numpy",
                                         ctx=ctx)
        use_xf = _xf_flag(pt, ctx, D) if int_bits else 0
        put_points(ctx, X, int_bits, use_xf)
    M = X.shape[0] if mode == "numpy" else sum(int(s[1]) for s in sources)

    # :323-327
    if acq_eval.acq_info.get("importance_sampling"):
        kw = {"rng": mode, "seed": sub_seed(seed, len(SOURCES))} if mode == "philox" else {"rng": mode}
        optim_state["active_importance_sampling"] = active_importance_sampling(vp, gp, acq_eval, options, **kw)
    # :329-332
    if acq_eval.acq_info.get("compute_var_log_joint"):
        from .variational_optimization import _gp_log_joint

        optim_state["var_log_joint_samples"] = _gp_log_joint(vp, gp, 0, 0, 0, 1)[2]

    # :334-335: AbstractAcqFcn.__call__ on the resident points
    upload_gp(gp, ctx)
    is_kind = isinstance(acq_eval, _QuantileAcq)
    if is_kind:
        acq_eval._upload_state(gp, optim_state["active_importance_sampling"], ctx)
    kind = _lib.ACQ_IS if is_kind else acq_eval._kind
    noise = (None, None, None)
    if is_kind or kind == ACQ_NOISY:
        noise = (_lib.f64(gp.temporary_data.get("X_rescaled")), _lib.f64(np.ravel(gp.temporary_data.get("sn2_new"))),
                 _lib.f64(np.ravel(optim_state.get("gp_length_scale"))))
    tol_var = float(optim_state.get("tol_gp_var")) if optim_state.get("variance_regularized_acq_fcn") else 0.0
    y_max = float(function_logger.y_max) if kind in (ACQ_STD, ACQ_LOG, ACQ_NOISY) else 0.0
    acq_fast, order, X_sorted = evaluate_resident(ctx, M, D, kind, y_max, tol_var, float(getattr(acq_eval, "u", 0.0)), noise,
                                                  _xf_flag(vp.parameter_transformer, ctx, D),
                                                  optim_state.get("lb_eps_orig"), optim_state.get("ub_eps_orig"))
    X_search = np.empty((M, D))
    X_search[order] = X_sorted

    # :337-342
    if options["search_cache_frac"] > 0:
        optim_state["search_cache"] = X_sorted
        idx = order[0]
    else:
        idx = np.argmin(acq_fast)
    # :344-349
    X_acq = X_search[[idx]]
    idx_cache_acq = idx_cache[idx]
    return SimpleNamespace(X_acq=X_acq, idx_cache_acq=idx_cache_acq, acq_fast=acq_fast, order=order,
                           X_search=np.delete(X_search, idx, 0), idx_cache=np.delete(idx_cache, idx, 0))


def cmaes_resident(ctx, D, kind, y_max, tol_var, u, noise, use_xf, lb_eps_orig, ub_eps_orig, x0, sigma0, lb, ub, *,
                   int_bits=0, lam=None, max_fevals, tol_fun, tol_x=None, seed=0):
    """``vbmc_search_cmaes``: R CMA-ES runs (the rows of ``x0``) in lockstep on the GP, mixture and importance state the
    context holds; the scoring arguments are ``evaluate_resident``'s.  Returns ``x_best`` (R, D), ``f_best``, ``f0``,
    ``mean``, ``sigma``, ``C`` (R, D, D) and ``stats`` (R, 4: generations, evaluations, stop reason, generation of the
    best), the fields ``pyvbmc_amd.cmaes.fmin`` returns per run."""
    x0 = _lib.f64(np.atleast_2d(x0))
    R = x0.shape[0]
    sigma0 = _lib.f64(np.broadcast_to(np.asarray(sigma0, dtype=np.float64), (R,)))
    lb, ub = _lib.f64(np.ravel(lb)), _lib.f64(np.ravel(ub))
    lb_eps, ub_eps = _lib.f64(np.ravel(lb_eps_orig)), _lib.f64(np.ravel(ub_eps_orig))
    opts = _lib.CmaesOpts(0 if lam is None else int(lam), int(max_fevals), float(tol_fun),
                          0.0 if tol_x is None else float(tol_x), int(seed) % 2**64)
    out = SimpleNamespace(x_best=np.empty((R, D)), f_best=np.empty(R), f0=np.empty(R), mean=np.empty((R, D)), sigma=np.empty(R),
                          C=np.empty((R, D, D)), stats=np.empty((R, 4), dtype=np.int64))
    ctx.check(ctx._lib.vbmc_search_cmaes(ctx._h, kind, y_max, tol_var, u, 0 if noise[0] is None else noise[0].shape[0],
                                         _lib.ptr(noise[0]), _lib.ptr(noise[1]), _lib.ptr(noise[2]), use_xf, _lib.ptr(lb_eps),
                                         _lib.ptr(ub_eps), R, _lib.ptr(x0), _lib.ptr(sigma0), _lib.ptr(lb), _lib.ptr(ub), int_bits,
                                         C.byref(opts), _lib.ptr(out.x_best), _lib.ptr(out.f_best), _lib.ptr(out.f0),
                                         _lib.ptr(out.mean), _lib.ptr(out.sigma), _lib.ptr(out.C),
                                         out.stats.ctypes.data_as(C.POINTER(C.c_int64))))
    return out


def _scoring_args(acq_eval, gp, vp, function_logger, optim_state, ctx, D):
    """What ``search`` hands to ``evaluate_resident`` for an acquisition object, with the GP, the mixture and the
    importance state uploaded: ``(kind, y_max, tol_var, u, noise, use_xf)``."""
    upload_vp(vp, ctx)
    upload_gp(gp, ctx)
    is_kind = isinstance(acq_eval, _QuantileAcq)
    if is_kind:
        acq_eval._upload_state(gp, optim_state["active_importance_sampling"], ctx)
    kind = _lib.ACQ_IS if is_kind else acq_eval._kind
    noise = (None, None, None)
    if is_kind or kind == ACQ_NOISY:
        noise = (_lib.f64(gp.temporary_data.get("X_rescaled")), _lib.f64(np.ravel(gp.temporary_data.get("sn2_new"))),
                 _lib.f64(np.ravel(optim_state.get("gp_length_scale"))))
    tol_var = float(optim_state.get("tol_gp_var")) if optim_state.get("variance_regularized_acq_fcn") else 0.0
    y_max = float(function_logger.y_max) if kind in (ACQ_STD, ACQ_LOG, ACQ_NOISY) else 0.0
    return kind, y_max, tol_var, float(getattr(acq_eval, "u", 0.0)), noise, _xf_flag(vp.parameter_transformer, ctx, D)


def refine(res, acq_fcn, gp, vp, function_logger, optim_state, options, *, n_starts=1, seed=None, device=True, ctx=None):
    """The local optimisation that follows the ranked search in ``active_sample`` (:355-423): from the best search
    point of ``res`` (what ``search`` returned) the acquisition function is minimised in the search box, and the result
    replaces the point only if it improves on the search's value.

    * ``options["search_optimizer"] == "none"``: ``res.X_acq`` comes back unchanged.
    * The box (:366-375): the search bounds extended to contain the start; with non-finite search bounds,
      ``gp.X.min(0) - 0.1 range`` .. ``gp.X.max(0) + 0.1 range``, extended likewise.  (The reference writes
      ``np.minimum(gp.X, x0)`` there, an N x D array; the per-dimension extreme is what is meant.)
    * ``tol_fun`` (:377-380): 1e-2 for a log-valued acquisition, else ``max(1e-12, |f_val_old| 1e-3)``.
    * The initial step (:383-389): ``max(sqrt(diag Sigma))``, Sigma the posterior's covariance in transformed space
      (``search_cmaes_vp_init``) or that of the HPD set of ``options["hpd_frac"]``.
    * ``max_fevals = options["search_max_fun_evals"]``.
    * D >= 2: CMA-ES -- ``vbmc_search_cmaes`` on the device (every generation one batch through the scoring launches
      of ``search``), or with ``device=False`` ``pyvbmc_amd.cmaes.fmin`` around this package's batched acquisition call:
      the same algorithm and draws.  The optimiser is this package's own (csrc/cmaes.hip), not ``cma``: no
      ``cma.NoiseHandler`` (the acquisition functions are deterministic), no boundary transformation, no restarts.
      ``n_starts > 1``: the start and the next best ranked rows of ``res`` with a finite value run side by side (the
      reference has one), and the best of the runs is taken.
    * D == 1: SciPy's Nelder-Mead around the acquisition call, as the reference; host code.
    * Accepted only if ``f_best < f_val_old``; then ``X_acq`` is the rounded point (``_real2int``) and
      ``idx_cache_acq`` NaN (:417-423).

    Returns ``X_acq`` (1, D), ``idx_cache_acq``, ``f_val``, ``f_val_old``, ``accepted`` and, for CMA-ES, ``stats`` (one
    row per run: generations, evaluations, stop reason, generation of the best), ``runs`` (the optimiser's fields per
    run), ``best_run`` and the optimiser's arguments ``lb``, ``ub``, ``sigma0``, ``tol_fun``."""
    from . import cmaes as _cmaes

    X_acq = np.array(res.X_acq, dtype=np.float64).reshape(1, -1)
    D = X_acq.shape[1]
    idx = int(res.order[0]) if options["search_cache_frac"] > 0 else int(np.argmin(res.acq_fast))
    f_val_old = float(res.acq_fast[idx])  # :363
    same = SimpleNamespace(X_acq=X_acq, idx_cache_acq=res.idx_cache_acq, f_val=f_val_old, f_val_old=f_val_old, accepted=False,
                           stats=None, runs=None, best_run=None)
    if options["search_optimizer"] == "none":  # :356
        return same
    acq_eval = string_to_acq(acq_fcn) if isinstance(acq_fcn, str) else acq_fcn
    if not isinstance(acq_eval, AbstractAcqFcn) or acq_eval._kind is None:
        raise TypeError("refine: acq_fcn must be one of pyvbmc_amd.acquisition's classes (or its constructor string)")
    _check_D(D)
    x0 = X_acq[0].copy()  # :364
    lb_s, ub_s = np.ravel(optim_state["lb_search"]), np.ravel(optim_state["ub_search"])
    gp_X = np.asarray(gp.X, dtype=np.float64)
    if np.isfinite(lb_s).all() and np.isfinite(ub_s).all():  # :366-375
        lb, ub = np.minimum(x0, lb_s), np.maximum(x0, ub_s)
    else:
        xrange = gp_X.max(0) - gp_X.min(0)
        lb, ub = np.minimum(gp_X.min(0), x0) - 0.1 * xrange, np.maximum(gp_X.max(0), x0) + 0.1 * xrange
    tol_fun = 1e-2 if acq_eval.acq_info.get("log_flag") else max(1e-12, abs(f_val_old * 1e-3))  # :377-380
    pt = function_logger.parameter_transformer
    integer_vars = optim_state.get("integer_vars")

    def acq_batch(X):
        return np.ravel(acq_eval(np.array(X, dtype=np.float64), gp, vp, function_logger, optim_state))

    def rounded(X):
        return AbstractAcqFcn._real2int(np.array(X, dtype=np.float64), pt, integer_vars)

    if D == 1:  # :357-361, :407-413
        from scipy.optimize import minimize

        r = minimize(lambda x: float(acq_batch(np.reshape(x, (1, 1)))[0]), x0, method="Nelder-Mead", tol=tol_fun)
        x_opt, f_opt, stats, runs, best_run = np.reshape(r.x, (1, 1)), float(r.fun), None, None, None
        x_opt = rounded(x_opt)
    else:
        optimizer = options["search_optimizer"]
        if optimizer != "cmaes":
            raise NotImplementedError("Not implemented yet")  # :414-415
        if options["search_cmaes_vp_init"]:  # :383-389
            _, Sigma = vp.moments(orig_flag=False, cov_flag=True)
        else:
            order_y = np.argsort(np.asarray(gp.y), axis=None)[::-1]
            X_hpd = gp_X[order_y[0:round(options["hpd_frac"] * gp_X.shape[0])]]
            Sigma = np.cov(X_hpd, rowvar=False, bias=True)
        sigma0 = float(np.max(np.sqrt(np.diag(np.atleast_2d(Sigma)))))
        max_fevals = int(options["search_max_fun_evals"])
        seed = _seed_or_draw(seed)
        starts = [x0]
        if n_starts > 1:  # the next best rows of the ranked set, in rank order
            X_search = np.asarray(res.X_search, dtype=np.float64)
            for j in res.order:
                j = int(j)
                if len(starts) >= n_starts or not np.isfinite(res.acq_fast[j]):
                    break
                if j != idx:
                    starts.append(np.minimum(np.maximum(X_search[j if j < idx else j - 1], lb), ub))
        starts = np.array(starts)
        if device:
            ctx = ctx_of(vp, ctx)
            if ctx.device < 0:
                raise _lib.NoDeviceError(_lib.E_NODEV, "refine(device=True) needs a gfx950 device (pyvbmc_amd has no CPU fallback)")
            kind, y_max, tol_var, u, noise, use_xf = _scoring_args(acq_eval, gp, vp, function_logger, optim_state, ctx, D)
            int_bits = _int_bits(integer_vars, D)
            if int_bits:
                _xf_flag(pt, ctx, D)
            out = cmaes_resident(ctx, D, kind, y_max, tol_var, u, noise, use_xf, optim_state.get("lb_eps_orig"),
                                 optim_state.get("ub_eps_orig"), starts, sigma0, lb, ub, int_bits=int_bits,
                                 max_fevals=max_fevals, tol_fun=tol_fun, seed=seed)
            runs = [SimpleNamespace(x_best=out.x_best[r], f_best=float(out.f_best[r]), f0=float(out.f0[r]), mean=out.mean[r],
                                    sigma=float(out.sigma[r]), C=out.C[r], stats=out.stats[r]) for r in range(len(starts))]
        else:
            runs = [_cmaes.fmin(acq_batch, s, sigma0, lb, ub, max_fevals=max_fevals, tol_fun=tol_fun, seed=seed, run=r,
                                evaluated=rounded) for r, s in enumerate(starts)]
        stats = np.array([r.stats for r in runs], dtype=np.int64)
        f_all = np.array([r.f_best for r in runs])
        best_run = int(np.nanargmin(f_all)) if np.isfinite(f_all).any() else 0
        x_opt, f_opt = np.reshape(runs[best_run].x_best, (1, D)), float(runs[best_run].f_best)
    info = dict(stats=stats, runs=runs, best_run=best_run, lb=lb, ub=ub, tol_fun=tol_fun, sigma0=sigma0 if D > 1 else None)
    if f_opt < f_val_old:  # :417-423
        return SimpleNamespace(X_acq=np.array(x_opt, dtype=np.float64), idx_cache_acq=np.nan, f_val=f_opt, f_val_old=f_val_old,
                               accepted=True, **info)
    same.__dict__.update(info)
    return same


__all__ = ["get_search_points", "search", "refine", "cmaes_resident", "philox_plan", "put_points", "evaluate_resident", "sub_seed",
           "mvn_factor", "SOURCES"]
