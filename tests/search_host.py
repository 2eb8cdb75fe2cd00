"""A NumPy restatement of the acquisition search (reference pyvbmc/vbmc/active_sample.py: ``_get_search_points``
:647-837 and the search lines :310-349) over the oracle's plain objects (oracle/mixture_ref.py ``Mixture``,
oracle/gp_ref.py ``GPData``).  TEST INFRASTRUCTURE: the mirror (pyvbmc_amd/active_search.py) is compared with it, and it
is itself held to the reference's recorded outputs (tests/test_search_host.py: tests/golden/search.npz).  Line numbers
cite the reference's file.

* ``points_numpy``   the reference's statements on NumPy's global stream (``vp.sample`` restated by ``sample_numpy``)
* ``points_philox``  the same sources from the device generator's streams (oracle/philox_ref.py, oracle/sample_ref.py):
                     the small host draws from ``np.random.default_rng(seed)``, source j under the key
                     ``seed + (j + 1) * 0x9E3779B97F4A7C15 mod 2^64`` (j: heavy 0, mvn 1, the six HPD fractions 2-7, box 8,
                     vp 9), Gaussian and box rows from Philox stream 7.  Also returns the row block of every source.
* ``real2int``, ``acq_values``, ``rank``  the rounding, the acquisition with the hard-bound mask through a parameter
                     transformer, and the ranking lines
* ``load_case``, ``wide_case``, ``gp_fixture``  the tests' inputs
"""
import math
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import acq_ref, mixture_ref, philox_ref, sample_ref  # noqa: E402

STREAM = 7
KEY_STEP = 0x9E3779B97F4A7C15


def load_case(g, name, number_of_points=None):
    """A case of tests/golden/search.npz (tools/make_search_golden.py) as the functions' arguments: ``mix``,
    ``optim_state``, ``flog`` (its transformer a tests/transform_host.py ``RefShapedTransformer``), ``options``,
    ``number_of_points``, the NumPy seed and the reference's recorded result."""
    from transform_host import RefShapedTransformer

    pt = RefShapedTransformer.from_golden(g, f"{name}_pt")
    mix = mixture_ref.Mixture.make(g[f"{name}_mu"], g[f"{name}_sigma"].ravel(), g[f"{name}_lambd"].ravel(),
                                   g[f"{name}_w"].ravel())
    optim_state = {"cache": {"x_orig": g[f"{name}_x_orig"].copy()}, "search_cache": g[f"{name}_search_cache"].copy()}
    for k in ("lb_search", "ub_search", "plb_tran", "pub_tran"):
        optim_state[k] = g[f"{name}_{k}"].copy()
    flog = SimpleNamespace(X=g[f"{name}_X"], y=g[f"{name}_y"], X_flag=g[f"{name}_X_flag"], parameter_transformer=pt)
    options = dict(zip([str(k) for k in g["option_keys"]], g[f"{name}_options"].tolist()))
    return SimpleNamespace(name=name, D=int(g[f"{name}_D"]), K=int(g[f"{name}_K"]), mix=mix, pt=pt, optim_state=optim_state,
                           flog=flog, options=options,
                           number_of_points=int(g[f"{name}_number_of_points"]) if number_of_points is None else number_of_points,
                           np_seed=int(g[f"{name}_np_seed"]), search_X=g[f"{name}_search_X"], idx_cache=g[f"{name}_idx_cache"],
                           raised=bool(g[f"{name}_raised"]))


def package_vp(case, ctx=None):
    """The package's VariationalPosterior with the case's mixture and transformer."""
    from pyvbmc_amd import VariationalPosterior

    vp = VariationalPosterior(case.D, case.K, parameter_transformer=case.pt)
    vp.mu, vp.sigma = case.mix.mu.copy(), case.mix.sigma.reshape(1, -1).copy()
    vp.lambd, vp.w = case.mix.lambd.reshape(-1, 1).copy(), case.mix.w.reshape(1, -1).copy()
    vp.eta = np.log(vp.w)
    if ctx is not None:
        vp.ctx = ctx
    return vp


def source_key(seed, j):
    return (int(seed) + (j + 1) * KEY_STEP) % 2**64


def sample_numpy(mix, N, df=np.inf):
    """``vp.sample(N, orig_flag=False, balance_flag=True, df=df)[0]`` on np.random
    (variational_posterior.py:296-353)."""
    lam = mix.lambd.reshape(1, -1)
    w = mix.w.reshape(1, -1)
    sigma = mix.sigma.reshape(1, -1)
    heavy = np.isfinite(df) and df != 0
    if mix.K > 1:
        reps = np.floor(w * N).astype("int")
        i = np.repeat(range(mix.K), reps.ravel())
        if N > i.shape[0]:
            w_extra = w * N - reps
            n_extra = np.ceil(np.sum(w_extra))
            w_extra += w * (n_extra - sum(w_extra))
            w_extra /= np.sum(w_extra)
            i = np.append(i, np.random.choice(range(mix.K), size=n_extra.astype("int"), p=w_extra.ravel()))
        np.random.shuffle(i)
        i = i[:N]
        if heavy:
            t = df / 2 / np.sqrt(np.random.gamma(df / 2, df / 2, (N, 1)))
            return mix.mu.T[i] + lam * np.random.randn(N, mix.D) * t * sigma[:, i].T
        return mix.mu.T[i] + lam * np.random.randn(N, mix.D) * sigma[:, i].T
    if heavy:
        t = df / 2 / np.sqrt(np.random.gamma(df / 2, df / 2, (N, 1)))
        return mix.mu.T + lam * t * np.random.randn(N, mix.D) * sigma
    return mix.mu.T + lam * np.random.randn(N, mix.D) * sigma


def moments_tran(mix):
    """``vp.moments(orig_flag=False, cov_flag=True)`` in the reference's order of operations
    (variational_posterior.py:793-804): the covariance's last bits decide those of every draw made with its factor."""
    w, sigma, lambd = mix.w.reshape(1, -1), mix.sigma.reshape(1, -1), mix.lambd.reshape(-1, 1)
    mubar = np.sum(w * mix.mu, axis=1)
    cov = np.sum(w * sigma**2) * np.eye(len(lambd)) * lambd**2
    for k in range(mix.K):
        cov += w[:, k] * ((mix.mu[:, k] - mubar)[:, np.newaxis]).dot((mix.mu[:, k] - mubar)[:, np.newaxis].T)
    return mubar.reshape(1, -1), cov


def get_hpd(X, y, hpd_frac):
    """stats/get_hpd.py:34-37"""
    order = np.argsort(y, axis=None)[::-1]
    return X[order[0:round(hpd_frac * X.shape[0])]]


def hpd_fractions(options, N_hpd, u4):
    """:743-756"""
    hpd_min = options.get("hpd_frac") / 8
    hpd_max = options.get("hpd_frac")
    fracs = np.sort(np.concatenate((u4 * (hpd_max - hpd_min) + hpd_min, np.array([hpd_min, hpd_max]))))
    return fracs, np.diff(np.round(np.linspace(0, N_hpd, len(fracs) + 1)))


def hpd_gaussian(X, y, frac, D):
    """:765-780"""
    X_hpd = get_hpd(X, y, frac)
    if X_hpd.size == 0:
        mubar = X[np.argmax(y)]
        sigmabar = np.cov(X, rowvar=False)
    else:
        mubar = np.mean(X_hpd, axis=0)
        sigmabar = np.cov(X_hpd, bias=True, rowvar=False)
    if sigmabar.shape != (D, D):
        sigmabar = np.ones((D, D)) * sigmabar
    return mubar, sigmabar


def box_bounds(optim_state, X):
    """:789-804"""
    lb_search, ub_search = optim_state.get("lb_search"), optim_state.get("ub_search")
    X_diam = np.amax(X, axis=0) - np.amin(X, axis=0)
    if np.all(np.isfinite(lb_search)) and np.all(np.isfinite(ub_search)):
        box_lb, box_ub = lb_search, ub_search
    else:
        plb_tran, pub_tran = optim_state.get("plb_tran"), optim_state.get("pub_tran")
        box_lb = plb_tran - 3 * (pub_tran - plb_tran)
        box_ub = pub_tran + 3 * (pub_tran - plb_tran)
    return (np.maximum(np.amin(X, axis=0) - 0.5 * X_diam, box_lb), np.minimum(np.amax(X, axis=0) + 0.5 * X_diam, box_ub))


def _counts(number_of_points, n_cache_total, options):
    N_random = number_of_points - n_cache_total  # :710
    c = {k: round(options.get(k + "_frac") * N_random)
         for k in ("search_cache", "heavy_tail_search", "mvn_search", "hpd_search", "box_search")}
    return N_random, c


def points_numpy(number_of_points, optim_state, flog, mix, options):
    """The reference's statements, NumPy's global stream."""
    x0 = np.copy(optim_state["cache"]["x_orig"])
    lb_search, ub_search = optim_state.get("lb_search"), optim_state.get("ub_search")
    D = ub_search.shape[1]
    search_X = np.full((0, D), np.nan)
    idx_cache = np.array([])
    if x0.size > 0:
        N_cache = math.ceil(number_of_points * options.get("cache_frac"))
        idx_cache = np.random.permutation(x0.shape[0])[: min(N_cache, x0.shape[0])]
        search_X = flog.parameter_transformer(x0[idx_cache])
    if x0.shape[0] < number_of_points:
        N_random, c = _counts(number_of_points, x0.shape[0], options)
        parts = [np.full((0, D), np.nan)]
        if c["search_cache"] > 0:
            sc = optim_state.get("search_cache")
            parts.append(sc[: min(len(sc), c["search_cache"])])
        if c["heavy_tail_search"] > 0:
            parts.append(sample_numpy(mix, c["heavy_tail_search"], df=3))
        if c["mvn_search"] > 0:
            mubar, sigmabar = moments_tran(mix)
            parts.append(np.random.multivariate_normal(np.ravel(mubar), sigmabar, size=c["mvn_search"]))
        if c["hpd_search"] > 0:
            fracs, n_vec = hpd_fractions(options, c["hpd_search"], np.random.uniform(size=4))
            X, y = flog.X[flog.X_flag], flog.y[flog.X_flag]
            for f, n in zip(fracs, n_vec):
                if n == 0:
                    continue
                mubar, sigmabar = hpd_gaussian(X, y, f, D)
                parts.append(np.random.multivariate_normal(mubar, sigmabar, size=int(n)))
        if c["box_search"] > 0:
            box_lb, box_ub = box_bounds(optim_state, flog.X[flog.X_flag])
            parts.append(np.random.standard_normal((c["box_search"], D)) * (box_ub - box_lb) + box_lb)
        random_Xs = np.concatenate(parts, axis=0)
        if N_random < random_Xs.shape[0]:
            raise ValueError("more points sampled than requested")
        N_vp = max(0, N_random - sum(c.values()))
        if N_vp > 0:
            random_Xs = np.append(random_Xs, sample_numpy(mix, N_vp), axis=0)
        search_X = np.append(search_X, random_Xs, axis=0)
        idx_cache = np.append(idx_cache, np.full(N_random, np.nan))
    return np.minimum(np.maximum(search_X, lb_search), ub_search), idx_cache


def mvn_factor(cov):
    """np.random.multivariate_normal's factor: x = z @ A + mean with A = sqrt(s)[:, None] * v of the SVD; singular
    values below np.linalg.matrix_rank's tolerance (s.max() D eps: the SVD's rounding) are zero."""
    _, s, v = np.linalg.svd(np.atleast_2d(cov))
    s = np.where(s > s.max() * len(s) * np.finfo(np.float64).eps, s, 0.0)
    return np.sqrt(s)[:, None] * v


def affine_rows(n, mean, A, key):
    """z A + mean with the products added in row order of A (csrc/search.hip), z from Philox stream 7."""
    D = A.shape[0]
    z = philox_ref.normals(np.arange(n, dtype=np.uint64), D, key, STREAM)
    acc = np.zeros((n, D))
    mag = np.abs(np.ravel(mean))[None, :] * np.ones((n, 1))
    for i in range(D):
        acc = acc + z[:, i:i + 1] * A[i][None, :]
        mag = mag + np.abs(z[:, i:i + 1] * A[i][None, :])
    return acc + np.ravel(mean)[None, :], mag


def box_rows(n, lb, ub, key):
    z = philox_ref.normals(np.arange(n, dtype=np.uint64), lb.size, key, STREAM)
    return z * (np.ravel(ub) - np.ravel(lb)) + np.ravel(lb), np.abs(z * (np.ravel(ub) - np.ravel(lb))) + np.abs(np.ravel(lb))


def mixture_rows(mix, n, key, df=np.inf):
    x, lab = sample_ref.sample(mix, n, key, True, df)
    return x, np.abs(mix.mu.T[lab]) + np.abs(x - mix.mu.T[lab])


def points_philox(number_of_points, optim_state, flog, mix, options, seed, detail=None):
    """``(search_X, idx_cache, blocks)``; blocks: name -> (first row, rows, parameters) of every source drawn.
    ``detail`` (a dict) receives ``raw``, the points before the clamp, and ``cond``, per element the sum of the magnitudes
    of the terms it is added up from over its own magnitude (1 for rows that are copied or transformed): the factor
    by which a relative error of the normals can grow in it."""
    g = np.random.default_rng(seed)
    x0 = np.copy(optim_state["cache"]["x_orig"])
    lb_search, ub_search = optim_state.get("lb_search"), optim_state.get("ub_search")
    D = ub_search.shape[1]
    parts, mags, blocks = [], [], {}
    idx_cache = np.array([])
    row = 0

    def put(name, rows, info=None):
        nonlocal row
        rows, mag = rows if isinstance(rows, tuple) else (rows, None)
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, D)
        parts.append(rows)
        mags.append(np.abs(rows) if mag is None else mag)
        blocks[name] = (row, rows.shape[0], info)
        row += rows.shape[0]

    if x0.size > 0:
        N_cache = math.ceil(number_of_points * options.get("cache_frac"))
        idx_cache = g.permutation(x0.shape[0])[: min(N_cache, x0.shape[0])]
        put("cache", flog.parameter_transformer(x0[idx_cache]))
    if x0.shape[0] < number_of_points:
        N_random, c = _counts(number_of_points, x0.shape[0], options)
        n_before = row
        if c["search_cache"] > 0:
            sc = optim_state.get("search_cache")
            put("search_cache", sc[: min(len(sc), c["search_cache"])])
        if c["heavy_tail_search"] > 0:
            put("heavy", mixture_rows(mix, c["heavy_tail_search"], source_key(seed, 0), 3.0))
        if c["mvn_search"] > 0:
            mubar, sigmabar = moments_tran(mix)
            A = mvn_factor(sigmabar)
            put("mvn", affine_rows(c["mvn_search"], mubar, A, source_key(seed, 1)), (np.ravel(mubar), A))
        if c["hpd_search"] > 0:
            fracs, n_vec = hpd_fractions(options, c["hpd_search"], g.uniform(size=4))
            X, y = flog.X[flog.X_flag], flog.y[flog.X_flag]
            for j, (f, n) in enumerate(zip(fracs, n_vec)):
                if n == 0:
                    continue
                mubar, sigmabar = hpd_gaussian(X, y, f, D)
                A = mvn_factor(sigmabar)
                put(f"hpd{j}", affine_rows(int(n), mubar, A, source_key(seed, 2 + j)), (np.ravel(mubar), A, f))
        if c["box_search"] > 0:
            box_lb, box_ub = box_bounds(optim_state, flog.X[flog.X_flag])
            put("box", box_rows(c["box_search"], np.ravel(box_lb), np.ravel(box_ub), source_key(seed, 8)),
                (np.ravel(box_lb), np.ravel(box_ub)))
        if N_random < row - n_before:
            raise ValueError("more points sampled than requested")
        N_vp = max(0, N_random - sum(c.values()))
        if N_vp > 0:
            put("vp", mixture_rows(mix, N_vp, source_key(seed, 9)))
        idx_cache = np.append(idx_cache, np.full(N_random, np.nan))
    search_X = np.concatenate(parts, axis=0) if parts else np.full((0, D), np.nan)
    if detail is not None:
        detail["raw"] = search_X
        with np.errstate(divide="ignore", invalid="ignore"):
            detail["cond"] = (np.concatenate(mags, axis=0) if mags else search_X) / np.abs(search_X)
    return np.minimum(np.maximum(search_X, lb_search), ub_search), idx_cache, blocks


def real2int(X, pt, integer_vars, return_pre=False):
    """AbstractAcqFcn._real2int (abstract_acq_fcn.py:149-193); ``return_pre``: also the values before np.around."""
    X = np.array(X, dtype=np.float64)
    pre = None
    if integer_vars is not None and np.any(integer_vars):
        X_temp = pt.inverse(X)
        pre = X_temp[:, integer_vars].copy()
        X_temp[:, integer_vars] = np.around(X_temp[:, integer_vars])
        X_temp = pt(X_temp)
        X[:, integer_vars] = X_temp[:, integer_vars]
    return (X, pre) if return_pre else X


def hard_bound_mask(X, pt, optim_state):
    """abstract_acq_fcn.py:133-139"""
    X_orig = pt.inverse(X)
    return np.any(X_orig < optim_state["lb_eps_orig"], axis=1) | np.any(X_orig > optim_state["ub_eps_orig"], axis=1)


def acq_values(kind, X, ogp, mix, y_max, optim_state, pt, X_rescaled=None, sn2_new=None, ais=None, u=None):
    """AbstractAcqFcn.__call__ after the rounding: ``kind`` one of acq_ref.STD .. NOISY, or "viqr" / "imiqr" with the
    importance state ``ais`` (oracle/acq_ref.py quantile_acq, then the regularisation and clamp of :110-131)."""
    open_state = dict(optim_state, lb_eps_orig=np.full(X.shape[1], -np.inf), ub_eps_orig=np.full(X.shape[1], np.inf))
    with np.errstate(all="ignore"):
        if kind in ("viqr", "imiqr"):
            from oracle import gp_ref

            sn2 = acq_ref.estimate_observation_noise(X, X_rescaled, sn2_new, optim_state["gp_length_scale"])
            acq = acq_ref.quantile_acq(ogp, X, sn2, ais, u, kind == "imiqr")
            if optim_state.get("variance_regularized_acq_fcn"):
                f_mu, f_s2 = gp_ref.predict(ogp, X, separate_samples=True)
                S = f_mu.shape[1]
                f_bar = np.sum(f_mu, axis=1, keepdims=True) / S
                var_f = np.sum((f_mu - f_bar) ** 2, axis=1) / (S - 1) if S > 1 else 0
                var_tot = var_f + np.sum(f_s2, axis=1) / S
                tol = optim_state.get("tol_gp_var")
                low = var_tot < tol
                acq[low] += tol / var_tot[low] - 1
            acq = np.maximum(acq, -sys.float_info.max)
        else:
            acq = acq_ref.acq_call(kind, X, ogp, mix, y_max, open_state, X_rescaled=X_rescaled, sn2_new=sn2_new)
    acq[hard_bound_mask(X, pt, optim_state)] = np.inf
    return acq


def rank(X_search, idx_cache, acq_fast, optim_state, options):
    """:337-349 with the stable order."""
    order = np.argsort(acq_fast, kind="stable")
    if options["search_cache_frac"] > 0:
        optim_state["search_cache"] = X_search[order]
        idx = order[0]
    else:
        idx = np.argmin(acq_fast)
    return SimpleNamespace(X_acq=X_search[[idx]], idx_cache_acq=idx_cache[idx], acq_fast=acq_fast, order=order,
                           X_search=np.delete(X_search, idx, 0), idx_cache=np.delete(idx_cache, idx, 0))


# ---------------------------------------------------------------------------------------------- fixtures for the GPU tests
def wide_case(D=32, K=2, N=40, number_of_points=300, seed=5, centre=25.0, sigma_scale=1.0):
    """A case like tests/golden/search.npz's at another shape (nothing recorded): unbounded transformer dimensions with a
    shift and a scale, a 4-row cache, search cache and HPD on.  Everything lies around ``centre``, far from zero in units
    of its spread: no element of a point is a sum that cancels, so a relative tolerance means the same for all of them."""
    from transform_host import RefShapedTransformer

    r = np.random.default_rng(seed)
    pt = RefShapedTransformer(np.zeros(D), np.full(D, -np.inf), np.full(D, np.inf), 0.1 * r.standard_normal(D),
                              0.5 + r.random(D))
    lam = 0.5 + r.random(D)
    mix = mixture_ref.Mixture.make(centre + r.standard_normal((D, K)), sigma_scale * (0.4 + 0.5 * r.random(K)),
                                   lam / np.sqrt(np.sum(lam**2) / D), np.full(K, 1.0 / K))
    X = centre + 1.2 * r.standard_normal((N, D))
    y = (-0.5 * np.sum((X - centre) ** 2, axis=1) + 0.1 * r.standard_normal(N)).reshape(-1, 1)
    optim_state = {"cache": {"x_orig": r.uniform(-2, 2, size=(4, D))},
                   "search_cache": centre + 0.8 * r.standard_normal((50, D)),
                   "lb_search": np.full((1, D), centre - 1.6), "ub_search": np.full((1, D), centre + 1.9),
                   "plb_tran": np.full((1, D), centre - 1.0), "pub_tran": np.full((1, D), centre + 1.0)}
    flog = SimpleNamespace(X=X, y=y, X_flag=np.ones(N, dtype=bool), parameter_transformer=pt)
    options = dict(cache_frac=0.5, search_cache_frac=0.125, heavy_tail_search_frac=0.125, mvn_search_frac=0.125,
                   hpd_search_frac=0.25, box_search_frac=0.125, hpd_frac=0.8)
    return SimpleNamespace(name="wide", D=D, K=K, mix=mix, pt=pt, optim_state=optim_state, flog=flog, options=options,
                           number_of_points=number_of_points)


def gp_fixture(case, S=2, seed=9, length_mult=1.0):
    """An oracle GP (S hyper-parameter samples, negative-quadratic mean) on the case's evaluated points, with the
    per-point noise table and length scale of the noisy acquisition functions.  ``length_mult`` multiplies the length
    scales (0.8 .. 1.1): at D = 20 and more, a search point of the wide case and a training point are so far apart in
    units of those that their median covariance is 3e-12 sf^2 (4e-17 at D = 32), below every bound the values are held to."""
    from oracle import gp_ref

    r = np.random.default_rng(seed)
    D = case.D
    X, y = case.flog.X[case.flog.X_flag], case.flog.y[case.flog.X_flag]
    hyp = np.array([np.concatenate([np.log(length_mult * (0.8 + 0.3 * r.random(D))), [np.log(2.0)], [np.log(0.05 * (s + 1))], [0.1], np.zeros(D),
                                    np.zeros(D)]) for s in range(S)])
    ogp = gp_ref.make_gp(X, y, hyp, gp_ref.MEAN_NEGQUAD)
    length = np.exp(hyp[:, :D].mean(axis=0))
    return ogp, length, 0.01 + r.random(X.shape[0])
