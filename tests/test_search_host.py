"""The acquisition search's point generation on the host (no GPU): pyvbmc_amd.active_search.get_search_points in the
NumPy-stream mode and the restatement tests/search_host.py, both against the reference's recorded outputs
(tests/golden/search.npz, tools/make_search_golden.py); the restatement's philox mode as a sample of the same
distributions; the drop-in's ``search=True``.

Bounds: same-stream points equal the recorded ones bit for bit (found exact here; the project's bound for such points is
rtol 1e-13, tests/test_ais_gpu.py); the statistical checks at 5 standard errors of the analytic value with seeds fixed here.
"""
import types

import numpy as np
import pytest
import search_host as sh
from scipy import optimize, stats

import pyvbmc_amd
from pyvbmc_amd import _lib, active_search, dropin

POINT_CASES = ("a", "b", "c", "d", "e", "f")


def unbounded(case):
    """The case with infinite search bounds: no clamp, so every block is a plain sample of its source."""
    D = case.D
    case.optim_state["lb_search"] = np.full((1, D), -np.inf)
    case.optim_state["ub_search"] = np.full((1, D), np.inf)
    return case


# ---------------------------------------------------------------------------------------------- NumPy-stream mode
@pytest.mark.parametrize("name", POINT_CASES)
def test_numpy_mode_equals_the_reference(golden, name):
    c = sh.load_case(golden("search"), name)
    vp = sh.package_vp(c)  # (the constructor draws from np.random: before the seed)
    np.random.seed(c.np_seed)
    X, idx = active_search.get_search_points(c.number_of_points, c.optim_state, c.flog, vp, c.options, rng="numpy",
                                             device=False)
    assert X.shape == c.search_X.shape and idx.shape == c.idx_cache.shape
    np.testing.assert_array_equal(X, c.search_X)  # the same statements on the same stream: the same bits
    np.testing.assert_array_equal(idx, c.idx_cache)  # (NaN for every random row, the cache's indices in front)
    n_cached = int(np.sum(~np.isnan(idx)))
    assert n_cached == min(c.optim_state["cache"]["x_orig"].shape[0], int(np.ceil(c.number_of_points * c.options["cache_frac"])))
    assert np.all(np.isnan(idx[n_cached:]))
    if name == "c":
        assert X.shape[0] < c.number_of_points  # :709-710: the cache's size is subtracted, not the rows taken


@pytest.mark.parametrize("name", POINT_CASES)
def test_restatement_numpy_mode_equals_the_reference(golden, name):
    c = sh.load_case(golden("search"), name)
    np.random.seed(c.np_seed)
    X, idx = sh.points_numpy(c.number_of_points, c.optim_state, c.flog, c.mix, c.options)
    np.testing.assert_array_equal(X, c.search_X)
    np.testing.assert_array_equal(idx, c.idx_cache)


def test_fractions_above_one_raise(golden):
    c = sh.load_case(golden("search"), "g")
    assert c.raised
    vp = sh.package_vp(c)
    for mode, kw in (("numpy", dict(device=False)), ("philox", dict(seed=5))):
        np.random.seed(c.np_seed)
        if mode == "philox":  # the host plan raises before anything is drawn on a device
            with pytest.raises(ValueError):
                active_search.philox_plan(c.number_of_points, c.optim_state, c.flog, vp, c.options, 5)
        else:
            with pytest.raises(ValueError):
                active_search.get_search_points(c.number_of_points, c.optim_state, c.flog, vp, c.options, rng=mode, **kw)
    np.random.seed(c.np_seed)
    with pytest.raises(ValueError):
        sh.points_numpy(c.number_of_points, c.optim_state, c.flog, c.mix, c.options)
    with pytest.raises(ValueError):
        sh.points_philox(c.number_of_points, c.optim_state, c.flog, c.mix, c.options, 5)


def test_philox_plan_matches_the_restatement_layout(golden):
    """The mirror's host plan and the restatement agree on the sources, their rows, keys and parameters."""
    c = sh.load_case(golden("search"), "d")
    vp = sh.package_vp(c)
    sources, idx = active_search.philox_plan(c.number_of_points, c.optim_state, c.flog, vp, c.options, 77)
    X, idx_h, blocks = sh.points_philox(c.number_of_points, c.optim_state, c.flog, c.mix, c.options, 77)
    np.testing.assert_array_equal(idx, idx_h)
    assert [int(s[1]) for s in sources] == [b[1] for b in blocks.values()]
    assert sum(int(s[1]) for s in sources) == X.shape[0]
    names = list(blocks)
    for s, n in zip(sources, names):
        if s[0] == _lib.SRC_AFFINE:
            np.testing.assert_array_equal(s[2][0], blocks[n][2][0])
            np.testing.assert_array_equal(s[2][1], blocks[n][2][1])
        if n in active_search.SOURCES:
            assert s[4] == sh.source_key(77, active_search.SOURCES.index(n))


# ---------------------------------------------------------------------------------------------- philox mode: a sample
def check_gaussian_block(rows, mean, A, what):
    n = rows.shape[0]
    cov = A.T @ A
    se_mean = np.sqrt(np.diag(cov) / n)
    z = np.abs(rows.mean(axis=0) - mean) / se_mean
    assert np.all(z < 5), (what, "mean", z)
    emp = np.cov(rows, rowvar=False, bias=True).reshape(cov.shape)
    se_cov = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov**2) / n)
    zc = np.abs(emp - cov) / se_cov
    assert np.all(zc < 5), (what, "cov", zc)


def t_mixture_quantile(mix, j, q, df):
    scale = mix.lambd[j] * mix.sigma
    cdf = lambda x: float(np.sum(mix.w * stats.t.cdf((x - mix.mu[j]) / scale, df))) - q  # noqa: E731
    x = optimize.brentq(cdf, -1e3, 1e3, xtol=1e-13)
    return x, float(np.sum(mix.w * stats.t.pdf((x - mix.mu[j]) / scale, df) / scale))


@pytest.mark.parametrize("name, seed", [("a", 11), ("d", 12)])
def test_philox_mode_samples_the_sources(golden, name, seed):
    c = unbounded(sh.load_case(golden("search"), name, number_of_points=8192))
    # (a search cache as long as its share of 8192 rows: a shorter one shortens the output, :720)
    c.optim_state["search_cache"] = np.random.default_rng(3).standard_normal((1024, c.D))
    X, idx, blocks = sh.points_philox(c.number_of_points, c.optim_state, c.flog, c.mix, c.options, seed)
    assert X.shape == (8192, c.D) and np.all(np.isfinite(X)) and np.all(np.isnan(idx))
    mix = c.mix
    seen = set()
    for what, (r0, n, info) in blocks.items():
        rows = X[r0:r0 + n]
        if what == "mvn" or what.startswith("hpd"):
            check_gaussian_block(rows, info[0], info[1], what)
        elif what == "box":
            lb, ub = info
            check_gaussian_block(rows, lb, np.diag(ub - lb), what)
        elif what == "vp":
            mubar, cov = sh.mixture_ref.moments(mix, cov_flag=True)
            z = np.abs(rows.mean(axis=0) - np.ravel(mubar)) / np.sqrt(np.diag(cov) / n)
            assert np.all(z < 5), (what, z)
        elif what == "heavy":  # df = 3: infinite fourth moment, so quantiles instead of moments
            for j in range(c.D):
                (q1, f1), (q2, f2), (q3, f3) = (t_mixture_quantile(mix, j, q, 3.0) for q in (0.25, 0.5, 0.75))
                s1, s2, s3 = np.quantile(rows[:, j], (0.25, 0.5, 0.75))
                assert abs(s2 - q2) < 5 * np.sqrt(0.25 / n) / f2, (what, j, "median")
                var_iqr = (0.1875 / f1**2 + 0.1875 / f3**2 - 2 * 0.0625 / (f1 * f3)) / n
                assert abs((s3 - s1) - (q3 - q1)) < 5 * np.sqrt(var_iqr), (what, j, "iqr")
        else:
            continue
        seen.add(what[:3])
    assert {"mvn", "box", "vp", "hea"} <= seen and (name != "d" or "hpd" in seen)
    if name == "d":
        assert sum(k.startswith("hpd") for k in blocks) == 6 and blocks["search_cache"][1] > 0


def test_rank_deficient_hpd_covariances(golden):
    """N = 4 points in D = 3: HPD sets of 0 (fallback), 1, 2 and 3 points.  The draws are finite and stay in the span of
    their set: the part outside it is at most 1e-12 of the data's diameter."""
    c = unbounded(sh.load_case(golden("search"), "e", number_of_points=8192))
    X, idx, blocks = sh.points_philox(c.number_of_points, c.optim_state, c.flog, c.mix, c.options, 14)
    assert np.all(np.isfinite(X))
    Xd, yd = c.flog.X[c.flog.X_flag], c.flog.y[c.flog.X_flag]
    diam = float(np.max(np.amax(Xd, axis=0) - np.amin(Xd, axis=0)))
    sizes = set()
    for what, (r0, n, info) in blocks.items():
        if not what.startswith("hpd"):
            continue
        mean, A, frac = info
        S = sh.get_hpd(Xd, yd, frac)
        sizes.add(S.shape[0])
        if S.shape[0] == 0:  # the fallback: X[argmax y] and np.cov(X), full rank here
            np.testing.assert_array_equal(mean, Xd[np.argmax(yd)])
            continue
        dev = X[r0:r0 + n] - mean
        B = S - S.mean(axis=0)
        u, s, vt = np.linalg.svd(B, full_matrices=True)
        rank = int(np.sum(s > 1e-10 * max(s.max(), 1e-300)))
        out = dev @ vt[rank:].T  # components along the directions the set does not span
        print(what, "set of", S.shape[0], "rank", rank, "outside span / diameter:", float(np.max(np.abs(out))) / diam)
        assert np.max(np.abs(out)) <= 1e-12 * diam, what
    assert 0 in sizes and len(sizes) >= 3


# ---------------------------------------------------------------------------------------------- the drop-in
def test_patch_active_sampling_search_rebinds_and_restores():
    mod = types.ModuleType("standin_active_sample")
    ref_ais = lambda *a, **kw: "ref_ais"  # noqa: E731
    ref_gsp = lambda *a, **kw: "ref_gsp"  # noqa: E731
    mod.active_importance_sampling, mod._get_search_points = ref_ais, ref_gsp
    pyvbmc_amd.patch_active_sampling(mod)  # the default leaves the search points alone
    assert mod._get_search_points is ref_gsp and mod.active_importance_sampling is not ref_ais
    pyvbmc_amd.patch_active_sampling(mod, search=True)
    assert mod._get_search_points.__wrapped__ is active_search.get_search_points
    assert mod.active_importance_sampling is not ref_ais
    pyvbmc_amd.patch_active_sampling(mod, search=True)  # idempotent: the saved function is still the reference's
    pyvbmc_amd.unpatch_active_sampling(mod)
    assert mod._get_search_points is ref_gsp and mod.active_importance_sampling is ref_ais
    assert not hasattr(mod, dropin._SAVED_GSP) and not hasattr(mod, dropin._SAVED_AIS)


def test_unsupported_shape_goes_back_to_the_reference_function(monkeypatch):
    log = []
    mod = types.ModuleType("standin_active_sample")

    def ref_gsp(*a, **kw):
        log.append((a, dict(kw)))
        return "ref"

    mod._get_search_points = ref_gsp
    mod.active_importance_sampling = lambda *a, **kw: None

    def raising(*a, **kw):
        raise _lib.UnsupportedShape("acquisition search: D=40 > 32 not supported")

    monkeypatch.setattr(dropin, "_gsp_mirror", raising)
    pyvbmc_amd.patch_active_sampling(mod, search=True)
    try:
        assert mod._get_search_points(300, "optim_state", "logger", "vp", "options", rng="philox", seed=1, device=True) == "ref"
        assert log == [((300, "optim_state", "logger", "vp", "options"), {})]  # none of the mirror's keyword-only extras
    finally:
        pyvbmc_amd.unpatch_active_sampling(mod)
    assert mod._get_search_points is ref_gsp


def test_philox_mode_refuses_d_above_32_before_drawing():
    D = 33
    state = {"ub_search": np.full((1, D), np.inf), "lb_search": np.full((1, D), -np.inf), "cache": {"x_orig": np.zeros((0, D))}}
    flog = types.SimpleNamespace(parameter_transformer=None)
    st = np.random.get_state()[1].copy()
    with pytest.raises(_lib.UnsupportedShape):
        active_search.get_search_points(300, state, flog, None, {}, rng="philox")
    assert np.array_equal(np.random.get_state()[1], st)  # (not even the seed was drawn)
