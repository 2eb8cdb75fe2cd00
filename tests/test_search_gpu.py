"""The acquisition search on the device (pyvbmc_amd/active_search.py, csrc/search.hip, csrc/api_search.hip) against the
NumPy restatement tests/search_host.py, against this package's own acquisition classes on the returned points, and --
for the ranking -- against ``np.argsort(kind="stable")`` of the device's own values.

Bounds: philox points rtol 1e-13, the transformed cache rows 1e-12 (the device transformer's bound,
tests/test_transform_gpu.py); acquisition values 1e-9 (tests/test_acquisition.py, tests/test_ais_gpu.py); the order,
the sorted points and the integer columns exactly.
"""
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import search_host as sh
from helpers import PlainGP

from oracle import acq_ref

pytestmark = pytest.mark.gpu

REALMAX = sys.float_info.max
CLOSED = {"AcqFcn": acq_ref.STD, "AcqFcnLog": acq_ref.LOG, "AcqFcnVanilla": acq_ref.VANILLA, "AcqFcnNoisy": acq_ref.NOISY}
# VIQR reads mcmc_samples as its number of importance points; IMIQR (no MCMC here) the other two
AIS_OPTIONS = {"AcqFcnVIQR": dict(active_importance_sampling_mcmc_samples=60),
               "AcqFcnIMIQR": dict(active_importance_sampling_mcmc_samples=0, active_importance_sampling_vp_samples=50,
                                   active_importance_sampling_box_samples=30)}


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


def the_case(golden, name, **kw):
    return sh.wide_case() if name == "wide" else sh.load_case(golden("search"), name, **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def full_set(res, options):
    """The search set in its own order: the chosen row (:337-342) put back where it was."""
    idx = int(res.order[0]) if options["search_cache_frac"] > 0 else int(np.argmin(res.acq_fast))
    return np.insert(res.X_search, idx, res.X_acq[0], axis=0), idx


def search_setup(case, ctx, S=2, acq_name="AcqFcnVIQR", length_mult=1.0):
    """Device-side arguments of ``search`` for a case, and the oracle objects of the restatement."""
    ogp, length, sn2_new = sh.gp_fixture(case, S, length_mult=length_mult)
    gp = PlainGP(ogp)
    gp._ctx = ctx
    gp.temporary_data["X_rescaled"] = ogp.X / length
    gp.temporary_data["sn2_new"] = sn2_new
    vp = sh.package_vp(case, ctx)
    y = case.flog.y[case.flog.X_flag]
    flog = SimpleNamespace(X=case.flog.X, y=case.flog.y, X_flag=case.flog.X_flag, parameter_transformer=case.pt,
                           y_max=float(np.max(y)))
    D = case.D
    state = dict(case.optim_state, integer_vars=None, gp_length_scale=length, tol_gp_var=1e-4,
                 variance_regularized_acq_fcn=False, lb_eps_orig=np.full(D, -7.5), ub_eps_orig=np.full(D, 8.5))
    options = dict(case.options, ns_search=case.number_of_points, **AIS_OPTIONS.get(acq_name, {}))
    return SimpleNamespace(ogp=ogp, gp=gp, vp=vp, flog=flog, state=state, options=options, length=length, sn2_new=sn2_new)


def check_rank(res, state, options, idx_cache_len):
    """order == the stable argsort of the device's own values; the stored cache and the row removal follow :337-349."""
    order = np.argsort(res.acq_fast, kind="stable")
    np.testing.assert_array_equal(res.order, order)
    X, idx = full_set(res, options)
    assert X.shape[0] == res.acq_fast.size and res.idx_cache.shape[0] == idx_cache_len - 1
    if options["search_cache_frac"] > 0:
        assert np.array_equal(bits(state["search_cache"]), bits(X[order]))  # sorted points == X_search[order], bit for bit
        assert np.array_equal(bits(res.X_acq[0]), bits(state["search_cache"][0]))
    return X, idx


# ---------------------------------------------------------------------------------------------- philox points
# Seeds under which no element of the restatement's points is a sum that cancels by more than a factor 100 (searched on
# the CPU, asserted below).  The device's normals are within 4.5 ulp of libm's (log_fast 1.93, sincospi_fast 1.7,
# profiles/fastmath_ulp.md, and libm's own 1), every product and sum after them is the same operation in the same
# order on both sides, so an element differs by at most 4.5 ulp times that factor: within rtol 1e-13 (450 ulp).
POINT_SEEDS = {"a": 112, "b": 292, "d": 49, "e": 33, "f": 2, "wide": 1}


def check_philox_points(ctx, c, seed, name, expect_clamped=True):
    """``get_search_points`` on the Philox streams against the restatement for one case and seed: the conditioning
    precondition, the index column, the rows at their two bounds, the clamp, reproducibility."""
    from pyvbmc_amd import active_search

    vp = sh.package_vp(c, ctx)
    detail = {}
    Xh, idxh, blocks = sh.points_philox(c.number_of_points, c.optim_state, c.flog, c.mix, c.options, seed, detail=detail)
    assert np.nanmax(detail["cond"]) <= 100
    X, idx = active_search.get_search_points(c.number_of_points, c.optim_state, c.flog, vp, c.options, rng="philox",
                                             seed=seed, ctx=ctx)
    assert X.shape == Xh.shape
    np.testing.assert_array_equal(idx, idxh)
    n_cache = blocks["cache"][1] if "cache" in blocks else 0
    rel = np.abs(X - Xh) / np.maximum(np.abs(Xh), 1e-300)
    print(name, "max rel: cache rows", float(rel[:n_cache].max()) if n_cache else 0.0, "other rows", float(rel[n_cache:].max()),
          {k: float(rel[v[0]:v[0] + v[1]].max()) for k, v in blocks.items() if v[1]})
    np.testing.assert_allclose(X[:n_cache], Xh[:n_cache], rtol=1e-12, atol=0)
    np.testing.assert_allclose(X[n_cache:], Xh[n_cache:], rtol=1e-13, atol=0)
    lb, ub = c.optim_state["lb_search"], c.optim_state["ub_search"]
    clamped = (Xh == lb) | (Xh == ub)
    assert np.array_equal(X[clamped], Xh[clamped]) and (not expect_clamped or clamped.any())
    assert np.all(X >= lb) and np.all(X <= ub)
    X2, _ = active_search.get_search_points(c.number_of_points, c.optim_state, c.flog, vp, c.options, rng="philox",
                                            seed=seed, ctx=ctx)
    assert np.array_equal(bits(X), bits(X2))  # a fixed seed is bit-reproducible
    X3, _ = active_search.get_search_points(c.number_of_points, c.optim_state, c.flog, vp, c.options, rng="philox",
                                            seed=seed + 1, ctx=ctx)
    assert not np.array_equal(X3[n_cache:], X[n_cache:])
    return float(rel[:n_cache].max()) if n_cache else 0.0, float(rel[n_cache:].max())


@pytest.mark.parametrize("name", list(POINT_SEEDS))
def test_philox_points_equal_the_restatement(ctx, golden, name):
    check_philox_points(ctx, the_case(golden, name), POINT_SEEDS[name], name, expect_clamped=name not in ("b",))


def test_d_above_32_is_an_unsupported_shape(ctx):
    from pyvbmc_amd import _lib, active_search

    D = 33
    state = {"ub_search": np.full((1, D), np.inf), "lb_search": np.full((1, D), -np.inf), "cache": {"x_orig": np.zeros((0, D))}}
    flog = SimpleNamespace(parameter_transformer=None)
    with pytest.raises(_lib.UnsupportedShape):
        active_search.get_search_points(300, state, flog, None, {}, rng="philox", ctx=ctx)
    with pytest.raises(_lib.UnsupportedShape):
        active_search.search("AcqFcnLog()", None, SimpleNamespace(_ctx=ctx), flog, state, {"ns_search": 300}, rng="philox")
    with pytest.raises(_lib.UnsupportedShape):  # the library's own check
        ctx.check(ctx._lib.vbmc_search_put(ctx._h, 1, D, _lib.ptr(np.zeros((1, D))), 0, 0))


# ---------------------------------------------------------------------------------------------- rounding and mask
def test_integer_rounding_and_hard_bound_mask(ctx, golden):
    from pyvbmc_amd import active_search

    c = the_case(golden, "b")  # logit transformer on [-10, 10], a 5-row cache
    s = search_setup(c, ctx)
    integer_vars = np.array([False, True, False])
    s.state["integer_vars"] = integer_vars
    seed = POINT_SEEDS["b"]
    Xh, idxh, _ = sh.points_philox(c.number_of_points, c.optim_state, c.flog, c.mix, c.options, seed)
    Xr, pre = sh.real2int(Xh, c.pt, integer_vars, return_pre=True)
    # the inputs stay clear of the discontinuities
    assert np.min(np.abs(pre - np.floor(pre) - 0.5)) > 1e-9
    Xo = c.pt.inverse(Xr)
    width = s.state["ub_eps_orig"] - s.state["lb_eps_orig"]
    assert np.min(np.abs(Xo - s.state["lb_eps_orig"]) / width) > 1e-9 and np.min(np.abs(Xo - s.state["ub_eps_orig"]) / width) > 1e-9
    mask = sh.hard_bound_mask(Xr, c.pt, s.state)
    assert 0 < mask.sum() < mask.size  # the bounds cut off part of the set
    res = active_search.search("AcqFcnLog()", s.gp, s.vp, s.flog, s.state, s.options, rng="philox", seed=seed, ctx=ctx)
    X, idx = check_rank(res, s.state, s.options, idxh.size)
    # integer columns: whole numbers in the original space, equal to the restatement's; the others untouched
    assert np.array_equal(np.around(c.pt.inverse(X)[:, 1]), np.around(Xo[:, 1]))
    np.testing.assert_allclose(X[:, 1], Xr[:, 1], rtol=1e-12, atol=0)
    np.testing.assert_allclose(X[5:, [0, 2]], Xr[5:, [0, 2]], rtol=1e-13, atol=0)
    np.testing.assert_allclose(X[:5, [0, 2]], Xr[:5, [0, 2]], rtol=1e-12, atol=0)
    assert len(np.unique(X[:, 1])) <= 21
    np.testing.assert_array_equal(np.isposinf(res.acq_fast), mask)
    assert np.all(res.acq_fast[res.order[-int(mask.sum()):]] == np.inf)


def check_integer_rounding(ctx, c, int_dims, seed):
    """Integer dimensions ``int_dims`` of a case through both entry points: the fill of the Philox sources and
    ``vbmc_search_put`` of host-drawn points."""
    from pyvbmc_amd import _lib, active_search

    vp = sh.package_vp(c, ctx)
    D = c.D
    integer_vars = np.zeros(D, dtype=bool)
    integer_vars[list(int_dims)] = True
    int_bits = active_search._int_bits(integer_vars, D)
    assert int_bits == sum(1 << d for d in set(int_dims))
    Xh, _, blocks = sh.points_philox(c.number_of_points, c.optim_state, c.flog, c.mix, c.options, seed)
    Xr, pre = sh.real2int(Xh, c.pt, integer_vars, return_pre=True)
    assert np.min(np.abs(pre - np.floor(pre) - 0.5)) > 1e-9  # clear of the rounding's discontinuities
    sources, _ = active_search.philox_plan(c.number_of_points, c.optim_state, c.flog, vp, c.options, seed)
    active_search.upload_vp(vp, ctx)
    use_xf = active_search._xf_flag(c.pt, ctx, D)
    assert use_xf == 1
    X = active_search._fill(ctx, D, sources, c.optim_state["lb_search"], c.optim_state["ub_search"], int_bits, use_xf, True)
    n_cache = blocks["cache"][1]
    assert np.array_equal(np.around(c.pt.inverse(X)[:, integer_vars]), np.around(c.pt.inverse(Xr)[:, integer_vars]))
    np.testing.assert_allclose(X[:, integer_vars], Xr[:, integer_vars], rtol=1e-12, atol=0)
    np.testing.assert_allclose(X[n_cache:, ~integer_vars], Xr[n_cache:, ~integer_vars], rtol=1e-13, atol=0)
    np.testing.assert_allclose(X[:n_cache, ~integer_vars], Xr[:n_cache, ~integer_vars], rtol=1e-12, atol=0)
    assert not np.array_equal(X[:, D - 1], Xh[:, D - 1])  # the last dimension was rounded
    # host-drawn points take the same rounding: vbmc_search_put accepts the mask, and the fill of one copy source (what put
    # is, with a read-back) rounds the integer columns and leaves the others as they came
    active_search.put_points(ctx, Xh, int_bits, use_xf)
    inf = np.full((1, D), np.inf)
    Xp = active_search._fill(ctx, D, [(_lib.SRC_COPY, Xh.shape[0], Xh, 0.0, 0)], -inf, inf, int_bits, use_xf, True)
    np.testing.assert_allclose(Xp[:, integer_vars], Xr[:, integer_vars], rtol=1e-12, atol=0)
    assert np.array_equal(bits(Xp[:, ~integer_vars]), bits(Xh[:, ~integer_vars]))


def test_integer_rounding_at_d32(ctx):
    """D = 32, the widest shape, with integer dimensions 0, 17 and 31 (the mask's last bit), through both entry points."""
    from pyvbmc_amd import _lib

    check_integer_rounding(ctx, sh.wide_case(), (0, 17, 31), POINT_SEEDS["wide"])
    for bad in (1 << 5,):  # a bit at or above D is an argument error, at D < 32 only
        with pytest.raises(ValueError):
            ctx.check(ctx._lib.vbmc_search_put(ctx._h, 1, 5, _lib.ptr(np.zeros((1, 5))), bad, 0))


# ---------------------------------------------------------------------------------------------- values
def eval_both(acq_name, s, c, X):
    """The restatement's and the package's own acquisition values at the returned points."""
    from pyvbmc_amd import acquisition

    if acq_name in CLOSED:
        host = sh.acq_values(CLOSED[acq_name], X, s.ogp, c.mix, s.flog.y_max, s.state, c.pt, s.gp.temporary_data["X_rescaled"],
                             s.sn2_new)
        own = getattr(acquisition, acq_name)()(X.copy(), s.gp, s.vp, s.flog, s.state)
    else:
        ais = s.state["active_importance_sampling"]
        obj = getattr(acquisition, acq_name)()
        host = sh.acq_values("viqr" if acq_name == "AcqFcnVIQR" else "imiqr", X, s.ogp, c.mix, 0.0, s.state, c.pt,
                             s.gp.temporary_data["X_rescaled"], s.sn2_new, ais=ais, u=obj.u)
        own = obj(X.copy(), s.gp, s.vp, s.flog, s.state)
    return host, own


def close(a, b, tol, what):
    inf = np.isinf(b)
    assert np.array_equal(np.isinf(a), inf), what
    assert np.array_equal(a[inf], b[inf]), what
    err = float(np.max(np.abs(a[~inf] - b[~inf]) / np.maximum(1.0, np.abs(b[~inf]))))
    print(what, f"{err:.2e}")
    assert err < tol, (what, err)
    return err


def check_values(ctx, c, s, acq_name, seed, what, cache_rtol=1e-12, points_conditioned=True):
    """One search of a prepared case: the ranking, the points, and the values against the restatement and against the
    package's own call at the returned points.  Returns (result, points, the two largest errors).
    ``points_conditioned``: the case and seed meet the conditioning precondition of check_philox_points, so the points are
    held to its relative bounds; without it (a case centred on zero, whose coordinates are sums that cancel) they are held
    to the same bounds relative to the largest coordinate."""
    from pyvbmc_amd import active_search

    res = active_search.search(acq_name + "()", s.gp, s.vp, s.flog, s.state, s.options, rng="philox", seed=seed, ctx=ctx)
    detail = {}
    Xh, idxh, blocks = sh.points_philox(c.number_of_points, c.optim_state, c.flog, c.mix, c.options, seed, detail=detail)
    assert res.acq_fast.shape == (c.number_of_points,)
    X, idx = check_rank(res, s.state, s.options, idxh.size)
    n_cache = blocks["cache"][1] if "cache" in blocks else 0
    scale = 0.0 if points_conditioned else float(np.max(np.abs(Xh)))
    if scale:  # the terms an element is added up from stay within a factor 100 of the largest coordinate
        assert np.nanmax(detail["cond"] * np.abs(detail["raw"])) <= 100 * scale
    np.testing.assert_allclose(X[:n_cache], Xh[:n_cache], rtol=0.0 if scale else cache_rtol, atol=cache_rtol * scale)
    np.testing.assert_allclose(X[n_cache:], Xh[n_cache:], rtol=0.0 if scale else 1e-13, atol=1e-13 * scale)
    assert ("active_importance_sampling" in s.state) == (acq_name in ("AcqFcnVIQR", "AcqFcnIMIQR"))
    host, own = eval_both(acq_name, s, c, X)
    e_own = close(res.acq_fast, own, 1e-9, f"{what} vs the package's own call")
    e_host = close(res.acq_fast, host, 1e-9, f"{what} vs the restatement")
    assert np.isposinf(res.acq_fast).any() and np.isfinite(res.acq_fast).any()
    return res, X, (e_own, e_host)


@pytest.mark.parametrize("reg", [False, True])
@pytest.mark.parametrize("acq_name", list(CLOSED) + ["AcqFcnVIQR", "AcqFcnIMIQR"])
def test_values_equal_the_restatement_and_the_package(ctx, golden, acq_name, reg):
    c = the_case(golden, "d")
    s = search_setup(c, ctx, acq_name=acq_name)
    s.state["variance_regularized_acq_fcn"] = reg
    s.state["tol_gp_var"] = 0.05  # (above the predictive variance near the training points: the penalty acts)
    seed = POINT_SEEDS["d"]  # (the points are compared too: a seed of the conditioning precondition above)
    res, _, _ = check_values(ctx, c, s, acq_name, seed, f"{acq_name} reg={reg}", cache_rtol=1e-13)
    assert res.acq_fast.shape == (300,)


# ---------------------------------------------------------------------------------------------- ranking
@pytest.mark.parametrize("M", [300, 8192, 8229])
def test_ranking(ctx, golden, M):
    """M = 300: padding to a power of two; 8192: one full LDS chunk; 8229: two chunks and a global pass.  The values hold
    exact ties (the +inf block of the hard bounds), -realmax and NaN (crafted below)."""
    from pyvbmc_amd import _lib, active_search

    c = the_case(golden, "d", number_of_points=M)
    c.optim_state["search_cache"] = np.random.default_rng(8).standard_normal((M // 8 + 1, c.D))
    s = search_setup(c, ctx)
    res = active_search.search("AcqFcnVIQR()", s.gp, s.vp, s.flog, s.state, s.options, rng="philox", seed=31, ctx=ctx)
    assert res.order.shape == (M,) and np.isposinf(res.acq_fast).sum() > 1
    X, idx = check_rank(res, s.state, s.options, M)
    assert np.isnan(res.idx_cache_acq)

    # a second search whose search cache is the first one's output: the copy source
    first = s.state["search_cache"].copy()
    n_sc = round(c.options["search_cache_frac"] * M)
    res2 = active_search.search("AcqFcnVIQR()", s.gp, s.vp, s.flog, s.state, s.options, rng="philox", seed=32, ctx=ctx)
    X2, _ = check_rank(res2, s.state, s.options, M)
    lb, ub = c.optim_state["lb_search"], c.optim_state["ub_search"]
    assert np.array_equal(bits(X2[:n_sc]), bits(np.minimum(np.maximum(first[:n_sc], lb), ub)))

    # without a search cache share nothing is stored, and the first index is the argmin
    opts0 = dict(s.options, search_cache_frac=0.0)
    state0 = {k: v for k, v in s.state.items() if k != "search_cache"}
    res0 = active_search.search("AcqFcnLog()", s.gp, s.vp, s.flog, state0, opts0, rng="philox", seed=33, ctx=ctx)
    check_rank(res0, state0, opts0, M)
    assert "search_cache" not in state0

    # crafted values.  A NaN coordinate in a row inside the hard bounds: the closed forms clamp with fmax, which turns the
    # NaN into -realmax, the smallest value there is.  A NaN importance weight (IMIQR adds ln_weights to every term):
    # every value inside the hard bounds is NaN, ranked behind the +inf block, ties in row order.
    from pyvbmc_amd.acquisition import AcqFcnIMIQR

    r = int(np.flatnonzero(np.isfinite(res.acq_fast))[3])
    Xn = X.copy()
    Xn[r, 0] = np.nan
    noise = (s.gp.temporary_data["X_rescaled"], s.sn2_new, s.length)
    active_search.put_points(ctx, Xn)
    ais = dict(s.state["active_importance_sampling"])
    ais["ln_weights"] = ais["ln_weights"].copy()
    ais["ln_weights"][0, 2] = np.nan
    imiqr = AcqFcnIMIQR()
    imiqr._upload_state(s.gp, ais, ctx)
    for kind in (acq_ref.LOG, _lib.ACQ_IS):
        acq, order, Xs = active_search.evaluate_resident(ctx, M, c.D, kind, s.flog.y_max, 0.0, float(imiqr.u), noise, 1,
                                                         s.state["lb_eps_orig"], s.state["ub_eps_orig"])
        n_inf = int(np.isposinf(acq).sum())
        assert n_inf > 1
        ref = np.argsort(acq, kind="stable")
        np.testing.assert_array_equal(order, ref)
        assert np.array_equal(bits(Xs), bits(Xn[ref]))
        if kind == acq_ref.LOG:
            assert acq[r] == -REALMAX and order[0] == r and not np.isnan(acq).any()
        else:
            assert np.isnan(acq).sum() == M - n_inf and np.all(np.isposinf(acq[order[:n_inf]])) and np.all(np.diff(order[n_inf:]) > 0)


# ---------------------------------------------------------------------------------------------- NumPy stream through the device
def test_numpy_stream_points_through_the_device(ctx, golden):
    from pyvbmc_amd import active_search

    c = the_case(golden, "b")
    s = search_setup(c, ctx)
    np.random.seed(c.np_seed)
    res = active_search.search("AcqFcnLog()", s.gp, s.vp, s.flog, s.state, s.options, rng="numpy", ctx=ctx)
    X, idx = check_rank(res, s.state, s.options, c.idx_cache.size)
    np.testing.assert_allclose(X[:5], c.search_X[:5], rtol=1e-12, atol=0)  # the cache rows: the device transformer
    np.testing.assert_allclose(X[5:], c.search_X[5:], rtol=1e-13, atol=0)
    full_idx = np.insert(res.idx_cache, idx, res.idx_cache_acq)
    np.testing.assert_array_equal(full_idx, c.idx_cache)
    host, own = eval_both("AcqFcnLog", s, c, X)
    close(res.acq_fast, own, 1e-9, "numpy stream vs the package's own call")
