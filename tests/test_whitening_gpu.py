"""GPU tests of input warping (csrc/warp.hip through pyvbmc_amd/whitening.py) against the NumPy statement of
tests/whitening_host.py and the reference's stored outputs (tests/golden/whitening.npz).

Tolerance.  One transform is held to 1e-12 in this project (tests/test_transform_gpu.py); the composed warp and its
reductions stack two transforms, a mean and a cancelling standard deviation, so the bound is measured, not guessed: the
statement is evaluated in ``np.longdouble`` (the truth) and in float64, and per quantity

    |device - truth| / max|truth|  <=  max(8 * |float64 statement - truth| / max|truth|,  1e-12)

the margin and the method of tests/test_gp_illcond_gpu.py.  Every check prints a table row; profiles/warp_parity.md holds
the rows of one run.
"""
import types

import numpy as np
import pytest

import whitening_host as wh

pytestmark = pytest.mark.gpu

FROM_OLD, FROM_ORIG, IN_NEW = 0, 1, 2
FLOOR = 1e-12
N_BOX = 1000  # box draws of the entry-point parity tests (the truth is long double: kept small)


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


def rel(a, truth):
    truth = np.asarray(truth, dtype=wh.LD)
    a = np.asarray(a).astype(wh.LD)
    assert a.shape == truth.shape, f"shapes {a.shape} {truth.shape}"
    if not truth.size:
        return 0.0
    scale = np.max(np.abs(truth))
    return float(np.max(np.abs(a - truth)) / (scale if scale > 0 else 1))  # (an all-zero quantity: absolute)


def check(what, dev, f64, truth):
    """The device value within max(8 e64, 1e-12) of the truth (relative to the truth's largest entry)."""
    e64, edev = rel(f64, truth), rel(dev, truth)
    bound = max(8 * e64, FLOOR)
    print(f"| {what} | {e64:.1e} | {bound:.1e} | {edev:.1e} | {edev / bound:.2f} |")
    assert edev <= bound, f"{what}: device error {edev:.2e} > bound {bound:.2e} (float64 statement {e64:.2e})"


def check_golden(what, dev, gold, f64, truth):
    """The device value within the same bound of the reference's stored value."""
    e64, edev = rel(f64, truth), rel(dev, gold)
    bound = max(8 * e64, FLOOR)
    print(f"| {what} (vs golden) | {e64:.1e} | {bound:.1e} | {edev:.1e} | {edev / bound:.2f} |")
    assert edev <= bound, f"{what}: |device - golden| {edev:.2e} > bound {bound:.2e} (float64 statement {e64:.2e})"


_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def route(ctx, c, new=None):
    from pyvbmc_amd import whitening

    return whitening._DeviceRoute(c.old.as_object(), (new or c.new).as_object(), ctx)


def both(c):
    """(old, new) of a case in float64 and in long double."""
    return (c.old, c.new), (c.old.astype(wh.LD), c.new.astype(wh.LD))


def base_points(c):
    """Points in the old inference space: the mixture centres and the GP's training inputs."""
    return np.ascontiguousarray(np.vstack([c.mu.T, c.gp_X]))


# ---- the four entry points against the statement ---------------------------------------------------------------------
def check_points(ctx, c, name):
    """vbmc_warp_points from the three sources on a case's base points and evaluated original-space points."""
    (o, n), (ol, nl) = both(c)
    x = base_points(c)
    y, lj_new, lj_old = route(ctx, c).points(x, FROM_OLD, True, True, True)
    tw = nl.forward(ol.inverse(x))
    fw = n.forward(o.inverse(x))
    check(f"{name} points y (old)", y, fw, tw)
    check(f"{name} points lj_new", lj_new, n.log_abs_det(fw), nl.log_abs_det(tw))
    check(f"{name} points lj_old", lj_old, o.log_abs_det(x), ol.log_abs_det(x))
    xo = c.X_orig[c.X_flag]
    y2, lj2, _ = route(ctx, c).points(xo, FROM_ORIG, True, True, False)
    check(f"{name} points y (orig)", y2, n.forward(xo), nl.forward(xo))
    check(f"{name} points lj_new (orig)", lj2, n.log_abs_det(n.forward(xo)), nl.log_abs_det(nl.forward(xo)))
    y3, lj3, _ = route(ctx, c).points(fw, IN_NEW, True, True, False)
    assert np.array_equal(y3, fw)
    check(f"{name} points lj_new (in new)", lj3, n.log_abs_det(fw), nl.log_abs_det(fw))


@pytest.mark.parametrize("name", wh.CASES)
def test_warp_points(ctx, name):
    check_points(ctx, wh.load_case(name), name)


def check_unscent(ctx, c, name):
    """vbmc_warp_unscent on a case's mixture: mean, sd and sigma points; one row of sigma against the tiled form; the
    reference's stored values where the case has them."""
    (o, n), (ol, nl) = both(c)
    x, sigma = c.mu.T, (c.lambd * c.sigma).T
    mean, sd, pts = route(ctx, c).unscent(x, sigma, want_pts=True)
    f, t = wh.unscent_warp(o, n, x, sigma), wh.unscent_warp(ol, nl, x, sigma)
    for what, d, a, b in zip(("mean", "sd", "points"), (mean, sd, pts), f, t):
        check(f"{name} unscent {what}", d, a, b)
    # one row of sigma is broadcast in the kernel: the same bits as the tiled form
    m1, s1, _ = route(ctx, c).unscent(x, sigma[:1])
    m2, s2, _ = route(ctx, c).unscent(x, np.tile(sigma[:1], (c.K, 1)))
    assert np.array_equal(m1, m2) and np.array_equal(s1, s2)
    f1, t1 = wh.unscent_warp(o, n, x, sigma[:1]), wh.unscent_warp(ol, nl, x, sigma[:1])
    check(f"{name} unscent mean (one row of sigma)", m1, f1[0], t1[0])
    check(f"{name} unscent sd (one row of sigma)", s1, f1[1], t1[1])
    if hasattr(c, "un_mean"):  # against the reference's stored values at the same bound
        check_golden(f"{name} unscent mean", mean, c.un_mean, f[0], t[0])
        check_golden(f"{name} unscent sd", sd, c.un_sd, f[1], t[1])


@pytest.mark.parametrize("name", wh.CASES)
def test_warp_unscent(ctx, name):
    c = wh.load_case(name)
    assert hasattr(c, "un_mean") and hasattr(c, "un_sd")
    check_unscent(ctx, c, name)


def test_unscent_matlab_example(ctx):
    from pyvbmc_amd import whitening

    g = wh.golden()
    old, new = wh.Xf.from_golden(g, "ua_old_"), wh.Xf.from_golden(g, "ua_new_")
    mean, sd, pts = whitening.unscent_warp(whitening.Warp(old.as_object(), new.as_object()), g["ua_x"], g["ua_sigma"],
                                           ctx=ctx)
    t = wh.unscent_warp(old.astype(wh.LD), new.astype(wh.LD), g["ua_x"], g["ua_sigma"])
    for what, d, a, b in zip(("mean", "sd", "points"), (mean, sd, pts), (g["ua_mean"], g["ua_sd"], g["ua_pts"]), t):
        check(f"matlab example unscent {what}", d, a, b)
    assert np.all(np.isclose(mean, g["matlab_ua_mean"], atol=1e-4)) and np.all(np.isclose(sd, g["matlab_ua_sd"], atol=1e-4))
    assert np.all(np.isclose(pts, g["matlab_ua_pts"], atol=1e-4))


def gp_terms(old, new, X, hyp):
    """The statement of vbmc_warp_gp's outputs in the transformers' dtype."""
    dt = new.dtype
    D, N = X.shape[1], X.shape[0]
    logell = np.stack([np.sum(np.log(wh.unscent_warp(old, new, X, np.exp(np.asarray(h[:D], dtype=dt)))[1]), axis=0) / dt(N)
                       for h in hyp])
    dy = np.sum(new.log_abs_det(wh.warp(old, new, X))) / dt(N)
    dy_old = np.sum(old.log_abs_det(X)) / dt(N)
    return logell, dy, dy_old


def check_gp(ctx, c, name):
    """vbmc_warp_gp on a case's training inputs and hyper-parameter samples, and its reproducibility."""
    (o, n), (ol, nl) = both(c)
    logell, dy, dy_old = route(ctx, c).gp(c.gp_X, c.hyp)
    f, t = gp_terms(o, n, c.gp_X, c.hyp), gp_terms(ol, nl, c.gp_X, c.hyp)
    assert logell.shape == (c.S, c.D)
    check(f"{name} gp log ell", logell, f[0], t[0])
    check(f"{name} gp mean dy", np.array([dy]), np.array([f[1]]), np.array([t[1]]))
    check(f"{name} gp mean dy_old", np.array([dy_old]), np.array([f[2]]), np.array([t[2]]))
    again = route(ctx, c).gp(c.gp_X, c.hyp)
    assert np.array_equal(logell, again[0]) and dy == again[1] and dy_old == again[2]


@pytest.mark.parametrize("name", wh.CASES)
def test_warp_gp(ctx, name):
    check_gp(ctx, wh.load_case(name), name)


def box_statement(old, new, u, lo, hi, source, mode):
    dt = new.dtype
    x = np.asarray(u, dtype=dt) * (np.ravel(hi).astype(dt) - np.ravel(lo).astype(dt)) + np.ravel(lo).astype(dt)
    y = new.forward(x) if source == FROM_ORIG else wh.warp(old, new, x)
    if mode == 1:
        return np.stack([np.min(y, axis=0), np.max(y, axis=0)])
    return np.stack([wh.quantile_linear(y, 0.05), wh.quantile_linear(y, 0.95)])


def check_box(ctx, c, name):
    """vbmc_warp_box on uploaded uniforms: the plausible box's quantiles, the search box's extremes and quantiles."""
    (o, n), (ol, nl) = both(c)
    u = np.random.RandomState(11).rand(N_BOX, c.D)
    for what, lo, hi, source, mode in (("plausible quantiles", c.plb_orig, c.pub_orig, FROM_ORIG, 0),
                                       ("search min / max", c.lb_search, c.ub_search, FROM_OLD, 1),
                                       ("search quantiles", c.lb_search, c.ub_search, FROM_OLD, 0)):
        out = route(ctx, c).box(u, lo, hi, source, mode)
        assert out.shape == (2, c.D)
        check(f"{name} box {what}", out, box_statement(o, n, u, lo, hi, source, mode),
              box_statement(ol, nl, u, lo, hi, source, mode))


@pytest.mark.parametrize("name", wh.CASES)
def test_warp_box(ctx, name):
    check_box(ctx, wh.load_case(name), name)


# ---- order statistics ------------------------------------------------------------------------------------------------
def ulps(a, b):
    return np.max(np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b))))


@pytest.mark.parametrize("n", [1000, 20000, 100000])  # one sort chunk; three chunks (the merge); the reference's size
def test_box_quantiles_are_exact_order_statistics(ctx, n):
    c = wh.load_case("b")
    r = route(ctx, c)
    u = np.random.RandomState(100 + n % 97).rand(n, c.D)
    lo, hi = np.ravel(c.plb_orig), np.ravel(c.pub_orig)
    q, srt = r.box(u, lo, hi, FROM_ORIG, 0, want_sorted=True)
    y = r.points(u * (hi - lo) + lo, FROM_ORIG)[0]  # the transformed values themselves
    assert srt.shape == (c.D, n) and np.array_equal(srt, np.sort(y, axis=0).T)
    want = np.quantile(y, [0.05, 0.95], axis=0)
    assert ulps(q, want) <= 2, f"quantiles differ by {ulps(q, want)} ulp"
    assert np.array_equal(q, r.box(u, lo, hi, FROM_ORIG, 0))


def test_box_min_max_is_numpys(ctx):
    c = wh.load_case("c")
    r = route(ctx, c)
    u = np.random.RandomState(5).rand(1000, c.D)
    lo, hi = np.ravel(c.lb_search), np.ravel(c.ub_search)
    mm = r.box(u, lo, hi, FROM_OLD, 1)
    y = r.points(u * (hi - lo) + lo, FROM_OLD)[0]
    assert np.array_equal(mm, np.stack([np.min(y, axis=0), np.max(y, axis=0)]))


def check_box_philox(r, D, lo, hi, n, two_sample=True):
    """The box draws of Philox stream 9 through ``vbmc_warp_box``: reproducible and seed-dependent, the extremes of the
    min / max mode those of the sorted columns, and -- draw by draw -- the uniforms of the restatement (wh.box_uniforms)
    uploaded instead give the same bits in every dimension.  ``two_sample``: also the quantiles within sampling error of
    a NumPy-stream sample's.  That comparison is between two independent samples, whose quantiles differ by N(0, 2 se^2)
    with se itself estimated from the 2 % of the sample around the quantile: it is sound at n = 1e5 over a few
    dimensions, not at n = 1000 (20 order statistics) over hundreds of comparisons, where the bit-exact restatement
    says more."""
    a, sa = r.box(None, lo, hi, FROM_ORIG, 0, n=n, seed=77, want_sorted=True)
    b = r.box(None, lo, hi, FROM_ORIG, 0, n=n, seed=77)
    other = r.box(None, lo, hi, FROM_ORIG, 0, n=n, seed=78)
    assert np.array_equal(a, b) and not np.array_equal(a, other)
    if two_sample:
        ref, s = r.box(np.random.RandomState(9).rand(n, D), lo, hi, FROM_ORIG, 0, want_sorted=True)
        # standard error of a sample quantile, sqrt(q (1 - q) / n) / f(x_q), the density from the sample's own order
        # statistics one percent either side of it
        for row, q in enumerate((0.05, 0.95)):
            i0, i1 = int((q - 0.01) * n), int((q + 0.01) * n)
            dens = 0.02 / (s[:, i1] - s[:, i0])
            se = np.sqrt(q * (1 - q) / n) / dens
            z = np.abs(a[row] - ref[row]) / se
            print(f"| philox quantile {q} | |difference| / standard error per dimension: {np.round(z, 2)} |")
            assert np.all(z <= 4), f"quantile {q}: {z} standard errors from the numpy-stream result"
    # min / max mode draws the same stream: its extremes bracket the quantiles
    mm = r.box(None, lo, hi, FROM_ORIG, 1, n=n, seed=77)
    assert np.array_equal(mm, np.stack([sa[:, 0], sa[:, -1]]))
    # the restated uniforms through the upload route: every dimension's sorted column, bit for bit
    up, su = r.box(wh.box_uniforms(n, D, 77), lo, hi, FROM_ORIG, 0, want_sorted=True)
    assert np.array_equal(su, sa) and np.array_equal(up, a)
    for d in range(D):
        assert len(np.unique(sa[d])) > n // 2  # (a dimension that was never drawn would be constant)


def test_box_philox(ctx):
    c = wh.load_case("b")
    check_box_philox(route(ctx, c), c.D, np.ravel(c.plb_orig), np.ravel(c.pub_orig), 100000)


# ---- end to end ------------------------------------------------------------------------------------------------------
def input_truth(name):
    return cached(("wi", name), lambda: (wh.run_warp_input(wh.load_case(name)),
                                         wh.run_warp_input(wh.load_case(name), wh.LD)))


@pytest.mark.parametrize("name", ["b", "c"])
def test_warp_input_end_to_end(ctx, name):
    from pyvbmc_amd import whitening

    c = wh.load_case(name)
    vp, state, flog, options, _ = wh.package_inputs(c)
    np.random.seed(int(c.np_seed))
    pt, st2, fl2, action = whitening.warp_input(vp, state, flog, options, ctx=ctx, rng="numpy")
    assert np.random.rand() == float(c.next_draw)
    # the whitening transform is the host's SVD: the reference's bits
    assert np.array_equal(pt.R_mat, c.new_R) and np.array_equal(pt.scale, c.new_scale)
    assert np.all(pt.mu == 0) and np.all(pt.delta == 1) and action == "rotoscale"
    (_, _, f), (_, _, t) = input_truth(name)
    for key in ("plb_tran", "pub_tran", "lb_search", "ub_search"):
        assert st2[key].shape == (1, c.D)
        check_golden(f"{name} warp_input {key}", st2[key], getattr(c, "out_" + key), getattr(f, key), getattr(t, key))
    check_golden(f"{name} warp_input X", fl2.X, c.out_X, f.X, t.X)
    check_golden(f"{name} warp_input y", fl2.y, c.out_y, f.y, t.y)
    cache = np.reshape(st2["search_cache"], (-1, c.D))
    check_golden(f"{name} warp_input search cache", cache, c.out_search_cache, f.search_cache, t.search_cache)
    assert cache.shape[0] == c.search_cache.shape[0]
    assert st2["recompute_var_post"] is True and st2["skip_active_sampling"] is True
    assert st2["warping_count"] == int(c.out_warping_count) == int(c.warping_count) + 1
    assert st2["last_warping"] == st2["last_successful_warping"] == int(c.iter) == int(c.out_last_warping)
    assert st2["run_mean"] == [] and st2["run_cov"] == [] and np.isnan(st2["last_run_avg"])
    assert fl2.parameter_transformer is pt and flog.parameter_transformer is not pt
    assert np.array_equal(flog.X, c.X) and state["warping_count"] == int(c.warping_count)  # deep copies


@pytest.mark.parametrize("name", ["b", "c"])
def test_warp_input_philox_route(ctx, name):
    from pyvbmc_amd import whitening

    c = wh.load_case(name)
    vp, state, flog, options, _ = wh.package_inputs(c)
    before = np.random.get_state()[1].copy()
    a = whitening.warp_input(vp, state, flog, options, ctx=ctx, rng="philox", seed=5)
    b = whitening.warp_input(vp, state, flog, options, ctx=ctx, rng="philox", seed=5)
    assert np.array_equal(np.random.get_state()[1], before)  # a given seed leaves NumPy's stream alone
    # another sample of the same boxes.  A quantile of 1e5 draws moves by ~1e-3 of the span between samples; the extreme
    # of 1000 draws of a rotated D = 3 box sits in a corner that a fraction ~1000^(-1/3) of the span deep holds one draw
    for keys, tol in ((("plb_tran", "pub_tran"), 0.02), (("lb_search", "ub_search"), 0.5)):
        span = np.max(getattr(c, "out_" + keys[1]) - getattr(c, "out_" + keys[0]))
        for key in keys:
            assert np.array_equal(a[1][key], b[1][key])
            assert np.max(np.abs(a[1][key] - getattr(c, "out_" + key))) <= tol * span, key
    assert np.array_equal(a[2].X, b[2].X)


@pytest.mark.parametrize("name", ["b", "c"])
def test_warp_gp_and_vp_end_to_end(ctx, name):
    from pyvbmc_amd import whitening

    c = wh.load_case(name)
    vp, state, _, _, gp = wh.package_inputs(c)
    vbmc = types.SimpleNamespace(D=c.D, optim_state=state)
    vp2, hyp = whitening.warp_gp_and_vp(c.new.as_object(), gp, vp, vbmc, ctx=ctx)
    t = cached(("gv", name), lambda: wh.run_warp_gp_and_vp(c, wh.LD))
    f = wh.run_warp_gp_and_vp(c)
    assert hyp.shape == (c.S, c.hyp.shape[1])
    for what, d, gold, f64, truth in zip(("hyp_warped", "mu", "sigma", "lambd", "w"),
                                         (hyp, vp2.mu, vp2.sigma, vp2.lambd, vp2.w),
                                         (c.hyp_warped, c.vp_mu, c.vp_sigma, c.vp_lambd, c.vp_w), f, t):
        check_golden(f"{name} warp_gp_and_vp {what}", d, gold, f64, truth)
    assert abs(np.sum(vp2.w) - 1) <= 2e-16 and vp2 is not vp
    vp3, hyp3 = whitening.warp_gp_and_vp(c.new.as_object(), gp, vp, vbmc, ctx=ctx)
    assert np.array_equal(hyp, hyp3) and np.array_equal(vp2.mu, vp3.mu) and np.array_equal(vp2.w, vp3.w)
    assert np.array_equal(vp2.sigma, vp3.sigma) and np.array_equal(vp2.lambd, vp3.lambd)


# ---- refusals --------------------------------------------------------------------------------------------------------
class RecordingLib:
    def __init__(self, lib):
        self._lib_real, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib_real, name)


def test_d33_is_refused_before_a_launch(ctx):
    from pyvbmc_amd import _lib, whitening
    from transform_host import RefShapedTransformer

    D = 33
    pt = RefShapedTransformer(np.zeros(D), np.full(D, -np.inf), np.full(D, np.inf), np.zeros(D), np.ones(D))
    real = ctx._lib
    ctx._lib = RecordingLib(real)
    try:
        with pytest.raises(_lib.UnsupportedShape):
            whitening.unscent_warp(whitening.Warp(pt, pt), np.zeros((2, D)), np.ones((1, D)), ctx=ctx)
        assert ctx._lib.names == []  # refused in Python: the library was not called
    finally:
        ctx._lib = real
    # and the library refuses it itself
    x, o1, o2 = np.zeros((2, D)), np.empty((2, D)), np.empty(2)
    lib, h = ctx._lib, ctx._h
    rcs = [lib.vbmc_warp_points(h, D, 2, 0, _lib.ptr(x), _lib.ptr(o1), None, None),
           lib.vbmc_warp_unscent(h, D, 2, _lib.ptr(x), 1, _lib.ptr(x), _lib.ptr(o1), _lib.ptr(o1.copy()), None),
           lib.vbmc_warp_gp(h, D, 2, 1, D + 3, _lib.ptr(x), _lib.ptr(np.zeros((1, D + 3))), _lib.ptr(np.empty((1, D))), None,
                            None),
           lib.vbmc_warp_box(h, D, 2, 1, _lib.ptr(o2), _lib.ptr(o2), None, 0, 0, _lib.ptr(np.empty((2, D))), None)]
    assert rcs == [_lib.E_UNSUP] * 4
    with pytest.raises(_lib.UnsupportedShape):
        ctx.check(rcs[0])


def test_no_points_no_launch(ctx):
    c = wh.load_case("b")
    y, lj, _ = route(ctx, c).points(np.zeros((0, c.D)), FROM_OLD, True, True, False)
    assert y.shape == (0, c.D) and lj.shape == (0,)
    # (nothing is needed for it: not even the transformer slots)
    from pyvbmc_amd import _lib

    fresh = _lib.Context(0)
    try:
        assert fresh._lib.vbmc_warp_points(fresh._h, c.D, 0, 0, None, None, None, None) == 0
    finally:
        fresh.close()
