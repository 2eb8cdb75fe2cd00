"""CPU tests of input warping: the NumPy statement of tests/whitening_host.py against the reference's stored outputs
(tests/golden/whitening.npz, tools/make_whitening_golden.py) and its MATLAB known answers, the package's ``device=False``
route against the statement, the edge cases, and the drop-in pair."""
import types

import numpy as np
import pytest

import whitening_host as wh

RTOL = 1e-12  # the statement against the reference, under the recorded seed
STATE_FLAGS = ("recompute_var_post", "skip_active_sampling", "warping_count", "last_warping", "last_successful_warping")


def close(a, b, what, rtol=RTOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, f"{what}: shapes {a.shape} {b.shape}"
    err = np.max(np.abs(a - b) / np.maximum(np.max(np.abs(b)), 1e-300)) if a.size else 0.0
    assert err <= rtol, f"{what}: relative error {err:.2e} > {rtol:.0e}"


@pytest.fixture(scope="module", params=wh.CASES)
def case(request):
    return wh.load_case(request.param)


@pytest.fixture(scope="module")
def host_input(case):
    return wh.run_warp_input(case)


def test_unscent_example_matches_reference_and_matlab():
    g = wh.golden()
    old, new = wh.Xf.from_golden(g, "ua_old_"), wh.Xf.from_golden(g, "ua_new_")
    mean, sd, pts = wh.unscent_warp(old, new, g["ua_x"], g["ua_sigma"])
    close(mean, g["ua_mean"], "mean")
    close(sd, g["ua_sd"], "sd")
    close(pts, g["ua_pts"], "points")
    # the reference test's own tolerance against MATLAB
    assert np.all(np.isclose(mean, g["matlab_ua_mean"], atol=1e-4))
    assert np.all(np.isclose(sd, g["matlab_ua_sd"], atol=1e-4))
    assert np.all(np.isclose(pts, g["matlab_ua_pts"], atol=1e-4))


def test_statement_unscent_matches_reference(case):
    mean, sd, pts = wh.unscent_warp(case.old, case.new, case.mu.T, (case.lambd * case.sigma).T)
    close(mean, case.un_mean, "mean")
    close(sd, case.un_sd, "sd")
    close(pts, case.un_pts, "points")


def test_statement_warp_input_matches_reference(case, host_input):
    R, scale, r = host_input
    close(R, case.new_R, "R_mat")
    close(scale, case.new_scale, "scale")
    assert np.all(case.new_mu == 0) and np.all(case.new_delta == 1)
    for key in ("plb_tran", "pub_tran", "lb_search", "ub_search"):
        close(getattr(r, key), getattr(case, "out_" + key), key)
    close(r.X, case.out_X, "X")
    close(r.y, case.out_y, "y")
    close(r.search_cache, case.out_search_cache, "search_cache")


def test_statement_warp_gp_and_vp_matches_reference(case):
    hyp, mu, sigma, lambd, w = wh.run_warp_gp_and_vp(case)
    close(hyp, case.hyp_warped, "hyp_warped")
    close(mu, case.vp_mu, "mu")
    close(sigma, case.vp_sigma, "sigma")
    close(lambd, case.vp_lambd, "lambd")
    close(w, case.vp_w, "w")


def test_matlab_tables_case_a():
    g, c = wh.golden(), wh.load_case("a")
    R, scale, _ = wh.run_warp_input(c)
    assert np.all(np.isclose(R, g["matlab_a_R_mat"], atol=1e-4))
    assert np.all(np.isclose(scale, g["matlab_a_scale"].ravel(), atol=1e-4))
    hyp, mu, sigma, lambd, w = wh.run_warp_gp_and_vp(c)
    assert np.allclose(hyp, g["matlab_a_hyp_warped"], atol=1e-4)
    assert np.allclose(mu, g["matlab_a_vp_mu"], atol=1e-4)
    assert np.allclose(w, g["matlab_a_vp_w"], atol=1e-4)
    assert np.allclose(sigma, g["matlab_a_vp_sigma"], atol=1e-4)
    assert np.allclose(lambd, g["matlab_a_vp_lambda"].T, atol=1e-4)


def test_long_double_statement_agrees(case):
    """The extended-precision evaluation is the same function: it agrees with float64 far inside the tests' bounds."""
    f = wh.run_warp_gp_and_vp(case)
    t = wh.run_warp_gp_and_vp(case, np.longdouble)
    for a, b in zip(f, t):
        assert b.dtype == np.longdouble
        close(a, b.astype(np.float64), "long double", rtol=1e-9)


# ---- the package's device=False route ------------------------------------------------------------------------------
def test_host_route_warp_input(case, host_input):
    from pyvbmc_amd import whitening

    vp, state, flog, options, _ = wh.package_inputs(case)
    np.random.seed(int(case.np_seed))
    before = (state["lb_search"].copy(), flog.X.copy())
    pt, st2, fl2, action = whitening.warp_input(vp, state, flog, options, device=False)
    # the global stream is where the reference leaves it
    assert np.random.rand() == float(case.next_draw)
    R, scale, r = host_input
    assert np.array_equal(pt.R_mat, R) and np.array_equal(pt.scale, scale)
    assert np.all(pt.mu == 0) and np.all(pt.delta == 1) and action == "rotoscale"
    for key in ("plb_tran", "pub_tran", "lb_search", "ub_search"):
        assert st2[key].shape == (1, case.D)
        close(st2[key], getattr(r, key), key)
    close(fl2.X, r.X, "X")
    close(fl2.y, r.y, "y")
    close(np.reshape(st2["search_cache"], (-1, case.D)), r.search_cache, "search_cache")
    for key in STATE_FLAGS:
        assert float(st2[key]) == float(getattr(case, "out_" + key)), key
    assert st2["run_mean"] == [] and st2["run_cov"] == [] and np.isnan(st2["last_run_avg"])
    assert fl2.parameter_transformer is pt
    # deep copies: the caller's objects are untouched
    assert np.array_equal(state["lb_search"], before[0]) and np.array_equal(flog.X, before[1])
    assert state["warping_count"] == int(case.warping_count) and vp.parameter_transformer is not pt


def test_host_route_warp_gp_and_vp(case):
    from pyvbmc_amd import whitening

    vp, state, _, _, gp = wh.package_inputs(case)
    vbmc = types.SimpleNamespace(D=case.D, optim_state=state)
    vp2, hyp = whitening.warp_gp_and_vp(case.new.as_object(), gp, vp, vbmc, device=False)
    ref = wh.run_warp_gp_and_vp(case)
    assert hyp.shape == case.hyp.shape
    for got, want, what in zip((hyp, vp2.mu, vp2.sigma, vp2.lambd, vp2.w), ref, ("hyp", "mu", "sigma", "lambd", "w")):
        close(got, want, what)
    assert abs(np.sum(vp2.w) - 1) < 1e-15 and vp2 is not vp and np.array_equal(vp.mu, case.mu)


def test_host_route_unscent_warp_shapes():
    from pyvbmc_amd import whitening

    c = wh.load_case("b")
    fun = whitening.Warp(c.old.as_object(), c.new.as_object())
    x, sigma = c.mu.T, (c.lambd * c.sigma).T
    mean, sd, pts = whitening.unscent_warp(fun, x, sigma, device=False)
    assert mean.shape == x.shape and pts.shape == (2 * c.D + 1, c.K, c.D)
    close(mean, c.un_mean, "mean")
    close(sd, c.un_sd, "sd")
    # sigma with one row against n rows is broadcast; a 1-D x gives 1-D results
    m1, s1, _ = whitening.unscent_warp(fun, x, sigma[:1], device=False)
    m2, s2, _ = whitening.unscent_warp(fun, x, np.tile(sigma[:1], (c.K, 1)), device=False)
    assert np.array_equal(m1, m2) and np.array_equal(s1, s2)
    m3, s3, p3 = whitening.unscent_warp(fun, x[0], sigma[0], device=False)
    assert m3.shape == (c.D,) and s3.shape == (c.D,) and p3.shape == (2 * c.D + 1, 1, c.D)
    close(m3, mean[0], "1-D mean")


# ---- edge cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_row_count_mismatch_raises(device):
    from pyvbmc_amd import whitening

    c = wh.load_case("b")
    fun = whitening.Warp(c.old.as_object(), c.new.as_object())
    with pytest.raises(ValueError, match="Mismatch between rows of X and SIGMA."):
        whitening.unscent_warp(fun, np.zeros((3, c.D)), np.ones((2, c.D)), device=device)
    with pytest.raises(ValueError, match="Mismatch between columns of X and SIGMA."):
        whitening.unscent_warp(fun, np.zeros((3, c.D)), np.ones((3, c.D + 1)), device=device)
    with pytest.raises(ValueError, match="Mismatch between rows"):
        wh.unscent_warp(c.old, c.new, np.zeros((3, c.D)), np.ones((2, c.D)))


def test_warp_nonlinear_raises():
    from pyvbmc_amd import whitening

    vp, state, flog, options, _ = wh.package_inputs(wh.load_case("b"))
    options["warp_nonlinear"] = True
    with pytest.raises(NotImplementedError, match="Non-linear warping is not supported."):
        whitening.warp_input(vp, state, flog, options, device=False)


def test_zero_mean_raises_value_error():
    from pyvbmc_amd import whitening

    c = wh.load_case("c")
    vp, state, _, _, gp = wh.package_inputs(c)
    gp.mean = wh.ZeroMean()
    vbmc = types.SimpleNamespace(D=c.D, optim_state=state)
    for device in (False, True):
        with pytest.raises(ValueError, match="Unsupported GP mean function for input warping."):
            whitening.warp_gp_and_vp(c.new.as_object(), gp, vp, vbmc, device=device)


class OpaqueTransformer:
    """A transformer with the three calls and none of the reference's fields."""

    def __init__(self, pt):
        self._pt = pt

    def __call__(self, x):
        return self._pt(x)

    def inverse(self, u):
        return self._pt.inverse(u)

    def log_abs_det_jacobian(self, u):
        return self._pt.log_abs_det_jacobian(u)


def test_unrecognised_transformer_is_unsupported_before_any_draw():
    from pyvbmc_amd import _lib, whitening

    c = wh.load_case("b")
    vp, state, flog, options, gp = wh.package_inputs(c)
    vp.parameter_transformer = OpaqueTransformer(vp.parameter_transformer)
    np.random.seed(3)
    with pytest.raises(_lib.UnsupportedShape):
        whitening.warp_input(vp, state, flog, options)
    st = np.random.RandomState(3)
    assert np.random.rand() == st.rand()  # nothing was drawn
    vbmc = types.SimpleNamespace(D=c.D, optim_state=state)
    with pytest.raises(_lib.UnsupportedShape):
        whitening.warp_gp_and_vp(c.new.as_object(), gp, vp, vbmc)
    with pytest.raises(_lib.UnsupportedShape):
        whitening.unscent_warp(lambda x: x, c.mu.T, c.mu.T)
    # the host route takes any transformer
    vp2, _ = whitening.warp_gp_and_vp(c.new.as_object(), gp, vp, vbmc, device=False)
    close(vp2.mu, c.vp_mu, "mu")


def test_d33_is_unsupported_in_python():
    from pyvbmc_amd import _lib, whitening
    from transform_host import RefShapedTransformer

    D = 33
    pt = RefShapedTransformer(np.zeros(D), np.full(D, -np.inf), np.full(D, np.inf), np.zeros(D), np.ones(D))
    with pytest.raises(_lib.UnsupportedShape):
        whitening.unscent_warp(whitening.Warp(pt, pt), np.zeros((2, D)), np.ones((1, D)))


# ---- the drop-in pair ------------------------------------------------------------------------------------------------
def test_patch_whitening_round_trip_and_fallback():
    from pyvbmc_amd import _lib, dropin, whitening

    calls = []

    def ref_warp_input(vp, optim_state, function_logger, options):
        calls.append("warp_input")
        return "reference result"

    def ref_warp_gp_and_vp(parameter_transformer, gp_old, vp_old, vbmc):
        calls.append("warp_gp_and_vp")
        return "reference result"

    mod = types.SimpleNamespace(warp_input=ref_warp_input, warp_gp_and_vp=ref_warp_gp_and_vp, other=1)
    assert dropin.patch_whitening(mod) is mod
    assert mod.warp_input.__wrapped__ is whitening.warp_input
    assert mod.warp_gp_and_vp.__wrapped__ is whitening.warp_gp_and_vp
    first = mod.warp_input
    dropin.patch_whitening(mod)  # idempotent: the saved functions are still the reference's
    assert mod.warp_input is not ref_warp_input and first.__wrapped__ is mod.warp_input.__wrapped__
    # an UnsupportedShape raised by the mirror reaches the saved function, without the mirror's keywords
    c = wh.load_case("b")
    vp, state, flog, options, gp = wh.package_inputs(c)
    vp.parameter_transformer = OpaqueTransformer(vp.parameter_transformer)
    assert mod.warp_input(vp, state, flog, options, rng="numpy", n_search=10) == "reference result"
    vbmc = types.SimpleNamespace(D=c.D, optim_state=state)
    assert mod.warp_gp_and_vp(c.new.as_object(), gp, vp, vbmc) == "reference result"
    assert calls == ["warp_input", "warp_gp_and_vp"]
    dropin.unpatch_whitening(mod)
    assert mod.warp_input is ref_warp_input and mod.warp_gp_and_vp is ref_warp_gp_and_vp and mod.other == 1
    assert not hasattr(mod, dropin._SAVED_WARP)
    dropin.unpatch_whitening(mod)  # a second unpatch is a no-op
    # a module without the names gets the mirrors and loses them again
    bare = types.SimpleNamespace()
    dropin.patch_whitening(bare)
    assert bare.warp_input is whitening.warp_input
    dropin.unpatch_whitening(bare)
    assert not hasattr(bare, "warp_input")
    assert issubclass(_lib.UnsupportedShape, NotImplementedError)
