"""VariationalPosterior.mode on the device (csrc/mode.hip, vbmc_mixture_mode) against tests/mode_host.py's
restatement and the reference's stored results (tests/golden/mode.npz, tools/make_mode_golden.py).

Tolerances.  F_TOL = K D eps max(1, |f|), the rounding of one log-density evaluation (both values come from the
same host function).  X_TOL = 1.7e-6: twice the largest distance between a reference result and the stationary
point the restatement reaches from it, measured over the fixture at 8.2e-7 (d6_overlap in the original space,
L-BFGS-B with difference gradients; 1.1e-7 over the transformed-space cases).  DEV_TOL, device against
restatement from the same start: both stop after a Newton step <= 1e-12 max(1, |y|_inf), which by quadratic
convergence leaves each within that of the stationary point; x moves at most (ub - lb) / 4 <= 2.5 times as far
as y (the steepest bounded map here, logit at its centre): 2 * 2.5e-12, doubled for the rounding of the
stationary point itself -> 1e-11 max(1, |y|_inf).  Stationarity: 1e-9 on the free dimensions, taken at the
search coordinates the device reports (mode_info["search_points"]; y recomputed from a bounded x next to its bound
would carry only ~8 digits).

The fixture's two "roto" cases have a negative ``delta`` in the original space: log|J| and with it every
original-space log-density is NaN, in the reference too (the fixture stores NaN).  There no candidate wins, the
first one is returned as it is, and the tests ask only that device and restatement agree.  The rotated and scaled
original-space search is therefore covered by ROTO_FINITE below: the same shapes and mixtures around a transformer
with rotation, scale and a positive delta (test_mode_host._transformer), checked like the bounded cases -- device
against restatement, stationarity, reported value, Philox -- without a reference run.

Measured on the MI355X over every case, space and seed: device against restatement <= 2e-16 (of max(1, |y|)),
reported value against the host density <= 4e-15, and the whole call with rng="philox" 0.33 ms at D = 10, K = 50
and 1.0-1.1 ms at D = 20, K = 100 (profiles/mode_rows.json; the reference takes 7-54 s there).
"""
import numpy as np
import pytest

import mode_host as mh
import kde_host
from test_mode_host import GOLDEN, X_TOL, _transformer, reference_conditions

pytestmark = pytest.mark.gpu

DEV_TOL = 1e-11
PDF_PARITY = 1e-12  # the project's pdf parity bound (tests/test_gpu_parity.py), relative to max(1, |f|)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    return _lib.default_context()


def _objective(vp, g, name, orig):
    return mh.Objective(vp.mu, vp.sigma, vp.lambd, vp.w, mh.golden_transformer(g, name), orig)


def _best_y(info, x):
    """The device's search coordinates of the returned point."""
    p = info["points"]
    r = int(np.flatnonzero(np.all((p == x) | (np.isnan(p) & np.isnan(x)), axis=1))[0])
    return info["search_points"][r]


def _check_stationary(obj, y, f):
    if not np.isfinite(f):
        print("log-density", f, ": no stationarity condition")
        return
    gmax, outward = mh.stationarity(obj, y)
    print("free gradient", gmax)
    assert gmax <= 1e-9
    assert outward


@pytest.mark.parametrize("orig", [False, True])
@pytest.mark.parametrize("name", list(mh.CASES))
def test_numpy_stream_matches_restatement_and_reference(ctx, golden, name, orig):
    D, K = mh.CASES[name][:2]
    vp = mh.golden_vp(golden, name)
    pt = mh.golden_transformer(golden, name)
    obj = _objective(vp, golden, name, orig)
    for si, seed in enumerate(mh.SEEDS):
        vp._mode = None
        np.random.seed(seed)
        x = vp.mode(orig_flag=orig)
        info = vp.mode_info
        assert info["device"] and x.shape == (D,) and x.dtype == np.float64
        # the restatement's search from the same candidates: the start index is the device's (start selection has
        # its own test), the candidates are the reference's draws
        np.random.seed(seed)
        cands = mh.draw_candidates(vp.mu, vp.sigma, vp.lambd, vp.w, pt, orig, info["records"].shape[0])
        worst = 0.0
        for r, rec in enumerate(info["records"]):
            y, _, _, _ = mh.search(obj, obj.y_from_x(cands[r][int(rec[0])]))
            d = np.max(np.abs(obj.x_from_y(y) - info["points"][r]))
            worst = max(worst, d / max(1.0, np.max(np.abs(y))))
        print(name, orig, seed, "device - restatement", worst)
        assert worst <= DEV_TOL
        f_host = mh.host_log_pdf(vp.mu, vp.sigma, vp.lambd, vp.w, pt, x, orig)[0]
        reference_conditions(golden, name, orig, si, x, f_host)
        _check_stationary(obj, _best_y(info, x), f_host)
        assert (np.isnan(info["log_pdf"]) and np.isnan(f_host)) or abs(info["log_pdf"] - f_host) <= PDF_PARITY * max(1.0, abs(f_host))


def _call(ctx, vp, orig, n, cand, seed, n_opts):
    from pyvbmc_amd import _lib
    from pyvbmc_amd import transformer as _xf
    from pyvbmc_amd.variational_posterior import _device_pt

    vp._upload(ctx)
    if orig:
        assert _xf.upload(_device_pt(vp), ctx, 0, vp.D) is not None
    x, f = np.empty(vp.D), np.empty(1)
    rec, pts = np.empty((n_opts, 5)), np.empty((n_opts, vp.D))
    ctx.check(ctx._lib.vbmc_mixture_mode(ctx._h, n_opts, int(orig), n, _lib.ptr(cand), seed, 200, 1e-12, _lib.ptr(x),
                                         _lib.ptr(f), _lib.ptr(rec), _lib.ptr(pts), None))
    return x, f[0], rec, pts


def check_start_selection(ctx, vp, orig, n, n_opts=3):
    """Per round the device's start index is np.argmin of -pdf over the same n candidates, centres included."""
    vp.ctx = ctx
    np.random.seed(5)
    cand = np.ascontiguousarray(np.stack([vp.sample(n, orig)[0] for _ in range(n_opts)]))
    _, _, rec, _ = _call(ctx, vp, orig, n, cand, 0, n_opts)
    for r in range(n_opts):
        pts = cand[r]
        if r == 0:
            centres = vp.mu.T
            pts = np.concatenate([pts, vp.parameter_transformer.inverse(centres) if orig else centres])
        vals = -vp.pdf(np.ascontiguousarray(pts), orig_flag=orig, log_flag=True).ravel()
        assert int(rec[r, 0]) == int(np.argmin(vals))
        assert abs(rec[r, 1] + vals[int(rec[r, 0])]) <= PDF_PARITY * max(1.0, abs(rec[r, 1]))


@pytest.mark.parametrize("name, orig", [("d10", False), ("d2_bounded", True), ("d10_bounded", True)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 100000])
def test_start_selection_is_the_host_argmin(ctx, golden, name, orig, n):
    """Per round the device's start index is np.argmin of -pdf over the same candidates, centres included (tile
    sizes 1, 63, 64, 65 and 1e5 + K)."""
    check_start_selection(ctx, mh.golden_vp(golden, name), orig, n)


def test_start_selection_tie_goes_to_the_lowest_index(ctx, golden):
    """Two copies of the best centre among the samples tie with the centre itself (index N + k): the lowest index wins."""
    vp = mh.golden_vp(golden, "d10")
    vp.ctx = ctx
    np.random.seed(6)
    cand = vp.sample(1000, False)[0][None].copy()
    k = int(np.argmax(vp.pdf(vp.mu.T, orig_flag=False, log_flag=True).ravel()))
    cand[0, 700] = vp.mu.T[k]
    cand[0, 130] = vp.mu.T[k]
    _, _, rec, _ = _call(ctx, vp, False, 1000, cand, 0, 1)
    vals = vp.pdf(np.concatenate([cand[0], vp.mu.T]), orig_flag=False, log_flag=True).ravel()
    assert int(np.argmin(-vals)) == 130
    assert int(rec[0, 0]) == 130


def check_philox_mode(vp, pt, obj, orig, monkeypatch):
    """``mode(rng="philox")`` calls no host method, repeats bit for bit, ends at a stationary point and beats the centres."""
    from pyvbmc_amd import VariationalPosterior

    vp.pdf(vp.mu.T[:1], orig_flag=orig)  # (uploads before the methods are patched)

    def boom(*a, **k):
        raise AssertionError("host method called")

    monkeypatch.setattr(VariationalPosterior, "sample", boom)
    monkeypatch.setattr(VariationalPosterior, "pdf", boom)
    x = vp.mode(orig_flag=orig, rng="philox", seed=77)
    vp._mode = None
    again = vp.mode(orig_flag=orig, rng="philox", seed=77)
    np.testing.assert_array_equal(x, again)
    f = mh.host_log_pdf(vp.mu, vp.sigma, vp.lambd, vp.w, pt, x, orig)[0]
    _check_stationary(obj, _best_y(vp.mode_info, x), f)
    centres = vp.mu.T if not (orig and pt is not None) else pt.inverse(vp.mu.T)
    fc = np.max(mh.host_log_pdf(vp.mu, vp.sigma, vp.lambd, vp.w, pt, centres, orig))
    assert f >= fc - mh.f_tol(vp.K, vp.D, f)
    return x, f


@pytest.mark.parametrize("name, orig", [("d10", False), ("d10", True), ("d10_bounded", True), ("d2_bounded", False),
                                        ("d6_overlap", False), ("d20", True)])
def test_philox_repeats_is_stationary_and_beats_the_centres(ctx, golden, name, orig, monkeypatch):
    vp = mh.golden_vp(golden, name)
    check_philox_mode(vp, mh.golden_transformer(golden, name), _objective(vp, golden, name, orig), orig, monkeypatch)


def test_philox_start_is_the_best_philox_sample(ctx, golden):
    vp = mh.golden_vp(golden, "d10_bounded")
    vp.ctx = ctx
    _, _, rec, _ = _call(ctx, vp, True, 5000, None, 31, 2)
    for r in range(2):
        xs = vp.sample(5000, True, rng="philox", seed=31 + r)[0]
        if r == 0:
            xs = np.concatenate([xs, vp.parameter_transformer.inverse(vp.mu.T)])
        assert int(rec[r, 0]) == int(np.argmin(-vp.pdf(xs, orig_flag=True, log_flag=True).ravel()))


def test_reported_value_is_the_pdf(ctx, golden):
    for name, orig in (("d10", False), ("d10_bounded", True), ("d6_overlap", True)):
        vp = mh.golden_vp(golden, name)
        x = vp.mode(orig_flag=orig, rng="philox", seed=3)
        f = float(np.ravel(vp.pdf(x, orig_flag=orig, log_flag=True))[0])
        assert abs(vp.mode_info["log_pdf"] - f) <= PDF_PARITY * max(1.0, abs(f))


def test_d1_original_space_returns_the_transformed_mode(ctx, golden):
    vp = mh.golden_vp(golden, "d1")
    np.random.seed(100)
    x = vp.mode(orig_flag=True)
    np.random.seed(100)
    u = vp.mode(orig_flag=False)
    assert x.shape == (1,) and abs(x[0] - u[0]) <= DEV_TOL * max(1.0, abs(u[0]))
    assert abs(x[0] - golden["d1_o0_x"][0, 0]) <= X_TOL


def test_d33_is_unsupported(ctx):
    from pyvbmc_amd import VariationalPosterior, _lib

    vp = VariationalPosterior(33, 2)
    with pytest.raises(_lib.UnsupportedShape):
        vp.mode(orig_flag=False)


def test_host_only_context_takes_the_host_path(ctx, golden):
    from pyvbmc_amd import _lib

    for name, orig in (("d2_bounded", False), ("d6_overlap", True)):
        vp = mh.golden_vp(golden, name)
        np.random.seed(100)
        x_dev = vp.mode(orig_flag=orig)
        assert vp.mode_info["device"]
        vh = mh.golden_vp(golden, name)
        vh.ctx = _lib.Context(-1)
        np.random.seed(100)
        x_host = vh.mode(orig_flag=orig)
        assert not vh.mode_info["device"]
        assert np.max(np.abs(x_host - x_dev)) <= X_TOL
        vh.ctx.close()


@pytest.mark.parametrize("n_opts", [1, 37])
def test_n_opts_rows(ctx, golden, n_opts):
    vp = mh.golden_vp(golden, "d10_bounded")
    x = vp.mode(orig_flag=False, n_opts=n_opts, rng="philox", seed=5)
    assert vp.mode_info["records"].shape == (n_opts, 5) and vp.mode_info["points"].shape == (n_opts, 10)
    assert np.all(np.isfinite(x))


ROTO_FINITE = [(10, 5, 7), (32, 4, 8), (6, 30, 21)]  # (D, K, seed): logit on the even dimensions, rotation, scale


def _roto_vp(D, K, seed):
    from pyvbmc_amd import VariationalPosterior

    pt = _transformer("roto", D, seed)
    state = np.random.get_state()
    vp = VariationalPosterior(D, K, parameter_transformer=pt)
    np.random.set_state(state)
    vp.mu, vp.sigma, vp.lambd, vp.w = kde_host.mixture_params(D, K, seed)
    if K == 30:
        vp.mu = vp.mu * 0.3  # overlapping components: the modes are not the centres
    return vp, pt


@pytest.mark.parametrize("D, K, seed", ROTO_FINITE)
def test_rotated_original_space_matches_the_restatement(ctx, D, K, seed):
    """Original space with rotation and scale, finite densities: J has off-diagonal terms, so a transposed R or J in
    the kernel would end at another point than the restatement."""
    vp, pt = _roto_vp(D, K, seed)
    obj = mh.Objective(vp.mu, vp.sigma, vp.lambd, vp.w, pt, True)
    assert np.max(np.abs(obj.J - np.diag(np.diag(obj.J)))) > 0.05
    for s in (100, 101):
        vp._mode = None
        np.random.seed(s)
        x = vp.mode(orig_flag=True)
        info = vp.mode_info
        assert info["device"]
        np.random.seed(s)
        cands = mh.draw_candidates(vp.mu, vp.sigma, vp.lambd, vp.w, pt, True, info["records"].shape[0])
        worst, moved = 0.0, 0.0
        for r, rec in enumerate(info["records"]):
            y0 = obj.y_from_x(cands[r][int(rec[0])])
            y, _, _, _ = mh.search(obj, y0)
            worst = max(worst, np.max(np.abs(obj.x_from_y(y) - info["points"][r])) / max(1.0, np.max(np.abs(y))))
            worst = max(worst, np.max(np.abs(y - info["search_points"][r])) / max(1.0, np.max(np.abs(y))))
            moved = max(moved, np.max(np.abs(y - y0)))
        print(D, K, s, "device - restatement", worst, "search moved", moved)
        assert worst <= DEV_TOL
        assert moved > 1e-3  # (the search did something: the start is not already the answer)
        f_host = mh.host_log_pdf(vp.mu, vp.sigma, vp.lambd, vp.w, pt, x, True)[0]
        assert np.isfinite(f_host)
        _check_stationary(obj, _best_y(info, x), f_host)
        f_dev = float(np.ravel(vp.pdf(x, orig_flag=True, log_flag=True))[0])
        assert abs(info["log_pdf"] - f_dev) <= PDF_PARITY * max(1.0, abs(f_dev))
        assert abs(info["log_pdf"] - f_host) <= PDF_PARITY * max(1.0, abs(f_host))
        f_start = np.max(info["records"][:, 1])
        assert info["log_pdf"] >= f_start - mh.f_tol(K, D, f_start)


@pytest.mark.parametrize("D, K, seed", ROTO_FINITE)
def test_rotated_original_space_philox(ctx, D, K, seed):
    vp, pt = _roto_vp(D, K, seed)
    obj = mh.Objective(vp.mu, vp.sigma, vp.lambd, vp.w, pt, True)
    x = vp.mode(orig_flag=True, rng="philox", seed=9)
    info = vp.mode_info
    vp._mode = None
    np.testing.assert_array_equal(x, vp.mode(orig_flag=True, rng="philox", seed=9))
    f = mh.host_log_pdf(vp.mu, vp.sigma, vp.lambd, vp.w, pt, x, True)[0]
    assert np.isfinite(f) and info["device"]
    _check_stationary(obj, _best_y(info, x), f)
    fc = np.max(mh.host_log_pdf(vp.mu, vp.sigma, vp.lambd, vp.w, pt, pt.inverse(vp.mu.T), True))
    assert f >= fc - mh.f_tol(K, D, f)
    # every round ends where the restatement ends from the same start (rebuilt from the device's own sample)
    for r, rec in enumerate(info["records"]):
        xs = vp.sample(100000, True, rng="philox", seed=9 + r)[0]
        if r == 0:
            xs = np.concatenate([xs, pt.inverse(vp.mu.T)])
        y, _, _, _ = mh.search(obj, obj.y_from_x(xs[int(rec[0])]))
        assert np.max(np.abs(y - info["search_points"][r])) <= DEV_TOL * max(1.0, np.max(np.abs(y)))


def test_non_orthogonal_rotation_takes_the_host_path(ctx):
    vp, pt = _roto_vp(4, 3, 5)
    pt.R_mat = pt.R_mat + 0.1 * np.random.RandomState(3).randn(4, 4)
    np.random.seed(100)
    x = vp.mode(orig_flag=True)
    assert not vp.mode_info["device"]
    f = float(np.ravel(vp.pdf(x, orig_flag=True, log_flag=True))[0])
    fc = np.max(vp.pdf(pt.inverse(vp.mu.T), orig_flag=True, log_flag=True))
    assert np.isfinite(f) and f >= fc - 1e-9
    u = vp.mode(orig_flag=False, rng="philox", seed=1)  # (the transformed space does not involve R)
    assert vp.mode_info["device"] and np.all(np.isfinite(u))


def test_explicit_numpy_rng_overrides_the_environment(ctx, golden, monkeypatch):
    vp = mh.golden_vp(golden, "d2_bounded")
    np.random.seed(100)
    x = vp.mode(orig_flag=False)
    rec = vp.mode_info["records"].copy()
    monkeypatch.setenv("VBMC_HIP_RNG", "philox")
    np.random.seed(100)
    x2 = vp.mode(orig_flag=False, rng="numpy")
    np.testing.assert_array_equal(rec, vp.mode_info["records"])
    np.testing.assert_array_equal(x, x2)
