"""CPU tests of VariationalPosterior.mode: argument errors and the ``_mode`` cache (no device touched), the
restatement's derivatives, the restatement against the reference's stored results (tests/golden/mode.npz,
tools/make_mode_golden.py), stationarity and known answers.

Tolerances.  F_TOL = K D eps max(1, |f|): the rounding of one log-density evaluation, both values coming from
the same host function.  X_TOL = 1.7e-6: twice the largest distance between a reference result and the
stationary point the restatement reaches from it -- measured over the fixture at 8.2e-7 (d6_overlap in the
original space: L-BFGS-B with difference gradients; 1.1e-7 over the transformed-space cases, d2_bounded).
Measured here: f_host - f_ref between 0 and 2e-14 in the transformed space (every case, every seed) and between 0
and 0.59 in the original space (the reference's L-BFGS-B stops early next to the bounds: d10_bounded); x within
1.2e-7 (transformed) and 8.2e-7 (original, identity transformer) of the reference's; free gradient <= 1e-15.
No (case, seed) pair needs an exception.

The "roto" cases' original-space log-density is NaN everywhere (a negative ``delta`` under the logarithm of
log|J|), in the reference too: the fixture holds NaN and those pairs carry no f condition.  The rotated search with
finite densities is tested in tests/test_mode_gpu.py (ROTO_FINITE) and, for the derivatives, here.
"""
from pathlib import Path

import numpy as np
import pytest

import mode_host as mh
from transform_host import RefShapedTransformer

GOLDEN = Path(__file__).resolve().parent / "golden" / "mode.npz"
X_TOL = 1.7e-6
# (case, seed) pairs of the bounded original-space cases whose reference run ended in another basin (at most one
# may be listed, each with the evidence that both points are stationary): none is needed
ORIG_BASIN_EXCEPTIONS = ()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def reference_conditions(g, name, orig, si, x, f_host):
    """The f and x conditions of result ``x`` (log-density ``f_host`` by mode_host.host_log_pdf) against the
    reference's run ``si`` of the case."""
    o = int(bool(orig))
    D, K, kind = mh.CASES[name][:3]
    if int(g[f"{name}_o{o}_raised"][si]):
        return
    mu, sigma, lambd, w = mh.case_mixture(name)
    pt = mh.golden_transformer(g, name)
    xr = g[f"{name}_o{o}_x"][si]
    f_ref = mh.host_log_pdf(mu, sigma, lambd, w, pt, xr, orig)[0]
    print(name, o, si, "f - f_ref", f_host - f_ref, "|x - x_ref|", np.max(np.abs(x - xr)))
    if np.isfinite(f_ref) and (name, mh.SEEDS[si]) not in ORIG_BASIN_EXCEPTIONS:
        assert f_host >= f_ref - mh.f_tol(K, D, f_ref)
    refs = g[f"{name}_o{o}_x"]
    agree = np.max(np.abs(refs - refs[0])) <= 1e-6
    if (not orig and agree) or (orig and kind == "identity" and not int(g[f"{name}_o{o}_raised"][si])):
        assert np.max(np.abs(x - xr)) <= X_TOL


def _no_device(monkeypatch):
    from pyvbmc_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_lib, "default_context", boom)
    monkeypatch.setattr(_lib, "Context", boom)


def test_argument_errors_touch_no_device(monkeypatch):
    from pyvbmc_amd import VariationalPosterior

    vp = VariationalPosterior(2, 2)
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="n_opts"):
        vp.mode(n_opts=0)
    with pytest.raises(ValueError, match="n_opts"):
        vp.mode(False, -3)
    with pytest.raises(ValueError, match="unknown rng"):
        vp.mode(rng="mt")
    monkeypatch.setenv("VBMC_HIP_RNG", "bogus")
    with pytest.raises(ValueError, match="unknown rng"):
        vp.mode()


def test_mode_cache(monkeypatch):
    from pyvbmc_amd import VariationalPosterior

    vp = VariationalPosterior(2, 2)
    calls = []

    def fake(orig_flag, n_opts, mode, seed):
        calls.append((orig_flag, n_opts, mode))
        return np.array([1.0, 2.0]) + len(calls), {}

    monkeypatch.setattr(vp, "_mode_search", fake)
    t = vp.mode(orig_flag=False)
    assert vp._mode is None and calls == [(False, 2, "numpy")]
    x = vp.mode()
    assert vp._mode is x and vp.mode() is x and len(calls) == 2
    assert vp.mode(orig_flag=False) is not t and len(calls) == 3
    vp.set_parameters(vp.get_parameters())
    assert vp._mode is None
    assert vp.mode() is not x and len(calls) == 4


def _transformer(kind, D, seed):
    r = np.random.RandomState(seed)
    typ = {"logit": 3, "probit": 12, "student4": 13, "roto": 3}[kind]
    types = np.where(np.arange(D) % 2 == 0, typ, 0).astype(float)
    lb = np.where(types != 0, -4.0 - r.rand(D), -np.inf)
    ub = np.where(types != 0, 4.0 + r.rand(D), np.inf)
    R = scale = None
    if kind == "roto":
        R, scale = mh.rotoscale(D, seed)
    return RefShapedTransformer(types, lb, ub, r.randn(D) * 0.3, np.exp(r.randn(D) * 0.2), R, scale)


@pytest.mark.parametrize("kind", ["none", "logit", "probit", "student4", "roto"])
def test_derivatives_match_central_differences(kind):
    """Analytic gradient against central differences of the oracle's log-pdf (mode_host.host_log_pdf), analytic
    Hessian against central differences of the analytic gradient, at random points of the search coordinates.
    A central difference with step h errs by h^2 M3 / 6 (truncation, M3 the third derivative) plus eps |f| / h
    (rounding): with h = 1e-5, |f| <= 50 and M3 <= 1e4 (the component scales are >= 0.3, so M3 ~ |y - mu| / s^4 ~
    1e3) that is 1.7e-7 + 1.1e-9; the bound is 1e-6 max(1, |value|)."""
    D, K, h = 4, 3, 1e-5
    mu, sigma, lambd, w = mh.kde_host.mixture_params(D, K, 17)
    pt = None if kind == "none" else _transformer(kind, D, 5)
    orig = pt is not None
    obj = mh.Objective(mu, sigma, lambd, w, pt, orig)
    r = np.random.RandomState(2)
    for _ in range(5):
        y = r.randn(D) * 1.2
        f, g, H, _ = obj.full(y)
        fx = mh.host_log_pdf(mu, sigma, lambd, w, pt, obj.x_from_y(y), orig)[0]
        assert abs(f - fx) <= 1e-12 * max(1.0, abs(fx))
        for d in range(D):
            e = h * (np.arange(D) == d)
            gd = (mh.host_log_pdf(mu, sigma, lambd, w, pt, obj.x_from_y(y + e), orig)[0]
                  - mh.host_log_pdf(mu, sigma, lambd, w, pt, obj.x_from_y(y - e), orig)[0]) / (2 * h)
            assert abs(gd - g[d]) <= 1e-6 * max(1.0, abs(g[d]))
            Hd = (obj.full(y + e)[1] - obj.full(y - e)[1]) / (2 * h)
            assert np.max(np.abs(Hd - H[d])) <= 1e-6 * max(1.0, np.max(np.abs(H[d])))


@pytest.mark.parametrize("orig", [False, True])
@pytest.mark.parametrize("name", list(mh.CASES))
def test_restatement_against_the_reference(golden, name, orig):
    D, K = mh.CASES[name][:2]
    mu, sigma, lambd, w = mh.case_mixture(name)
    pt = mh.golden_transformer(golden, name)
    obj = mh.Objective(mu, sigma, lambd, w, pt, orig)
    n_opts = int(np.ceil(np.sqrt(K)))
    for si, seed in enumerate(mh.SEEDS):
        np.random.seed(seed)
        with np.errstate(all="ignore"):
            cands = mh.draw_candidates(mu, sigma, lambd, w, pt, orig, n_opts)
            x, f, recs, pts, ys = mh.mode_host(mu, sigma, lambd, w, pt, orig, cands, fast=True)
        reference_conditions(golden, name, orig, si, x, f)
        if np.isfinite(f):
            best = int(np.argmax([r[2] for r in recs]))
            gmax, outward = mh.stationarity(obj, ys[best])
            print(name, orig, seed, "free gradient", gmax)
            assert gmax <= 1e-9 and outward


def test_single_component_mode_is_its_centre():
    mu, sigma, lambd, w = mh.kde_host.mixture_params(5, 1, 9)
    y, f, it, st = mh.search(mh.Objective(mu, sigma, lambd, w), mu[:, 0] + 0.7)
    assert np.max(np.abs(y - mu[:, 0])) <= 1e-12 and st == mh.CONVERGED


def test_two_far_components_mode_is_the_denser_centre():
    D = 3
    mu = np.array([[-20.0, 20.0]] * D)
    sigma, lambd = np.array([[1.0, 0.5]]), np.ones((D, 1))
    w = np.array([[0.7, 0.3]])  # w / sigma^D: 0.7 against 2.4
    np.random.seed(1)
    cands = mh.draw_candidates(mu, sigma, lambd, w, None, False, 2, n=2000)
    x, f, recs, _, _ = mh.mode_host(mu, sigma, lambd, w, None, False, cands)
    assert np.max(np.abs(x - mu[:, 1])) <= 1e-9


def test_host_path_without_a_device(golden):
    """No device: the reference's loop around a NumPy density, its result within X_TOL of the fixture's."""
    from pyvbmc_amd import _lib

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    vp = mh.golden_vp(golden, "d2_bounded")
    np.random.seed(100)
    u = vp.mode(orig_flag=False)
    assert not vp.mode_info["device"] and u.shape == (2,) and vp._mode is None
    assert np.max(np.abs(u - golden["d2_bounded_o0_x"][0])) <= X_TOL
    x = vp.mode()
    assert vp._mode is x and vp.mode() is x


def test_host_only_context_with_philox_is_a_loud_failure(golden):
    """The device generator needs a device: no quiet change of generator on the host path."""
    from pyvbmc_amd import _lib

    vp = mh.golden_vp(golden, "d2_bounded")
    vp.ctx = _lib.Context(-1)
    with pytest.raises(_lib.NoDeviceError):
        vp.mode(orig_flag=False, rng="philox", seed=3)
    assert vp._mode is None
    vp.ctx.close()
