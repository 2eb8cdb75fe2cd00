"""The parameter transformer on the device (csrc/transform.hip) against the reference's values in
tests/golden/transform.npz, and VariationalPosterior's original-space calls routed through it
against the host path (``VBMC_HIP_TRANSFORM=0``) on the same draws.

Measured on the MI355X over the fixture's five cases: forward / inverse / log|J| at most 9.8e-16 from
the reference (relative to the larger of |value| and 1; probit's forward), bit-equal on every
non-finite and nudged value; pdf at most 8.6e-13 relative (probit, next to the bounds where
exp(log|J|) is far from 1), log_pdf at most 1.1e-14."""
import numpy as np
import pytest
from helpers import rel_err
from transform_host import CASES, RefShapedTransformer, golden_vp

pytestmark = pytest.mark.gpu

XF_TOL = 2e-15  # the measured maximum (docstring) with headroom for libm differences between boxes
PDF_TOL = 1e-11


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


def _close(a, b, tol):
    """Equal where b is not finite (NaN where NaN), |a - b| <= tol * max(|b|, 1) elsewhere."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    fin = np.isfinite(b)
    assert np.array_equal(a[~fin], b[~fin], equal_nan=True), (a[~fin], b[~fin])
    err = np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), 1.0)
    return float(err.max()) if err.size else 0.0


@pytest.mark.parametrize("name", CASES)
def test_transform_matches_the_reference(ctx, golden, name):
    from pyvbmc_amd.transformer import DeviceTransformer

    g = golden("transform")
    dt = DeviceTransformer(RefShapedTransformer.from_golden(g, name), ctx)
    x, u = g[f"{name}_x"], g[f"{name}_u"]
    assert _close(dt(x), g[f"{name}_u_fwd"], XF_TOL) <= XF_TOL
    assert _close(dt.inverse(u), g[f"{name}_x_inv"], XF_TOL) <= XF_TOL
    assert _close(dt.log_abs_det_jacobian(u), g[f"{name}_ladj"], XF_TOL) <= XF_TOL
    # the nudged boundary values come back exactly (one ulp inside the bounds)
    xi = dt.inverse(u)
    ref = g[f"{name}_x_inv"]
    edge = np.isfinite(ref) & ((ref == np.nextafter(dt.lb_orig, np.inf)) | (ref == np.nextafter(dt.ub_orig, -np.inf)))
    assert np.array_equal(xi[edge], ref[edge])
    # handle_0D_1D_input: a 1-D point comes back 1-D, its log|J| as a scalar
    assert dt(x[0]).shape == (x.shape[1],) and np.ndim(dt.log_abs_det_jacobian(u[0])) == 0
    assert _close(dt.inverse(u[1]), ref[1], XF_TOL) <= XF_TOL


@pytest.mark.parametrize("name", CASES)
def test_pdf_orig_matches_the_reference(ctx, golden, name):
    from pyvbmc_amd import VariationalPosterior

    g = golden("transform")
    vp = golden_vp(VariationalPosterior, g, name, RefShapedTransformer.from_golden(g, name), ctx)
    xp = g[f"{name}_pdf_x"]
    for df in ("0", "7"):
        y, ly = g[f"{name}_pdf_df{df}"], g[f"{name}_logpdf_df{df}"]
        out = vp.pdf(xp, orig_flag=True, df=float(df))
        assert out.shape == y.shape and np.array_equal(out == 0, y == 0)
        # (outside this range the linear value passes through a subnormal or overflowing exp(log|J|))
        sel = (y > 1e-200) & (y < 1e200)
        assert np.max(np.abs(out[sel] - y[sel]) / y[sel]) <= PDF_TOL
        lo = vp.log_pdf(xp, orig_flag=True, df=float(df))
        assert np.array_equal(np.isneginf(lo), np.isneginf(ly))
        assert _close(lo, ly, PDF_TOL) <= PDF_TOL


def test_variants_logit_case_on_the_device(ctx, golden):
    """variants.npz's pdfo_* case (the reference's logit transformer) through the fused entry, at the
    tolerances of test_pdf_orig_space_bounded_transformer -- gradient rows included."""
    from test_gpu_parity import make_vp

    g = golden("variants")
    D = int(g["D"])
    lb, ub = g["pt_lb"].reshape(1, D), g["pt_ub"].reshape(1, D)
    pt = RefShapedTransformer(g["pt_type"], lb, ub, g["pt_mu"], g["pt_delta"])
    vp = make_vp(g, ctx)
    vp.parameter_transformer = pt
    x, m = g["pdfo_x"], g["pdfo_mask"]
    y = vp.pdf(x, orig_flag=True)
    assert y.shape == g["pdfo_y"].shape and np.all(y[~m] == 0)
    assert rel_err(y, g["pdfo_y"]) < 1e-10
    ly = vp.log_pdf(x, orig_flag=True)
    assert np.all(np.isneginf(ly[~m])) and np.allclose(ly[m], g["pdfo_logy"][m], rtol=0, atol=1e-10)
    yy, dy = vp.pdf(x, orig_flag=True, grad_flag=True)
    assert rel_err(yy, g["pdfo_y_g"]) < 1e-10
    assert np.allclose(dy, g["pdfo_dy"], rtol=1e-9, atol=1e-300 + 1e-10 * np.abs(g["pdfo_dy"]).max())
    for df in (7.0, -3.0):
        assert rel_err(vp.pdf(x, orig_flag=True, df=df), g[f"pdfo_y_df{df}"]) < 1e-10
    one = vp.pdf(x[3], orig_flag=True)
    assert one.shape == g["pdfo_1d"].shape and rel_err(one, g["pdfo_1d"]) < 1e-10
    with pytest.raises(NotImplementedError):
        vp.pdf(x, orig_flag=True, log_flag=True, grad_flag=True)


def _vp(golden, ctx, name="roto"):
    from pyvbmc_amd import VariationalPosterior

    g = golden("transform")
    return golden_vp(VariationalPosterior, g, name, RefShapedTransformer.from_golden(g, name), ctx)


def _raising(pt):
    def boom(*a, **k):
        raise AssertionError("host transformer called")

    pt.__class__ = type("RaisingTransformer", (RefShapedTransformer,),
                        {"__call__": boom, "inverse": boom, "log_abs_det_jacobian": boom})
    return pt


@pytest.mark.parametrize("name", ["roto", "student4", "mixed"])
def test_sample_orig_is_the_inverse_of_the_transformed_draws(ctx, golden, name, monkeypatch):
    vp = _vp(golden, ctx, name)
    pt = vp.parameter_transformer
    for bal in (False, True):
        u, iu = vp.sample(5000, orig_flag=False, balance_flag=bal, rng="philox", seed=77, shuffle=False)
        x, ix = vp.sample(5000, orig_flag=True, balance_flag=bal, rng="philox", seed=77, shuffle=False)
        assert np.array_equal(iu, ix)
        assert _close(x, pt.inverse(u), 1e-12) <= 1e-12
    # numpy stream: the host draws exactly as before, then the device inverse; NumPy's state is the host path's
    np.random.seed(5)
    x_dev, _ = vp.sample(3000, orig_flag=True, balance_flag=True)
    st_dev = np.random.get_state()
    monkeypatch.setenv("VBMC_HIP_TRANSFORM", "0")
    np.random.seed(5)
    x_host, _ = vp.sample(3000, orig_flag=True, balance_flag=True)
    st_host = np.random.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(st_dev, st_host))
    assert _close(x_dev, x_host, 1e-12) <= 1e-12


def test_moments_orig_on_the_device(ctx, golden):
    vp = _vp(golden, ctx)
    N = 200_000
    x, _ = vp.sample(N, orig_flag=True, balance_flag=True, rng="philox", seed=11, shuffle=False)
    mu, cov = vp.moments(N, orig_flag=True, cov_flag=True, rng="philox", seed=11)
    assert mu.shape == (1, vp.D) and cov.shape == (vp.D, vp.D)
    scale = np.sqrt(np.diag(np.cov(x.T)))
    assert np.max(np.abs(mu[0] - np.mean(x, axis=0)) / np.maximum(np.abs(np.mean(x, axis=0)), scale)) <= 1e-12
    c = np.cov(x.T)
    assert np.max(np.abs(cov - c) / np.outer(scale, scale)) <= 1e-12
    assert np.allclose(vp.moments(N, orig_flag=True, rng="philox", seed=11), mu, rtol=0, atol=0)


def _kl_pair(golden, ctx):
    a = _vp(golden, ctx, "roto")
    b = _vp(golden, ctx, "roto")
    pb = b.parameter_transformer
    pb.mu = pb.mu + 0.1
    pb.scale = pb.scale * 1.2
    b.mu = b.mu + 0.05
    return a, b


def test_kl_div_between_transformers_matches_the_host_branch(ctx, golden, monkeypatch):
    a, b = _kl_pair(golden, ctx)
    kl_dev = a.kl_div(b, N=100_000, rng="philox", seed=3)
    # equal-by-value but distinct transformer objects: the transformed-space call
    c = _vp(golden, ctx, "roto")
    kl_same = a.kl_div(c, N=100_000, rng="philox", seed=3)
    monkeypatch.setenv("VBMC_HIP_TRANSFORM", "0")
    kl_host = a.kl_div(b, N=100_000, rng="philox", seed=3)
    kl_same_host = a.kl_div(c, N=100_000, rng="philox", seed=3)
    assert np.all(kl_host > 0)
    assert np.max(np.abs(kl_dev - kl_host)) <= 1e-10 * max(1.0, np.max(np.abs(kl_host)))
    assert np.max(np.abs(kl_same - kl_same_host)) <= 1e-10 * max(1.0, np.max(np.abs(kl_same_host)))


def test_original_space_calls_never_use_the_host_transformer(ctx, golden, monkeypatch):
    """The feature's own test: with the recognised transformer's host methods replaced by functions that
    raise, pdf / sample / moments / the cross-transformer kl_div still return the host path's values."""
    a, b = _kl_pair(golden, ctx)
    g = golden("transform")
    xp = g["roto_pdf_x"]
    monkeypatch.setenv("VBMC_HIP_TRANSFORM", "0")
    y_host = a.pdf(xp, orig_flag=True)
    xs_host, _ = a.sample(2000, orig_flag=True, rng="philox", seed=9)
    xm, _ = a.sample(50_000, orig_flag=True, balance_flag=True, rng="philox", seed=9, shuffle=False)
    kl_host = a.kl_div(b, N=20_000, rng="philox", seed=4)
    monkeypatch.setenv("VBMC_HIP_TRANSFORM", "1")
    _raising(a.parameter_transformer)
    _raising(b.parameter_transformer)
    assert _close(a.pdf(xp, orig_flag=True), y_host, 1e-11) <= 1e-11
    xs, _ = a.sample(2000, orig_flag=True, rng="philox", seed=9)
    assert _close(xs, xs_host, 1e-12) <= 1e-12
    mu, cov = a.moments(50_000, orig_flag=True, cov_flag=True, rng="philox", seed=9)
    assert np.allclose(mu[0], np.mean(xm, axis=0), rtol=1e-12, atol=1e-12)
    c = np.cov(xm.T)
    assert np.max(np.abs(cov - c) / np.sqrt(np.outer(np.diag(c), np.diag(c)))) <= 1e-12
    kl = a.kl_div(b, N=20_000, rng="philox", seed=4)
    assert np.max(np.abs(kl - kl_host)) <= 1e-10 * max(1.0, np.max(np.abs(kl_host)))
