"""The device transformer (csrc/transform.h, transform.hip) at every padded width of its kernels, against the
reference's values in tests/golden/transform_wide.npz (D = 1 .. 32, both sides of log|J|'s pairwise-sum
switch at D = 8, rotated and scaled cases up to D = 32), and the original-space calls routed through it:
pdf, sample, moments (every pair slot of the covariance kernel), kl_div, batch boundaries, and one context
switching between transformers.

Tolerances.  Without rotation: XF_TOL of max(|ref|, 1), as test_transform_gpu.py.  With rotation both sides
round a dot product of length D (BLAS there, a chain of fma here), each within D eps (|a| @ |b|) of the exact
one, so the two differ by up to 2 D eps (|a| @ |b|):
  forward  u = (v @ R) / scale, v the vector before the rotation:  2 D eps (|v| @ |R|) / scale;
  inverse and log|J| start from the same rounding of the unrotated w = (u scale) @ R^T, E = 2 D eps
  (|u scale| @ |R^T|), and carry it through y = w delta + mu.  The inverse of a bounded dimension is
  (ub - lb) g^-1(y) + lb, and the slope of g^-1 is at most 1/4 (logit), 1/sqrt(2 pi) (probit) or 3/8
  (student4): at most 0.4 (ub - lb) delta E; an unbounded one moves by delta E.  log|J|'s term has slope
  below 1 (logit), 5/4 (student4) or |y| (probit: the change is at most |y| dY + dY^2 / 2), dY = delta E.
Rows with a finite coordinate beyond 1e150 are compared only without rotation: with it, what the rotation's
cancellation leaves in the other coordinates is rounding residue (~1e290 at 1e308), and which of 0, -inf or
NaN comes out is decided by that residue, on either side.

Measured on the MI355X, as a fraction of the allowed error (XF_TOL max(|ref|, 1), plus the bound above where
rotated): forward at most 0.22 (w6, w8, w16: 4.5e-16 relative), inverse 0.89 (w6, w8, w17), log|J| 0.076
(w12); pdf / log_pdf at most 8.1e-14 relative (w25), every case below 1e-13."""
import numpy as np
import pytest
from test_transform_gpu import PDF_TOL, XF_TOL, _close
from transform_host import WIDE_CASES, RefShapedTransformer, golden_vp

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
BIG = 1e150  # a coordinate beyond this is one of the fixture's overflowing extremes
# the largest slope of g^-1 and of the log|J| term per type (probit's log|J| slope is |y|: handled apart)
_INV_SLOPE = {3.0: 0.25, 12.0: 0.3989422804014327, 13.0: 0.375}
_LJ_SLOPE = {3.0: 1.0, 13.0: 1.25}


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


@pytest.fixture(scope="module")
def wide(golden):
    return golden("transform_wide")


def _pt(g, name):
    return RefShapedTransformer.from_golden(g, name)


def _vp(g, name, ctx, pt=None):
    from pyvbmc_amd import VariationalPosterior

    return golden_vp(VariationalPosterior, g, name, _pt(g, name) if pt is None else pt, ctx)


def _check(a, b, bound):
    """b non-finite: a equal (NaN where NaN); finite: |a - b| <= XF_TOL max(|b|, 1) + bound.  Entries whose
    bound is not finite are not compared.  Returns the largest error in units of the allowed one."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    bound = np.broadcast_to(bound, b.shape)
    assert a.shape == b.shape
    det = np.isfinite(bound)
    fin = np.isfinite(b) & det
    nf = ~np.isfinite(b) & det
    assert np.array_equal(a[nf], b[nf], equal_nan=True), (a[nf], b[nf])
    allowed = XF_TOL * np.maximum(np.abs(b[fin]), 1.0) + bound[fin]
    r = np.abs(a[fin] - b[fin]) / allowed
    assert np.all(r <= 1.0), float(r.max())
    return float(r.max()) if r.size else 0.0


def _rows_ok(pt, pts):
    """Rows whose values are determined by the computation, not by a rotation's cancellation residue."""
    if pt.R_mat is None:
        return np.ones(pts.shape[0], dtype=bool)
    with np.errstate(invalid="ignore"):
        return ~np.any(np.isfinite(pts) & (np.abs(pts) > BIG), axis=1)


def _bounds(pt, x, u):
    """Per-entry rotation bounds of forward(x), inverse(u), log|J|(u) (module docstring); 0 without R."""
    D = pt.type.size
    if pt.R_mat is None:
        return 0.0, 0.0, 0.0
    aR = np.abs(pt.R_mat)
    with np.errstate(all="ignore"):
        plain = RefShapedTransformer(pt.type, pt.lb_orig, pt.ub_orig, pt.mu, pt.delta)
        v = plain(x)
        fwd = 2 * D * EPS * (np.abs(v) @ aR) / pt.scale
        w = np.abs(u * pt.scale) @ aR.T
        E = 2 * D * EPS * w
        y = (u * pt.scale) @ pt.R_mat.T * pt.delta + pt.mu
        dY = pt.delta * E
        span = (pt.ub_orig - pt.lb_orig)[0]
        inv = np.empty_like(E)
        lj = np.zeros(u.shape[0])
        for d in range(D):
            t = float(pt.type[d])
            if t == 0:
                inv[:, d] = dY[:, d]
            else:
                inv[:, d] = _INV_SLOPE[t] * span[d] * dY[:, d]
                lj += (np.abs(y[:, d]) + 0.5 * dY[:, d]) * dY[:, d] if t == 12.0 else _LJ_SLOPE[t] * dY[:, d]
    return np.nan_to_num(fwd, nan=np.inf), np.nan_to_num(inv, nan=np.inf), np.nan_to_num(lj, nan=np.inf)


@pytest.mark.parametrize("name", WIDE_CASES)
def test_transform_at_every_width(ctx, wide, name):
    from pyvbmc_amd.transformer import DeviceTransformer

    g = wide
    pt = _pt(g, name)
    dt = DeviceTransformer(pt, ctx)
    x, u = g[f"{name}_x"], g[f"{name}_u"]
    bf, bi, bl = _bounds(pt, x, u)
    okx, oku = _rows_ok(pt, x), _rows_ok(pt, u)
    ef = _check(dt(x)[okx], g[f"{name}_u_fwd"][okx], np.broadcast_to(bf, x.shape)[okx])
    xi = dt.inverse(u)
    ref = g[f"{name}_x_inv"]
    ei = _check(xi[oku], ref[oku], np.broadcast_to(bi, u.shape)[oku])
    el = _check(dt.log_abs_det_jacobian(u)[oku], g[f"{name}_ladj"][oku], np.broadcast_to(bl, u.shape[:1])[oku])
    print(f"{name}: forward {ef:.3g}, inverse {ei:.3g}, log|J| {el:.3g} of the allowed error")
    # the nudged boundary values come back exactly (one ulp inside the bounds)
    edge = np.isfinite(ref) & ((ref == np.nextafter(pt.lb_orig, np.inf)) | (ref == np.nextafter(pt.ub_orig, -np.inf)))
    if pt.R_mat is None:
        assert edge.sum() >= 2
    assert np.array_equal(xi[edge], ref[edge])
    # handle_0D_1D_input: a 1-D point comes back 1-D, its log|J| as a scalar
    assert dt(x[0]).shape == (x.shape[1],) and np.ndim(dt.log_abs_det_jacobian(u[0])) == 0
    _check(dt.inverse(u[1]), ref[1], np.broadcast_to(bi, u.shape)[1])
    if pt.type.size == 1:  # D = 1: a 0-D point is one row and stays 2-D, a 1-D one is one point
        for f, h in ((dt, pt), (dt.inverse, pt.inverse)):
            assert f(x[0, 0]).shape == (1, 1) and f(x[:1, 0]).shape == (1,)
            assert _close(f(x[3, 0]), h(x[3, 0]), XF_TOL) <= XF_TOL
        assert np.ndim(dt.log_abs_det_jacobian(u[2, 0])) == 1 and np.ndim(dt.log_abs_det_jacobian(u[2, :1])) == 0
        assert _close(dt.log_abs_det_jacobian(u[2, :1]), g[f"{name}_ladj"][2], XF_TOL) <= XF_TOL


@pytest.mark.parametrize("name", WIDE_CASES)
def test_pdf_orig_at_every_width(ctx, wide, name):
    g = wide
    vp = _vp(g, name, ctx)
    pt = vp.parameter_transformer
    xp = g[f"{name}_pdf_x"]
    ok = _rows_ok(pt, xp) | ~(np.all(xp > pt.lb_orig, axis=1) & np.all(xp < pt.ub_orig, axis=1))
    big = np.any(np.abs(xp) > BIG, axis=1)
    errs = []
    for df in ("0", "7"):
        y, ly = g[f"{name}_pdf_df{df}"][ok], g[f"{name}_logpdf_df{df}"][ok]
        out = vp.pdf(xp, orig_flag=True, df=float(df))[ok]
        assert out.shape == y.shape and np.array_equal(out == 0, y == 0)
        assert np.array_equal(np.isnan(out), np.isnan(y))
        sel = (y > 1e-200) & (y < 1e200)
        errs.append(np.max(np.abs(out[sel] - y[sel]) / y[sel]))
        lo = vp.log_pdf(xp, orig_flag=True, df=float(df))[ok]
        assert np.array_equal(np.isneginf(lo), np.isneginf(ly))
        errs.append(_close(lo, ly, PDF_TOL))
        if pt.R_mat is None:  # the overflowing squared distances: exactly 0 and -inf, no NaN
            assert np.all(out[big[ok]] == 0) and np.all(np.isneginf(lo[big[ok]]))
            assert not np.any(np.isnan(out)) and not np.any(np.isnan(lo))
    if f"{name}_pdf_g" in g:
        y, dy = vp.pdf(xp, orig_flag=True, grad_flag=True)
        yr, dyr = g[f"{name}_pdf_g"][ok], g[f"{name}_dpdf_g"][ok]
        y, dy = y[ok], dy[ok]
        assert np.array_equal(np.isnan(y), np.isnan(yr)) and np.array_equal(y == 0, yr == 0)
        sel = (yr > 1e-200) & (yr < 1e200)
        errs.append(np.max(np.abs(y[sel] - yr[sel]) / yr[sel]))
        assert np.array_equal(np.isnan(dy), np.isnan(dyr))
        fin = np.isfinite(dyr)
        scale = np.abs(dyr[fin]).max()
        assert np.allclose(dy[fin], dyr[fin], rtol=1e-9, atol=1e-300 + 1e-10 * scale)
        assert np.all(dy[big[ok] & ~np.isnan(yr[:, 0])] == 0)
    print(f"{name}: pdf / log_pdf at most {max(errs):.3g}")
    assert max(errs) <= PDF_TOL


@pytest.mark.parametrize("name", WIDE_CASES)
def test_sample_orig_at_every_width(ctx, wide, name):
    vp = _vp(wide, name, ctx)
    pt = vp.parameter_transformer
    for df in (np.inf, 7.0):
        for bal in (False, True):
            kw = dict(balance_flag=bal, df=df, rng="philox", seed=31, shuffle=False)
            u, iu = vp.sample(1500, orig_flag=False, **kw)
            x, ix = vp.sample(1500, orig_flag=True, **kw)
            assert np.array_equal(iu, ix) and x.shape == (1500, pt.type.size)
            assert _close(x, pt.inverse(u), 1e-12) <= 1e-12


@pytest.mark.parametrize("name", WIDE_CASES)
def test_moments_orig_at_every_width(ctx, wide, name):
    """N = 2 and 300 leave most of the 512 blocks empty; N = 64 * 512 + 1 gives the blocks 65 rows each, a
    64-row tile and one row left.  At D = 32 the covariance's P = 528 pairs fill the third pair slot."""
    vp = _vp(wide, name, ctx)
    for N in (2, 300, 64 * 512 + 1):
        x, _ = vp.sample(N, orig_flag=True, balance_flag=True, rng="philox", seed=11, shuffle=False)
        mu, cov = vp.moments(N, orig_flag=True, cov_flag=True, rng="philox", seed=11)
        D = vp.D
        c = np.cov(x.T)
        assert x.shape == (N, D) and mu.shape == (1, D) and cov.shape == c.shape  # (np.cov's: 0-D at D = 1)
        c, cov = np.atleast_2d(c), np.atleast_2d(cov)
        scale = np.sqrt(np.diag(c))
        m = np.mean(x, axis=0)
        assert np.max(np.abs(mu[0] - m) / np.maximum(np.abs(m), scale)) <= 1e-12
        assert np.max(np.abs(cov - c) / np.outer(scale, scale)) <= 1e-12
        assert np.array_equal(cov, cov.T)


@pytest.mark.parametrize("name", ["w9", "w17", "w32"])
def test_kl_div_between_transformers_at_width(ctx, wide, name, monkeypatch):
    a = _vp(wide, name, ctx)
    b = _vp(wide, name, ctx)
    pb = b.parameter_transformer
    pb.mu = pb.mu + 0.1
    pb.delta = pb.delta * 1.1
    if pb.scale is not None:
        pb.scale = pb.scale * 1.2
    b.mu = b.mu + 0.05
    kl_dev = a.kl_div(b, N=50_000, rng="philox", seed=3)
    monkeypatch.setenv("VBMC_HIP_TRANSFORM", "0")
    kl_host = a.kl_div(b, N=50_000, rng="philox", seed=3)
    assert np.all(kl_host > 0)
    assert np.max(np.abs(kl_dev - kl_host)) <= 1e-10 * max(1.0, np.max(np.abs(kl_host)))


def _split(f, z, cut):
    return np.concatenate([f(z[:cut]), f(z[cut:])])


@pytest.mark.parametrize("name", ["w1", "w2"])
def test_transform_across_the_batch_boundary(ctx, wide, name):
    """vbmc_transform works in batches of 2^21 points: one call over 2^21 + 3 is the two calls it is made of."""
    from pyvbmc_amd.transformer import DeviceTransformer

    g = wide
    pt = _pt(g, name)
    dt = DeviceTransformer(pt, ctx)
    n = (1 << 21) + 3
    rng = np.random.default_rng(5)
    x = g[f"{name}_x"][rng.integers(0, 24, n)]  # (the fixture's points inside the bounds)
    u = rng.standard_normal((n, pt.type.size)) * 2.0
    for f, h, z in ((dt, pt, x), (dt.inverse, pt.inverse, u), (dt.log_abs_det_jacobian, pt.log_abs_det_jacobian, u)):
        whole = f(z)
        assert np.array_equal(whole, _split(f, z, (1 << 21) - 5))
        tail = slice(n - 1000, n)
        assert _close(whole[tail], h(z[tail]), 1e-13) <= 1e-13


def test_pdf_orig_across_the_batch_boundary(ctx, wide):
    """vbmc_mixture_pdf_orig works in batches of 2^22 points."""
    g = wide
    vp = _vp(g, "w1", ctx)
    n = (1 << 22) + 5
    xp = g["w1_pdf_x"]
    x = xp[np.random.default_rng(6).integers(0, xp.shape[0], n)]
    y = vp.pdf(x, orig_flag=True)
    assert np.array_equal(y, _split(lambda z: vp.pdf(z, orig_flag=True), x, (1 << 22) - 7))
    tail = slice(n - 1000, n)
    ref = vp.pdf(x[tail], orig_flag=True)
    assert np.array_equal(y[tail], ref)
    small = np.concatenate([xp, x[tail]])
    assert np.array_equal(vp.pdf(small, orig_flag=True)[xp.shape[0]:], ref)


def test_one_context_switches_between_transformers(ctx, wide):
    """Each call runs with the transformer it is given: widths 32 -> 1 -> 32 on one context (the descriptor
    upload's skip of unchanged values), and a field edited in place between two calls (the field-id cache)."""
    from pyvbmc_amd.transformer import DeviceTransformer

    g = wide
    p32, p1 = _pt(g, "w32"), _pt(g, "w1")
    u32, u1 = g["w32_u"][:40], g["w1_u"][:40]
    first = DeviceTransformer(p32, ctx).inverse(u32)
    assert _close(first, g["w32_x_inv"][:40], 1e-13) <= 1e-13
    assert _close(DeviceTransformer(p1, ctx).inverse(u1), g["w1_x_inv"][:40], XF_TOL) <= XF_TOL
    assert np.array_equal(DeviceTransformer(p32, ctx).inverse(u32), first)
    d32 = DeviceTransformer(p32, ctx)
    mu0, delta0 = p32.mu.copy(), p32.delta.copy()
    p32.mu[0] += 0.5
    p32.delta[3] *= 2.0
    moved = d32.inverse(u32)
    assert not np.array_equal(moved, first)
    assert _close(moved, p32.inverse(u32), 1e-12) <= 1e-12
    assert _close(d32.log_abs_det_jacobian(u32), p32.log_abs_det_jacobian(u32), 1e-12) <= 1e-12
    # the same through the posterior's calls: pdf with w1, then w32 edited in place, on one context
    v1, v32 = _vp(g, "w1", ctx, p1), _vp(g, "w32", ctx, p32)
    x1, x32 = g["w1_pdf_x"][:20], g["w32_pdf_x"][:20]
    y1 = v1.pdf(x1, orig_flag=True)
    assert _close(y1, g["w1_pdf_df0"][:20], PDF_TOL) <= PDF_TOL
    p32.mu[:], p32.delta[:] = mu0, delta0
    y32 = v32.pdf(x32, orig_flag=True)
    assert _close(y32, g["w32_pdf_df0"][:20], PDF_TOL) <= PDF_TOL
    assert np.array_equal(v1.pdf(x1, orig_flag=True), y1)
