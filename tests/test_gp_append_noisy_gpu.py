"""GPU tests of the one-point append under per-point noise: vbmc_gp_append_noisy (csrc/api_gp_post.hip; the append
kernels of csrc/gp_post.hip with the new point's noise read through a pointer and a stride) and its Python route
``pyvbmc_amd.gp.append_point`` / ``GP.append(s2_new=...)``.

Shapes: N = 63 -> 64, 64 -> 65, 127 -> 128 (the block boundaries of the 64 x 64 Cholesky and of the padded width of
L^-1), S = 2, D = 3 and D = 32, zero and negative-quadratic mean.  The appended state is compared with
vbmc_gp_posterior on the extended data and with the oracle, under the bounds tests/test_gp_post_gpu.py holds the
constant-noise append to (its ``check_records`` / ``check_predict`` / ``predict_bound``: L and alpha within the
forward factor 4 N eps cond2(A), predict within max(1e-10, that) sf^2), reused by name.
"""
import numpy as np
import pytest

import gp_post_host as gph
import test_gp_post_gpu as tgp
from oracle import gp_ref

pytestmark = pytest.mark.gpu

S = 2
SHAPES = [(N0, D, mean) for N0 in (63, 64, 127) for D in (3, 32) for mean in (gp_ref.MEAN_ZERO, gp_ref.MEAN_NEGQUAD)]


class CallLog:
    """The library handle with the names of the entry points looked up recorded."""

    def __init__(self, lib):
        self._lib_real, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib_real, name)


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


@pytest.fixture()
def calls(ctx):
    real = ctx._lib
    ctx._lib = CallLog(real)
    yield ctx._lib
    ctx._lib = real


def noisy_case(N0, D, mean):
    """N0 + 1 points, S samples, and a user noise column whose last entry is not the smallest: the appended point then
    leaves every sample's sn2_div as it is."""
    X, y, hyp = gph.make_case(N0 + 1, D, S, mean, seed=700 + N0 + D)
    s2 = 0.01 + 0.02 * np.random.default_rng(N0 + D).random((N0 + 1, 1))
    s2[N0, 0] = max(s2[N0, 0], 1.5 * np.min(s2[:N0]))
    return X, y, hyp, s2


@pytest.mark.parametrize("N0,D,mean", SHAPES)
def test_noisy_append_against_the_build(ctx, calls, N0, D, mean):
    from pyvbmc_amd.gp import append_point, device_posterior, upload_gp

    X, y, hyp, s2 = noisy_case(N0, D, mean)
    gp = tgp.mirror_gp(ctx, X[:N0], y[:N0], mean, s2=s2[:N0])
    assert device_posterior(gp, hyp, ctx=ctx)
    del calls.names[:]
    append_point(gp, X[N0], y[N0, 0], s2[N0, 0], ctx=ctx)
    assert "vbmc_gp_append_noisy" in calls.names and "vbmc_gp_posterior" not in calls.names
    assert gp.X.shape == (N0 + 1, D) and gp.y.shape == (N0 + 1, 1) and np.array_equal(gp.s2, s2)
    ogp = gp_ref.make_gp(X, y, hyp, mean, s2=s2, noise_user=True)
    factors = tgp.sample_factors(ogp)
    tgp.check_records(gp.posteriors, ogp, factors, f"noisy append {N0}->{N0 + 1} D={D}")
    upload_gp(gp, ctx)
    assert "vbmc_set_gp" not in calls.names
    xs = tgp.points(ogp, 32, N0)
    fmu, fs2 = tgp.check_predict(gp, ogp, factors, xs, f"N={N0 + 1} D={D}")
    fresh = tgp.mirror_gp(ctx, X, y, mean, s2=s2)
    assert device_posterior(fresh, hyp, ctx=ctx)
    fmu_f, fs2_f = fresh.predict(xs, separate_samples=True)
    for p, q, (A, f) in zip(gp.posteriors, fresh.posteriors, factors):
        e_L = np.max(np.abs(p.L - q.L)) / np.max(np.abs(q.L))
        e_a = np.max(np.abs(p.alpha - q.alpha)) / np.max(np.abs(q.alpha))
        print(f"vs build: dL {e_L:.2e}, dalpha {e_a:.2e}, factor {f:.2e}")
        assert e_L <= f and e_a <= f
        assert np.array_equal(p.sW, q.sW)
    b = tgp.predict_bound(factors, tgp.sf2_of(hyp, D))
    assert np.max(np.abs(fs2 - fs2_f)) <= b and np.max(np.abs(fmu - fmu_f)) <= b


def test_two_noisy_appends_and_the_class_method(ctx, calls):
    """GP.append(s2_new=...) twice in a row, without fetching L in between."""
    from pyvbmc_amd.gp import device_posterior, fetch_posteriors

    N0, D, mean = 63, 3, gp_ref.MEAN_NEGQUAD
    X, y, hyp = gph.make_case(N0 + 2, D, S, mean, seed=31)
    s2 = 0.01 + 0.02 * np.random.default_rng(3).random((N0 + 2, 1))
    s2[N0:, 0] = np.maximum(s2[N0:, 0], 1.5 * np.min(s2[:N0]))
    gp = tgp.mirror_gp(ctx, X[:N0], y[:N0], mean, s2=s2[:N0])
    assert device_posterior(gp, hyp, ctx=ctx, fetch=False)
    del calls.names[:]
    for n in (N0, N0 + 1):
        gp.append(X[n], y[n, 0], s2[n, 0], fetch=False)
        assert all(p.L is None for p in gp.posteriors)
    assert calls.names.count("vbmc_gp_append_noisy") == 2 and "vbmc_gp_posterior" not in calls.names
    fetch_posteriors(gp, ctx)
    ogp = gp_ref.make_gp(X, y, hyp, mean, s2=s2, noise_user=True)
    tgp.check_records(gp.posteriors, ogp, tgp.sample_factors(ogp), "two noisy appends")


def test_noise_below_sn2_div_is_refused_and_rebuilt(ctx, calls):
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gp import append_point, device_posterior

    N0, D, mean = 64, 3, gp_ref.MEAN_NEGQUAD
    X, y, hyp, s2 = noisy_case(N0, D, mean)
    s2[N0, 0] = 0.5 * np.min(s2[:N0])  # the new point would lower every sample's sn2_div
    gp = tgp.mirror_gp(ctx, X[:N0], y[:N0], mean, s2=s2[:N0])
    assert device_posterior(gp, hyp, ctx=ctx)
    before = [p.alpha.copy() for p in gp.posteriors]
    sn2_new = _lib.f64(np.exp(2 * hyp[:, D + 1]) + s2[N0, 0])
    rc = ctx._lib.vbmc_gp_append_noisy(ctx._h, _lib.ptr(_lib.f64(X[N0])), float(y[N0, 0]), _lib.ptr(sn2_new), None, None)
    assert rc == _lib.E_UNSUP
    alpha = np.empty((S, N0))
    ctx.check(ctx._lib.vbmc_gp_fetch(ctx._h, _lib.ptr(alpha), None))  # the resident state is untouched
    assert all(np.array_equal(alpha[s], before[s].ravel()) for s in range(S))
    del calls.names[:]
    append_point(gp, X[N0], y[N0, 0], s2[N0, 0], ctx=ctx)
    assert "vbmc_gp_append_noisy" in calls.names and "vbmc_gp_posterior" in calls.names
    fresh = tgp.mirror_gp(ctx, X, y, mean, s2=s2)
    assert device_posterior(fresh, hyp, ctx=ctx)
    for p, q in zip(gp.posteriors, fresh.posteriors):  # the same build of the same data
        assert np.array_equal(p.alpha, q.alpha) and np.array_equal(p.L, q.L) and np.array_equal(p.sW, q.sW)
    assert gp.X.shape[0] == N0 + 1 and np.array_equal(gp.s2, s2)


@pytest.mark.parametrize("N0", [63, 64, 127])
def test_constant_noise_entries_are_bitwise_equal(ctx, N0):
    """On a constant-noise state vbmc_gp_append and vbmc_gp_append_noisy (new entries = sl) give the same bits, the
    state stays appendable by vbmc_gp_append, and a truly noisy append ends that."""
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gp import device_posterior, invalidate_gp

    D, mean = 3, gp_ref.MEAN_NEGQUAD
    X, y, hyp = gph.make_case(N0 + 2, D, S, mean, seed=N0)
    x, xx = _lib.f64(X[N0]), _lib.f64(X[N0 + 1])
    sl = _lib.f64(np.exp(2 * hyp[:, D + 1]))  # GaussianNoise.compute's constant
    out = []
    for noisy in (False, True):
        gp = tgp.mirror_gp(ctx, X[:N0], y[:N0], mean)
        assert device_posterior(gp, hyp, ctx=ctx)
        alpha, L = np.empty((S, N0 + 1)), np.empty((S, N0 + 1, N0 + 1))
        if noisy:
            rc = ctx._lib.vbmc_gp_append_noisy(ctx._h, _lib.ptr(x), float(y[N0, 0]), _lib.ptr(sl), _lib.ptr(alpha), _lib.ptr(L))
        else:
            rc = ctx._lib.vbmc_gp_append(ctx._h, _lib.ptr(x), float(y[N0, 0]), _lib.ptr(alpha), _lib.ptr(L))
        ctx.check(rc)
        alpha2 = np.empty((S, N0 + 2))
        ctx.check(ctx._lib.vbmc_gp_append(ctx._h, _lib.ptr(xx), float(y[N0 + 1, 0]), _lib.ptr(alpha2), None))
        out.append((alpha, L, alpha2))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    more = _lib.f64(1.25 * sl)
    x3 = _lib.f64(X[0] + 0.2)
    ctx.check(ctx._lib.vbmc_gp_append_noisy(ctx._h, _lib.ptr(x3), 0.1, _lib.ptr(more), None, None))
    assert ctx._lib.vbmc_gp_append(ctx._h, _lib.ptr(x3 + 0.1), 0.1, None, None) == _lib.E_UNSUP
    invalidate_gp(ctx)  # (the state was changed behind the Python key)


def test_noisy_append_needs_a_device_built_posterior(ctx):
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gp import append_point

    N0, D, mean = 63, 3, gp_ref.MEAN_CONST
    X, y, hyp, s2 = noisy_case(N0, D, mean)
    gp = tgp.mirror_gp(ctx, X[:N0], y[:N0], mean, s2=s2[:N0])
    gp.update(hyp=hyp)  # host route
    gp.predict(X[:4])   # uploaded through vbmc_set_gp
    sn2_new = _lib.f64(np.exp(2 * hyp[:, D + 1]) + s2[N0, 0])
    rc = ctx._lib.vbmc_gp_append_noisy(ctx._h, _lib.ptr(_lib.f64(X[N0])), float(y[N0, 0]), _lib.ptr(sn2_new), None, None)
    assert rc == _lib.E_ARG
    append_point(gp, X[N0], y[N0, 0], s2[N0, 0], ctx=ctx)  # the Python route rebuilds on the extended data
    ogp = gp_ref.make_gp(X, y, hyp, mean, s2=s2, noise_user=True)
    tgp.check_records(gp.posteriors, ogp, tgp.sample_factors(ogp), "append without a resident device posterior")
    with pytest.raises(ValueError):
        append_point(gp, X[0] + 0.1, 0.5, None, ctx=ctx)  # a GP with s2 needs the new point's
