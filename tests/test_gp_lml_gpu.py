"""GPU tests of the batched GP log marginal likelihood on the device: vbmc_gp_lml (csrc/gp_lml.hip, csrc/api_gp_lml.hip)
through pyvbmc_amd.gp.log_marginal_likelihood, against the host route and the longdouble restatement of
tests/gp_lml_host.py within the derived bounds stated there (f = 4 N eps cond2(A) times the absolute-term sums), plus
what the entry point promises: value-only calls, bit-reproducibility, chunking, a bad candidate in the middle of a
batch, and the posterior the context holds surviving the call."""
import ctypes as C

import numpy as np
import pytest

import gp_lml_host as glh
import gp_post_host as gph
from oracle import gp_ref
from test_gp_post_gpu import CountingLib, mirror_gp, points

pytestmark = pytest.mark.gpu

# (N, D, B, mean): the block edge and one column past it, three and five block steps with remainders, a padded D, the
# widest D (the [DMX][64] coordinate panels of the gradient tile full) and an odd D between the workload's two
CASES = [
    (1, 2, 1, gp_ref.MEAN_ZERO),
    (63, 3, 2, gp_ref.MEAN_CONST),
    (64, 3, 3, gp_ref.MEAN_NEGQUAD),
    (65, 3, 2, gp_ref.MEAN_NEGQUAD),
    (130, 10, 5, gp_ref.MEAN_NEGQUAD),
    (257, 20, 2, gp_ref.MEAN_NEGQUAD),
    (65, 32, 2, gp_ref.MEAN_NEGQUAD),
    (130, 13, 2, gp_ref.MEAN_CONST),
]


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


@pytest.fixture()
def counting(ctx):
    real = ctx._lib
    ctx._lib = CountingLib(real)
    yield ctx._lib
    ctx._lib = real


def check_against_both(dev, host, refs, factors, what):
    """Device against longdouble and against the host route, the host route against longdouble: value and every
    gradient entry within f vabs / f gabs."""
    for s, (ref, f) in enumerate(zip(refs, factors)):
        glh.check_within(dev[0][s], dev[1][s], ref, f, f"{what} s={s} device vs longdouble")
        glh.check_within(host[0][s], host[1][s], ref, f, f"{what} s={s} host vs longdouble")
        as_ref = dict(lml=np.longdouble(host[0][s]), grad=host[1][s].astype(np.longdouble), vabs=ref["vabs"], gabs=ref["gabs"])
        glh.check_within(dev[0][s], dev[1][s], as_ref, f, f"{what} s={s} device vs host")


@pytest.mark.parametrize("N,D,B,mean", CASES)
def test_parity(ctx, N, D, B, mean):
    from pyvbmc_amd.gp import log_marginal_likelihood

    X, y, hyp, _, refs, factors = glh.reference(N, D, B, mean)
    gp = mirror_gp(ctx, X, y, mean)
    dev = log_marginal_likelihood(gp, hyp, grad=True, ctx=ctx)
    host = log_marginal_likelihood(gp, hyp, grad=True, device=False)
    assert dev[0].shape == (B,) and dev[1].shape == hyp.shape
    check_against_both(dev, host, refs, factors, f"N={N} D={D}")
    via_gp = gp.log_likelihood(hyp, grad=True)
    assert np.array_equal(via_gp[0], dev[0]) and np.array_equal(via_gp[1], dev[1])


def test_user_noise(ctx):
    from pyvbmc_amd.gp import log_marginal_likelihood

    N, D, B, mean = 65, 3, 2, gp_ref.MEAN_NEGQUAD
    X, y, hyp, s2, refs, factors = glh.reference(N, D, B, mean, True)
    gp = mirror_gp(ctx, X, y, mean, s2=s2)
    dev = log_marginal_likelihood(gp, hyp, grad=True, ctx=ctx)
    host = log_marginal_likelihood(gp, hyp, grad=True, device=False)
    check_against_both(dev, host, refs, factors, "user noise")


def test_value_only_and_determinism_and_chunks(ctx):
    from pyvbmc_amd.gp import log_marginal_likelihood

    N, D, B, mean = 130, 10, 5, gp_ref.MEAN_NEGQUAD
    X, y, hyp, _, _, _ = glh.reference(N, D, B, mean)
    gp = mirror_gp(ctx, X, y, mean)
    lml, dlml = log_marginal_likelihood(gp, hyp, grad=True, ctx=ctx)
    only = log_marginal_likelihood(gp, hyp, ctx=ctx)  # want_grad = 0
    assert only.shape == (B,) and np.array_equal(only, lml)
    again = log_marginal_likelihood(gp, hyp, grad=True, ctx=ctx)
    assert np.array_equal(again[0], lml) and np.array_equal(again[1], dlml)
    ctx.set_option("gp_lml_chunk", 2)  # chunks of 2 + 2 + 1
    try:
        chunked = log_marginal_likelihood(gp, hyp, grad=True, ctx=ctx)
        chunked_only = log_marginal_likelihood(gp, hyp, ctx=ctx)
    finally:
        ctx.set_option("gp_lml_chunk", 0)
    assert np.array_equal(chunked[0], lml) and np.array_equal(chunked[1], dlml) and np.array_equal(chunked_only, lml)


def bad_batch(hyp, D):
    bad = np.vstack([hyp[0], hyp[1], hyp[1], hyp[2]])
    bad[1, D] = 400.0  # log sf: sf^2 overflows, the covariance is not finite
    return bad


def test_bad_row_in_the_middle(ctx):
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gp import log_marginal_likelihood

    N, D, mean = 130, 10, gp_ref.MEAN_NEGQUAD
    X, y, hyp, _, _, _ = glh.reference(N, D, 5, mean)
    gp = mirror_gp(ctx, X, y, mean)
    bad = bad_batch(hyp, D)
    lml, dlml = log_marginal_likelihood(gp, bad, grad=True, ctx=ctx)
    assert lml[1] == -np.inf and np.all(np.isnan(dlml[1]))
    good = log_marginal_likelihood(gp, bad[[0, 2, 3]], grad=True, ctx=ctx)
    assert np.array_equal(lml[[0, 2, 3]], good[0]) and np.array_equal(dlml[[0, 2, 3]], good[1])
    assert np.all(np.isfinite(good[0])) and np.all(np.isfinite(good[1]))
    assert log_marginal_likelihood(gp, bad, ctx=ctx)[1] == -np.inf
    # the entry point itself: status 1 for that row alone, VBMC_OK
    Xc, yc, hc = _lib.f64(X), _lib.f64(np.ravel(y)), _lib.f64(bad)
    B, P = hc.shape
    sn2 = _lib.f64(np.stack([gp_ref.noise_var(h[D + 1 : D + 2], N) for h in hc]))
    div, dsn2 = _lib.f64(sn2.min(axis=1)), _lib.f64(2 * np.exp(2 * hc[:, D + 1]))
    out, dout, status = np.empty(B), np.empty((B, P)), np.full(B, 7, dtype=np.int32)
    rc = ctx._lib.vbmc_gp_lml(ctx._h, N, D, B, P, mean, _lib.ptr(Xc), _lib.ptr(yc), _lib.ptr(sn2), _lib.ptr(div),
                              _lib.ptr(dsn2), _lib.ptr(hc), 1, _lib.ptr(out), _lib.ptr(dout),
                              status.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0 and list(status) == [0, 1, 0, 0]
    assert np.array_equal(out, lml) and np.array_equal(dout, dlml, equal_nan=True)
    rc = ctx._lib.vbmc_gp_lml(ctx._h, N, D, B, P + 1, mean, _lib.ptr(Xc), _lib.ptr(yc), _lib.ptr(sn2), _lib.ptr(div),
                              _lib.ptr(dsn2), _lib.ptr(hc), 1, _lib.ptr(out), _lib.ptr(dout),
                              status.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == _lib.E_ARG
    div[2] = 5e-7
    rc = ctx._lib.vbmc_gp_lml(ctx._h, N, D, B, P, mean, _lib.ptr(Xc), _lib.ptr(yc), _lib.ptr(sn2), _lib.ptr(div),
                              _lib.ptr(dsn2), _lib.ptr(hc), 1, _lib.ptr(out), _lib.ptr(dout),
                              status.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == _lib.E_UNSUP


def test_installed_gp_survives(ctx, counting):
    from pyvbmc_amd.gp import log_marginal_likelihood

    N, D, S, mean = 65, 3, 2, gp_ref.MEAN_NEGQUAD
    X, y, hyp = gph.make_case(N, D, S, mean, seed=100 + N)
    ogp = gp_ref.make_gp(X, y, hyp, mean)
    gp = mirror_gp(ctx, X, y, mean)
    gp.update(hyp=hyp, device=True)
    xs = points(ogp, 16, 4)
    before = gp.predict(xs, separate_samples=True)
    # another batch, of another N, D and mean
    X2, y2, hyp2, _, _, _ = glh.reference(130, 10, 5, gp_ref.MEAN_NEGQUAD)
    other = mirror_gp(ctx, X2, y2, gp_ref.MEAN_NEGQUAD)
    lml = log_marginal_likelihood(other, hyp2, grad=True, ctx=ctx)[0]
    assert np.all(np.isfinite(lml))
    after = gp.predict(xs, separate_samples=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    lml_bad = log_marginal_likelihood(other, bad_batch(hyp2, 10), grad=True, ctx=ctx)[0]
    assert lml_bad[1] == -np.inf
    after = gp.predict(xs, separate_samples=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert counting.n_set_gp == 0
    # the state is still the device-built one: a point can be appended to it
    gp.append(X[0] + 0.1, 0.5)
    assert gp.X.shape[0] == N + 1 and counting.n_set_gp == 0


def test_unsupported_D_takes_the_host_route(ctx):
    from pyvbmc_amd.gp import log_marginal_likelihood

    N, D, mean = 40, 33, gp_ref.MEAN_CONST
    X, y, hyp = gph.make_case(N, D, 2, mean, seed=100 + N)
    gp = mirror_gp(ctx, X, y, mean)
    dev = log_marginal_likelihood(gp, hyp, grad=True, ctx=ctx)
    host = log_marginal_likelihood(gp, hyp, grad=True, device=False)
    assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])
    assert np.all(np.isfinite(dev[0])) and np.all(np.isfinite(dev[1]))
