"""``gp.reinstall`` on the device: a fitted GP that went through a pickle is put back into ANOTHER context exactly as the
device had built it -- ``alpha`` and ``L`` fetched from there equal the records bit for bit -- so that a one-point append
on the copy gives the bits of the same append on the original.  This is the device half of the exact resume of a
checkpointed VBMC run (pyvbmc_amd/vbmc.py).

Shapes: D = 2, negative-quadratic mean, ``GP.fit(optimizer="fused")``; N = 20 (one 64-block of the factorisation) and
N = 70 (two blocks: the smallest N where its panel and trailing update run); S = 1 (the optimum alone) and S = 4 (slice
samples); constant noise and per-point ``s2``.
"""
import logging
import pickle
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, P = 2, 9
LB = np.array([-3.0, -3.0, -3.0, -4.0, -5.0, -3.0, -3.0, -2.0, -2.0])
UB = np.array([3.0, 3.0, 3.0, 0.0, 5.0, 3.0, 3.0, 3.0, 3.0])
X_NEW, Y_NEW, S2_NEW = np.array([0.31, -0.42]), -0.17, 0.5


@pytest.fixture(scope="module")
def ctxs():
    from pyvbmc_amd import _lib

    a, b = _lib.Context(0), _lib.Context(0)
    yield a, b
    a.close()
    b.close()


def fitted(ctx, N, S, noisy):
    """A quadratic plus a small fixed perturbation, fitted on ``ctx``: the posterior stays installed there."""
    from pyvbmc_amd import gp as gpm

    rng = np.random.default_rng(100 * N + S)
    X = 1.5 * rng.standard_normal((N, D))
    y = -0.5 * np.sum((X / np.array([1.0, 2.0])) ** 2, axis=1, keepdims=True) + 0.05 * rng.standard_normal((N, 1))
    s2 = 0.01 + 0.04 * rng.random((N, 1)) if noisy else None
    gp = gpm.GP(D, gpm.SquaredExponential(), gpm.NegativeQuadratic(), gpm.GaussianNoise(constant_add=True, user_provided_add=noisy))
    gp.ctx = ctx
    gp.set_bounds({"lb": LB, "ub": UB})
    opts = {"init_N": 32, "opts_N": 1, "n_samples": 0 if S == 1 else S, "thin": 1, "burn": 2, "tol_opt": 1e-3}
    hyp, _, _ = gp.fit(X, y, s2, hyp0=0.5 * (LB + UB)[None, :], options=opts, seed=11, optimizer="fused")
    assert hyp.shape == (S, P) and ctx._gp_dev is not None
    return gp


def fetch(ctx, S, N):
    from pyvbmc_amd import _lib

    alpha, L = np.empty((S, N)), np.empty((S, N, N))
    ctx.check(ctx._lib.vbmc_gp_fetch(ctx._h, _lib.ptr(alpha), _lib.ptr(L)))
    return alpha, L


def same_records(a, b):
    return len(a.posteriors) == len(b.posteriors) and all(
        np.array_equal(p.alpha, q.alpha) and np.array_equal(p.L, q.L) and np.array_equal(p.hyp, q.hyp)
        for p, q in zip(a.posteriors, b.posteriors))


def reinstalled_copy(gp, ctx2, caplog):
    """``gp`` through a pickle and installed again on ``ctx2``: exact, and nothing logged."""
    from pyvbmc_amd import gp as gpm

    copy = pickle.loads(pickle.dumps(gp))
    assert copy._ctx is None and same_records(gp, copy)
    held = [(p.alpha, p.L) for p in copy.posteriors]
    with caplog.at_level(logging.WARNING):
        assert gpm.reinstall(copy, ctx=ctx2) is True
    assert not [r for r in caplog.records if "bit-exact" in r.getMessage()]
    assert all(p.alpha is a and p.L is L for p, (a, L) in zip(copy.posteriors, held))  # the records' arrays stay
    assert ctx2._gp_dev is not None
    S, N = len(copy.posteriors), copy.X.shape[0]
    alpha, L = fetch(ctx2, S, N)
    for s, p in enumerate(copy.posteriors):
        assert np.array_equal(alpha[s], p.alpha.ravel()) and np.array_equal(L[s], p.L)
    return copy


def append_both(gp, copy, ctx1, ctx2, noisy):
    """The same point appended to the original on its context and to the copy on the other: the same bits, and both by
    extending the resident state (N + 1 points, still device-built)."""
    from pyvbmc_amd import gp as gpm

    N = gp.X.shape[0]
    gpm.append_point(gp, X_NEW, Y_NEW, S2_NEW if noisy else None, ctx=ctx1)
    gpm.append_point(copy, X_NEW, Y_NEW, S2_NEW if noisy else None, ctx=ctx2)
    assert gp.X.shape[0] == copy.X.shape[0] == N + 1 and ctx1._gp_dev is not None and ctx2._gp_dev is not None
    assert same_records(gp, copy)
    assert [p.sn2_div for p in gp.posteriors] == [p.sn2_div for p in copy.posteriors]


@pytest.mark.parametrize("noisy", [False, True], ids=["const", "s2"])
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("N", [20, 70])
def test_fit_reinstall_append(ctxs, caplog, N, S, noisy):
    ctx1, ctx2 = ctxs
    gp = fitted(ctx1, N, S, noisy)
    assert all(hasattr(p, "sn2_div") and hasattr(p, "sn2_const") for p in gp.posteriors)
    copy = reinstalled_copy(gp, ctx2, caplog)
    append_both(gp, copy, ctx1, ctx2, noisy)


@pytest.mark.parametrize("noisy", [False, True], ids=["const", "s2"])
@pytest.mark.parametrize("N,S", [(20, 4), (70, 1)])
def test_reupdate_reinstall_append(ctxs, caplog, N, S, noisy):
    """The other build that can be live at an iteration's end: ``reupdate`` on a trimmed set (five rows dropped), whose
    noise scalars are the host's."""
    from pyvbmc_amd import gp as gpm

    ctx1, ctx2 = ctxs
    gp = fitted(ctx1, N, S, noisy)
    flag = np.ones(N, dtype=bool)
    flag[[1, 4, 9, 13, 17]] = False
    log = SimpleNamespace(X=gp.X, y=gp.y.ravel(), X_flag=flag, n_evals=np.ones(N), noise_flag=noisy)
    if noisy:
        log.S = np.sqrt(gp.s2.ravel())
    gp = gpm.reupdate(log, gp, ctx=ctx1)
    assert gp.X.shape[0] == N - 5 and ctx1._gp_dev is not None
    assert all(hasattr(p, "sn2_div") and not hasattr(p, "sn2_const") for p in gp.posteriors)
    copy = reinstalled_copy(gp, ctx2, caplog)
    append_both(gp, copy, ctx1, ctx2, noisy)


@pytest.mark.parametrize("N", [20, 70])
def test_without_sn2_div_falls_back(ctxs, caplog, N):
    """Records of another maker: uploaded as saved (the host-installed route that exists), one warning, False."""
    from pyvbmc_amd import gp as gpm

    ctx1, ctx2 = ctxs
    gp = fitted(ctx1, N, 4, False)
    copy = pickle.loads(pickle.dumps(gp))
    for p in copy.posteriors:
        del p.sn2_div
    with caplog.at_level(logging.WARNING):
        assert gpm.reinstall(copy, ctx=ctx2) is False
    assert len([r for r in caplog.records if "bit-exact" in r.getMessage()]) == 1
    assert ctx2._gp_dev is None and ctx2._gp_key is not None
    xs = np.random.default_rng(2).standard_normal((50, D))
    mu1, s1 = gp.predict(xs, ctx=ctx1)
    mu2, s2 = copy.predict(xs, ctx=ctx2)
    assert np.allclose(mu1, mu2, rtol=1e-12, atol=0) and np.allclose(s1, s2, rtol=1e-12, atol=0)
