"""CPU tests of the GP log marginal likelihood: the host route of pyvbmc_amd.gp.log_marginal_likelihood
(``device=False``) and the float64 restatement against the longdouble restatement of tests/gp_lml_host.py, within the
derived bounds stated there (f = 4 N eps cond2(A) times the absolute-term sums); the analytic gradient against central
differences of the longdouble value; the noise rules, the non-finite row, the non-Cholesky rows and the routing without
a device."""
import numpy as np
import pytest

import gp_lml_host as glh
import gp_post_host as gph
from oracle import gp_ref

# the cases the bounds were stated on, and a zero-mean one so that all three mean kinds are covered
HOST_CASES = glh.CASES + [(64, 3, 2, gp_ref.MEAN_ZERO)]


def mirror_gp(X, y, mean, s2=None, constant_add=True):
    from pyvbmc_amd import _lib
    from pyvbmc_amd import gp as gpm

    cls = {gp_ref.MEAN_ZERO: gpm.ZeroMean, gp_ref.MEAN_CONST: gpm.ConstantMean, gp_ref.MEAN_NEGQUAD: gpm.NegativeQuadratic}
    gp = gpm.GP(X.shape[1], gpm.SquaredExponential(), cls[mean](),
                gpm.GaussianNoise(constant_add=constant_add, user_provided_add=s2 is not None))
    gp.ctx = _lib.Context(-1)
    gp.X, gp.y = np.array(X, dtype=np.float64), np.array(y, dtype=np.float64).reshape(-1, 1)
    gp.s2 = None if s2 is None else np.array(s2, dtype=np.float64).reshape(-1, 1)
    return gp


@pytest.mark.parametrize("N,D,S,mean", HOST_CASES)
def test_host_route_and_float64_restatement_within_bounds(N, D, S, mean):
    from pyvbmc_amd.gp import log_marginal_likelihood

    X, y, hyp, _, refs, factors = glh.reference(N, D, S, mean)
    gp = mirror_gp(X, y, mean)
    lml, dlml = log_marginal_likelihood(gp, hyp, grad=True, device=False)
    only = log_marginal_likelihood(gp, hyp, device=False)
    assert lml.shape == (S,) and dlml.shape == hyp.shape and np.array_equal(only, lml)
    for s in range(S):
        glh.check_within(lml[s], dlml[s], refs[s], factors[s], f"host route N={N} D={D} s={s}")
        r64 = glh.lml_and_grad(hyp[s], X, y, mean, dtype=np.float64)
        glh.check_within(r64["lml"], r64["grad"], refs[s], factors[s], f"float64 restatement N={N} D={D} s={s}")
    via_gp = gp.log_likelihood(hyp, grad=True, device=False)
    assert np.array_equal(via_gp[0], lml) and np.array_equal(via_gp[1], dlml)


@pytest.mark.parametrize("mean", [gp_ref.MEAN_ZERO, gp_ref.MEAN_CONST, gp_ref.MEAN_NEGQUAD])
def test_gradient_is_the_derivative_of_the_value(mean):
    N, D = 63, 3
    X, y, hyp = gph.make_case(N, D, 1, mean, seed=100 + N)
    h0 = hyp[0].astype(np.longdouble)
    ref = glh.lml_and_grad(h0, X, y, mean, dtype=np.longdouble)
    step = np.longdouble(1e-4)
    fd = np.zeros(h0.size, dtype=np.longdouble)
    for p in range(h0.size):
        hp, hm = h0.copy(), h0.copy()
        hp[p] += step
        hm[p] -= step
        fd[p] = (_value_ld(hp, X, y, mean) - _value_ld(hm, X, y, mean)) / (2 * step)
    err = float(np.max(np.abs(fd - ref["grad"])) / np.max(np.abs(ref["grad"])))
    print(f"mean kind {mean}: central differences within {err:.2e} of max |grad|")
    assert err <= 1e-6


def _value_ld(h, X, y, mean):
    """The longdouble value at a longdouble hyper-parameter vector (lml_and_grad rounds its input to float64)."""
    N, D = X.shape
    Xl, yl = X.astype(np.longdouble), np.ravel(y).astype(np.longdouble)
    sn2 = np.exp(2 * h[D + 1])
    Xs = Xl / np.exp(h[:D])
    K = np.exp(2 * h[D]) * np.exp(-np.sum((Xs[:, None, :] - Xs[None, :, :]) ** 2, axis=2) / 2)
    U = glh.cholesky_upper(K / sn2 + np.eye(N, dtype=np.longdouble))
    m, _ = glh.mean_and_grad(mean, h[D + 2 :], Xl)
    r = yl - m
    Ui = glh.upper_inverse(U)
    alpha = (Ui @ (Ui.T @ r)) / sn2
    return -(r @ alpha) / 2 - np.sum(np.log(np.diag(U))) - N * np.log(2 * np.arccos(np.longdouble(-1)) * sn2) / 2


def test_noise_rules():
    from pyvbmc_amd.gp import log_marginal_likelihood

    N, D, S, mean = 65, 3, 2, gp_ref.MEAN_NEGQUAD
    X, y, hyp, s2, refs, factors = glh.reference(N, D, S, mean, True)
    # user-provided s2 on top of the constant: sn2_div changes and the value follows
    gp = mirror_gp(X, y, mean, s2=s2)
    lml, dlml = log_marginal_likelihood(gp, hyp, grad=True, device=False)
    for s in range(S):
        glh.check_within(lml[s], dlml[s], refs[s], factors[s], f"user noise s={s}")
    plain = log_marginal_likelihood(mirror_gp(X, y, mean), hyp, device=False)
    assert np.all(plain != lml)
    # without the constant part the noise parameter does nothing: zero derivative, a value that ignores it
    s2_big = s2 + 0.05
    gp0 = mirror_gp(X, y, mean, s2=s2_big, constant_add=False)
    l0, d0 = log_marginal_likelihood(gp0, hyp, grad=True, device=False)
    assert np.all(d0[:, D + 1] == 0.0) and np.all(np.isfinite(l0)) and np.all(np.isfinite(d0))
    moved = hyp.copy()
    moved[:, D + 1] += 0.7
    l1, d1 = log_marginal_likelihood(gp0, moved, grad=True, device=False)
    assert np.array_equal(l0, l1) and np.array_equal(d0, d1)


def test_non_finite_row_gives_minus_inf_and_nan():
    from pyvbmc_amd.gp import log_marginal_likelihood

    N, D, S, mean = 63, 3, 2, gp_ref.MEAN_CONST
    X, y, hyp, _, refs, factors = glh.reference(N, D, S, mean)
    bad = np.vstack([hyp[0], hyp[1], hyp[1]])
    bad[1, D] = 400.0  # log sf: sf^2 overflows
    lml, dlml = log_marginal_likelihood(mirror_gp(X, y, mean), bad, grad=True, device=False)
    assert lml[1] == -np.inf and np.all(np.isnan(dlml[1]))
    good = log_marginal_likelihood(mirror_gp(X, y, mean), hyp, grad=True, device=False)
    assert np.array_equal(lml[[0, 2]], good[0]) and np.array_equal(dlml[[0, 2]], good[1])
    assert log_marginal_likelihood(mirror_gp(X, y, mean), bad, device=False)[1] == -np.inf


def test_rows_below_the_cholesky_threshold_take_the_host_branch():
    """sn2_div < 1e-6: computed on the host even with device=True (here on a context without a device, which any
    library call would refuse)."""
    from pyvbmc_amd.gp import log_marginal_likelihood

    N, D, mean = 63, 3, gp_ref.MEAN_CONST
    X, y, hyp = gph.make_case(N, D, 2, mean, seed=100 + N)
    hyp = hyp.copy()
    hyp[:, D + 1] = np.log(5e-4)  # sn2 = 2.5e-7
    gp = mirror_gp(X, y, mean)
    lml, dlml = log_marginal_likelihood(gp, hyp, grad=True, device=True)
    host = log_marginal_likelihood(gp, hyp, grad=True, device=False)
    assert np.array_equal(lml, host[0]) and np.array_equal(dlml, host[1])
    assert np.all(np.isfinite(lml)) and np.all(np.isfinite(dlml))
    for s in range(2):
        ref = glh.lml_and_grad(hyp[s], X, y, mean, dtype=np.longdouble)
        glh.check_within(lml[s], dlml[s], ref, glh.factor_of(hyp[s], X), f"sn2_div < 1e-6 s={s}")


def test_device_route_needs_a_device():
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gp import log_marginal_likelihood

    X, y, hyp, _, _, _ = glh.reference(63, 3, 2, gp_ref.MEAN_CONST)
    gp = mirror_gp(X, y, gp_ref.MEAN_CONST)
    with pytest.raises(_lib.NoDeviceError):
        log_marginal_likelihood(gp, hyp, grad=True)
    with pytest.raises(_lib.NoDeviceError):
        gp.log_likelihood(hyp)


def test_exported_names_and_abi():
    import pyvbmc_amd
    from pyvbmc_amd import _lib

    assert pyvbmc_amd.log_marginal_likelihood is pyvbmc_amd.gp.log_marginal_likelihood
    assert pyvbmc_amd.GP is pyvbmc_amd.gp.GP
    assert "vbmc_gp_lml" in _lib.SIGNATURES and _lib.T_GP_LML == 8
    assert _lib.load().vbmc_abi_version() == 2
