"""CPU tests of tests/gp_post_host.py, the NumPy restatement of the device-built GP posterior (csrc/gp_post.hip),
against oracle/gp_ref.make_posterior.

Bounds (derived, not measured):
* residual: for Cholesky in floating point |U^T U - A|_ij <= gamma_{N+1} sqrt(a_ii a_jj), asserted as
  max |U^T U - A| <= (N + 2) eps max_i a_ii;
* entries below the diagonal are exactly zero;
* L and alpha against the oracle: max |dL| <= 4 N eps cond2(A) max |L|, max |dalpha| <= 4 N eps cond2(A) max |alpha|
  (the forward-error law of a Cholesky solve).  The cases include well-conditioned ones, so an indexing error cannot
  hide behind conditioning.
"""
import numpy as np
import pytest

import gp_post_host as gph
from oracle import gp_ref
from test_ais_host import gpcov_gp

# (N, D, S, mean, well conditioned)
CASES = [
    (1, 2, 1, gp_ref.MEAN_ZERO, True),
    (63, 3, 2, gp_ref.MEAN_CONST, True),
    (64, 3, 2, gp_ref.MEAN_NEGQUAD, True),
    (65, 3, 2, gp_ref.MEAN_NEGQUAD, True),
    (130, 10, 3, gp_ref.MEAN_NEGQUAD, True),
    (257, 20, 2, gp_ref.MEAN_NEGQUAD, True),
    (130, 10, 1, gp_ref.MEAN_NEGQUAD, False),
]


def check_sample(st, ref):
    frac = gph.check_factor(st["L"], st["A"])
    f = gph.forward_factor(st["A"])
    e_L = float(np.max(np.abs(st["L"] - ref.L)))
    e_a = float(np.max(np.abs(st["alpha"] - ref.alpha.ravel())))
    print(f"residual {frac:.2f} of bound, cond factor {f:.2e}, dL {e_L / np.max(np.abs(ref.L)):.2e}, "
          f"dalpha {e_a / np.max(np.abs(ref.alpha)):.2e}")
    assert e_L <= f * np.max(np.abs(ref.L))
    assert e_a <= f * np.max(np.abs(ref.alpha))
    assert np.array_equal(st["sW"], ref.sW) and ref.L_chol and ref.sn2_mult == 1.0
    # L^-1 is the inverse: |Linv L - I| within the same law
    assert np.max(np.abs(st["Linv"] @ st["L"] - np.eye(st["L"].shape[0]))) <= max(f, 64 * gph.EPS)
    assert np.all(np.tril(st["Linv"], -1) == 0.0)


@pytest.mark.parametrize("N,D,S,mean,well", CASES)
def test_blocked_factorisation_vs_oracle(N, D, S, mean, well):
    X, y, hyp = gph.make_case(N, D, S, mean, seed=100 + N, well=well)
    for h in hyp:
        check_sample(gph.posterior(h, X, y, mean), gp_ref.make_posterior(h, X, y, mean))


def test_well_conditioned_case_is_well_conditioned():
    X, y, hyp = gph.make_case(130, 10, 1, gp_ref.MEAN_NEGQUAD, seed=230, well=True)
    st = gph.posterior(hyp[0], X, y, gp_ref.MEAN_NEGQUAD)
    assert gph.forward_factor(st["A"]) <= 1e-11  # cond2(A) <= ~90: the bound leaves no room for a misplaced entry


@pytest.mark.parametrize("name", ["homo", "hetero"])
def test_gpcov_fixture_vs_oracle(golden, name):
    c = golden("gpcov")
    ogp = gpcov_gp(c, name)
    for p in ogp.posteriors:
        st = gph.posterior(p.hyp, ogp.X, ogp.y, gp_ref.MEAN_NEGQUAD, s2=ogp.s2, noise_user=ogp.noise_user)
        check_sample(st, p)


def test_not_positive_definite_raises():
    X, y, hyp = gph.make_case(70, 3, 1, gp_ref.MEAN_CONST, seed=7)
    h = hyp[0].copy()
    h[0] = np.nan
    with pytest.raises(np.linalg.LinAlgError):
        gph.posterior(h, X, y, gp_ref.MEAN_CONST)


@pytest.mark.parametrize("N0", [62, 127])
def test_append_equals_fresh_factorisation(N0):
    mean = gp_ref.MEAN_NEGQUAD
    X, y, hyp = gph.make_case(N0 + 4, 3, 1, mean, seed=N0)
    h = hyp[0]
    st = gph.posterior(h, X[:N0], y[:N0], mean)
    for n in range(N0, N0 + 4):
        st = gph.append(st, h, X[:n], X[n], float(y[n, 0]), mean)
    fresh = gph.posterior(h, X, y, mean)
    ref = gp_ref.make_posterior(h, X, y, mean)
    f = gph.forward_factor(fresh["A"])
    for other in (fresh["L"], ref.L):
        e = float(np.max(np.abs(st["L"] - other)) / np.max(np.abs(other)))
        print(f"N {N0} -> {N0 + 4}: dL rel {e:.2e} (bound {f:.2e})")
        assert e <= f
    assert np.max(np.abs(st["alpha"] - ref.alpha.ravel())) <= f * np.max(np.abs(ref.alpha))
    assert np.all(np.tril(st["L"], -1) == 0.0) and np.all(np.tril(st["Linv"], -1) == 0.0)
    st["A"] = fresh["A"]
    gph.check_factor(st["L"], fresh["A"])


# ---- the Python route's host-side decisions (no device) -----------------------------------------------------------
def host_only_gp(c, hyp_name):
    from pyvbmc_amd import _lib
    from pyvbmc_amd import gp as gpm

    gp = gpm.GP(3, gpm.SquaredExponential(), gpm.NegativeQuadratic(), gpm.GaussianNoise(constant_add=True))
    gp.ctx = _lib.Context(-1)
    gp.X, gp.y = c["X"].copy(), c["y"].copy()
    return gp, c[hyp_name]


def test_non_cholesky_sample_routes_to_the_host_path_with_its_bits(golden):
    """A sample with sn2_div < 1e-6 sends the whole call down today's path: decided on the host, before any library call."""
    from pyvbmc_amd.gp import device_posterior

    c = golden("gpcov")
    a, hyp = host_only_gp(c, "tiny_hyp")
    b, _ = host_only_gp(c, "tiny_hyp")
    a.update(hyp=hyp)
    b.update(hyp=hyp, device=True)
    assert [bool(p.L_chol) for p in a.posteriors] == [bool(v) for v in c["tiny_L_chol"]]
    for p, q in zip(a.posteriors, b.posteriors):
        assert np.array_equal(p.L, q.L) and np.array_equal(p.alpha, q.alpha) and np.array_equal(p.sW, q.sW)
    d, _ = host_only_gp(c, "tiny_hyp")
    assert device_posterior(d, hyp, ctx=d.ctx) is False and d.posteriors is None


def test_device_route_needs_a_device(golden):
    from pyvbmc_amd import _lib

    gp, hyp = host_only_gp(golden("gpcov"), "homo_hyp")
    with pytest.raises(_lib.NoDeviceError):
        gp.update(hyp=hyp, device=True)  # no quiet fall-back to the host when the device route applies


def test_fingerprint_handles_records_without_L(golden):
    from types import SimpleNamespace

    from pyvbmc_amd.gp import _gp_fingerprint

    gp, hyp = host_only_gp(golden("gpcov"), "homo_hyp")
    gp.update(hyp=hyp)
    full, _ = _gp_fingerprint(gp)
    for p in gp.posteriors:
        p.L = None
    bare, _ = _gp_fingerprint(gp)
    assert bare != full
    assert bare == _gp_fingerprint(gp)[0]
    gp.posteriors[0] = SimpleNamespace(**vars(gp.posteriors[0]))  # another record with equal contents: another key
    assert _gp_fingerprint(gp)[0] != bare
