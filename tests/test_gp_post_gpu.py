"""GPU tests of the device-built GP posterior: vbmc_gp_posterior / vbmc_gp_append / vbmc_gp_fetch (csrc/gp_post.hip,
csrc/api_gp_post.hip) and their Python route (pyvbmc_amd.gp.device_posterior, GP.update(device=True), GP.append,
fetch_posteriors), against oracle/gp_ref.make_posterior and tests/gp_post_host.py.

Bounds are the derived ones of tests/test_gp_post_host.py: residual (N + 2) eps max a_ii, exact zeros below the
diagonal, L / alpha within 4 N eps cond2(A) of the oracle, predict within max(1e-10, 4 N eps cond2(A)) sf^2 (1e-10 sf^2
is the project's predict bound), and the device against the NumPy restatement of its own algorithm to 64 eps max |L| on
the well-conditioned cases (same algorithm, only the rounding inside the products differs); alpha against the restatement
to 8 N eps max |alpha| (it pins the two triangular matrix-vector kernels to the restatement as well).
"""
from functools import lru_cache

import numpy as np
import pytest

import gp_post_host as gph
from helpers import PlainGP, PlainVP, oracle_gp, rel_err
from oracle import gp_ref
from test_ais_host import gpcov_gp

pytestmark = pytest.mark.gpu

# (N, D, S, mean): 63 / 64 / 65 on the block edge, 130 = three block steps with a remainder of 2, 257 = five with a
# remainder of 1 and a padded D
BUILD_CASES = [
    (1, 2, 1, gp_ref.MEAN_ZERO),
    (63, 3, 2, gp_ref.MEAN_CONST),
    (64, 3, 2, gp_ref.MEAN_NEGQUAD),
    (65, 3, 2, gp_ref.MEAN_NEGQUAD),
    (130, 10, 3, gp_ref.MEAN_NEGQUAD),
    (257, 20, 2, gp_ref.MEAN_NEGQUAD),
]


class CountingLib:
    """The library handle with the calls that upload a GP counted."""

    def __init__(self, lib):
        self._lib_real, self.n_set_gp = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib_real, name)
        if name == "vbmc_set_gp":
            self.n_set_gp += 1
        return fn


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


@lru_cache(maxsize=None)
def case(N, D, S, mean):
    """Data, the oracle's GP and the conditioning factor of every sample, computed once per case."""
    X, y, hyp = gph.make_case(N, D, S, mean, seed=100 + N)
    ogp = gp_ref.make_gp(X, y, hyp, mean)
    return X, y, hyp, ogp, sample_factors(ogp)


def sample_factors(ogp):
    out = []
    for p in ogp.posteriors:
        sn2, sn2_div, sl = gph.noise_scalars(p.hyp, ogp.X.shape[0], ogp.D, ogp.s2, ogp.noise_user)
        A = gph.cov_matrix(p.hyp, ogp.X, sn2, sn2_div, sl)
        out.append((A, gph.forward_factor(A)))
    return out


def mirror_gp(ctx, X, y, mean, s2=None):
    from pyvbmc_amd import gp as gpm

    cls = {gp_ref.MEAN_ZERO: gpm.ZeroMean, gp_ref.MEAN_CONST: gpm.ConstantMean, gp_ref.MEAN_NEGQUAD: gpm.NegativeQuadratic}
    gp = gpm.GP(X.shape[1], gpm.SquaredExponential(), cls[mean](),
                gpm.GaussianNoise(constant_add=True, user_provided_add=s2 is not None))
    gp.ctx = ctx
    gp.X, gp.y = np.array(X, dtype=np.float64), np.array(y, dtype=np.float64).reshape(-1, 1)
    gp.s2 = None if s2 is None else np.array(s2, dtype=np.float64).reshape(-1, 1)
    return gp


def sf2_of(hyp, D):
    return float(np.max(np.exp(2 * np.atleast_2d(hyp)[:, D])))


def check_records(posts, ogp, factors, what, host=None):
    for s, (p, ref, (A, f)) in enumerate(zip(posts, ogp.posteriors, factors)):
        frac = gph.check_factor(p.L, A)
        e_L = float(np.max(np.abs(p.L - ref.L)) / np.max(np.abs(ref.L)))
        e_a = float(np.max(np.abs(p.alpha - ref.alpha)) / np.max(np.abs(ref.alpha)))
        msg = f"{what} s={s}: residual {frac:.2f} of bound, factor {f:.2e}, dL {e_L:.2e}, dalpha {e_a:.2e}"
        assert p.alpha.shape == ref.alpha.shape and p.L.shape == ref.L.shape
        if host is not None:
            e_h = float(np.max(np.abs(p.L - host[s]["L"])) / np.max(np.abs(host[s]["L"])))
            e_ha = float(np.max(np.abs(p.alpha.ravel() - host[s]["alpha"])) / np.max(np.abs(host[s]["alpha"])))
            msg += f", vs host restatement L {e_h / gph.EPS:.1f} eps, alpha {e_ha / gph.EPS:.1f} eps"
        print(msg)
        assert e_L <= f and e_a <= f
        assert np.array_equal(p.sW, ref.sW) and p.L_chol is True and p.sn2_mult == 1.0
        assert np.array_equal(p.hyp, ref.hyp)
        if host is not None:
            assert e_h <= 64 * gph.EPS
            # alpha = L^-1 (L^-T r) / sl: two sums of up to N terms over an L^-1 that itself differs by rounding; 8 N eps
            # of max |alpha| covers both sums' reordering at these condition numbers (<= ~200)
            assert e_ha <= 8 * p.L.shape[0] * gph.EPS


def predict_bound(factors, sf2):
    return max(1e-10, max(f for _, f in factors)) * sf2


def check_predict(gp, ogp, factors, xs, what):
    D = ogp.D
    sf2 = sf2_of(np.stack([p.hyp for p in ogp.posteriors]), D)
    fmu, fs2 = gp.predict(xs, separate_samples=True)
    omu, os2 = gp_ref.predict(ogp, xs, separate_samples=True)
    e_m, e_v = float(np.max(np.abs(fmu - omu))), float(np.max(np.abs(fs2 - os2)))
    b = predict_bound(factors, sf2)
    print(f"{what}: predict dmu {e_m:.2e}, ds2 {e_v:.2e}, bound {b:.2e}")
    assert e_m <= b and e_v <= b
    return fmu, fs2


def points(ogp, M, seed):
    rng = np.random.default_rng(seed)
    return ogp.X[rng.integers(0, ogp.X.shape[0], M)] + 0.3 * rng.standard_normal((M, ogp.D))


# ------------------------------------------------------------------------------------------------- 1. build parity
@pytest.mark.parametrize("N,D,S,mean", BUILD_CASES)
def test_build_parity(ctx, N, D, S, mean):
    from pyvbmc_amd.gp import device_posterior

    X, y, hyp, ogp, factors = case(N, D, S, mean)
    gp = mirror_gp(ctx, X, y, mean)
    assert device_posterior(gp, hyp, ctx=ctx) is True
    host = [gph.posterior(h, X, y, mean) for h in hyp]
    check_records(gp.posteriors, ogp, factors, f"N={N} D={D}", host=host)
    # the host route's records for the same data: sW, L_chol, sn2_mult exactly
    ref = mirror_gp(ctx, X, y, mean)
    ref.update(hyp=hyp)
    for p, q in zip(gp.posteriors, ref.posteriors):
        assert np.array_equal(p.sW, q.sW) and p.L_chol == q.L_chol and p.sn2_mult == q.sn2_mult


@pytest.mark.parametrize("name", ["homo", "hetero"])
def test_build_parity_gpcov(ctx, golden, name):
    from pyvbmc_amd.gp import device_posterior

    ogp = gpcov_gp(golden("gpcov"), name)
    gp = PlainGP(ogp)  # attribute-only duck type: no noise object, user noise through s2
    hyp = np.stack([p.hyp for p in ogp.posteriors])
    assert device_posterior(gp, hyp, ctx=ctx) is True
    check_records(gp.posteriors, ogp, sample_factors(ogp), name)


# ---------------------------------------------------------------------------- 2. the installed state is what consumers read
@pytest.mark.parametrize("fetch", [True, False])
def test_installed_state_serves_predict_without_upload(ctx, counting, fetch):
    from pyvbmc_amd.gp import device_posterior, fetch_posteriors, upload_gp

    N, D, S, mean = 130, 10, 3, gp_ref.MEAN_NEGQUAD
    X, y, hyp, ogp, factors = case(N, D, S, mean)
    gp = mirror_gp(ctx, X, y, mean)
    assert device_posterior(gp, hyp, ctx=ctx, fetch=fetch)
    assert all((p.L is None) != fetch for p in gp.posteriors)
    upload_gp(gp, ctx)
    check_predict(gp, ogp, factors, points(ogp, 96, 5), f"fetch={fetch}")
    assert counting.n_set_gp == 0
    if not fetch:
        full = mirror_gp(ctx, X, y, mean)
        assert device_posterior(full, hyp, ctx=ctx, fetch=True)
        assert device_posterior(gp, hyp, ctx=ctx, fetch=False)
        posts = fetch_posteriors(gp, ctx)
        for p, q in zip(posts, full.posteriors):
            assert np.array_equal(p.L, q.L) and np.array_equal(p.alpha, q.alpha)
        gp.predict(points(ogp, 8, 6))
        assert counting.n_set_gp == 0


def test_records_without_L_are_rebuilt_when_the_context_moved_on(ctx, counting):
    from pyvbmc_amd.gp import device_posterior

    X, y, hyp, ogp, factors = case(65, 3, 2, gp_ref.MEAN_NEGQUAD)
    X2, y2, hyp2, ogp2, factors2 = case(63, 3, 2, gp_ref.MEAN_CONST)
    a = mirror_gp(ctx, X, y, gp_ref.MEAN_NEGQUAD)
    b = mirror_gp(ctx, X2, y2, gp_ref.MEAN_CONST)
    assert device_posterior(a, hyp, ctx=ctx, fetch=False)
    xs = points(ogp, 16, 1)
    before = a.predict(xs, separate_samples=True)
    assert device_posterior(b, hyp2, ctx=ctx, fetch=False)
    check_predict(b, ogp2, factors2, points(ogp2, 16, 2), "b")
    after = a.predict(xs, separate_samples=True)  # (a's records carry no L: built again on the device)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert counting.n_set_gp == 0


@pytest.mark.parametrize("fetch", [True, False])
def test_installed_state_serves_gp_log_joint(ctx, golden, counting, fetch):
    from pyvbmc_amd.gp import device_posterior
    from pyvbmc_amd.variational_optimization import _gp_log_joint

    g = golden("c1")
    ogp = oracle_gp(g)
    gp = PlainGP(ogp)
    assert device_posterior(gp, g["hyp"], ctx=ctx, fetch=fetch)
    vp = PlainVP(g)
    G, dG, varG, _, var_ss, I_sk, J_sjk = _gp_log_joint(vp, gp, False, True, True, True, True)
    assert counting.n_set_gp == 0
    sf2 = sf2_of(g["hyp"], int(g["D"]))
    assert abs(G - g["glj_SM_var_G"]) <= 1e-10 * abs(G)
    assert rel_err(I_sk, g["glj_SM_I_sk"]) < 1e-10
    e_J = float(np.max(np.abs(J_sjk - g["glj_SM_J_sjk"])))
    e_v = float(np.max(np.abs(np.ravel(varG) - np.ravel(g["glj_SM_varG"]))))
    e_ss = abs(var_ss - g["glj_SM_var_ss"])
    print(f"glj fetch={fetch}: dJ {e_J / sf2:.2e} sf2, dvarG {e_v / sf2:.2e} sf2, dvar_ss {e_ss / sf2:.2e} sf2")
    assert e_J <= 1e-10 * sf2 and e_v <= 1e-10 * sf2 and e_ss <= 1e-10 * sf2


# ------------------------------------------------------------------------------------------------------- 3. append
@pytest.mark.parametrize("N0,n_add", [(62, 4), (127, 3)])
@pytest.mark.parametrize("fetch", [True, False])
def test_append(ctx, counting, N0, n_add, fetch):
    from pyvbmc_amd.gp import device_posterior, fetch_posteriors, upload_gp

    mean, D, S = gp_ref.MEAN_NEGQUAD, 3, 2
    X, y, hyp = gph.make_case(N0 + n_add, D, S, mean, seed=N0)
    gp = mirror_gp(ctx, X[:N0], y[:N0], mean)
    assert device_posterior(gp, hyp, ctx=ctx, fetch=fetch)
    for n in range(N0, N0 + n_add):
        gp.append(X[n], y[n, 0], fetch=fetch)
        assert gp.X.shape == (n + 1, D) and gp.y.shape == (n + 1, 1)
        ogp = gp_ref.make_gp(X[: n + 1], y[: n + 1], hyp, mean)
        factors = sample_factors(ogp)
        upload_gp(gp, ctx)
        check_predict(gp, ogp, factors, points(ogp, 24, n), f"N={n + 1}")
    assert counting.n_set_gp == 0
    xs = points(ogp, 24, 99)
    fetch_posteriors(gp, ctx)
    fmu, fs2 = gp.predict(xs, separate_samples=True)
    assert counting.n_set_gp == 0  # (appended, fetched, predicted: the GP never went up through vbmc_set_gp)
    check_records(gp.posteriors, ogp, factors, f"appended {N0}->{N0 + n_add}")
    fresh = mirror_gp(ctx, X, y, mean)
    assert device_posterior(fresh, hyp, ctx=ctx)
    fmu_f, fs2_f = fresh.predict(xs, separate_samples=True)
    sf2 = sf2_of(hyp, D)
    for s, (p, q, (A, f)) in enumerate(zip(gp.posteriors, fresh.posteriors, factors)):
        assert np.max(np.abs(p.L - q.L)) <= f * np.max(np.abs(q.L))
        assert np.max(np.abs(p.alpha - q.alpha)) <= f * np.max(np.abs(q.alpha))
    b = predict_bound(factors, sf2)
    assert np.max(np.abs(fs2 - fs2_f)) <= b and np.max(np.abs(fmu - fmu_f)) <= b


# --------------------------------------------------------------------------------------------- 4. routing and errors
def test_non_cholesky_sample_takes_the_host_path(ctx, golden):
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gp import device_posterior

    c = golden("gpcov")
    hyp = c["tiny_hyp"]
    assert list(c["tiny_L_chol"]) != [1, 1]
    a = mirror_gp(ctx, c["X"], c["y"], gp_ref.MEAN_NEGQUAD)
    b = mirror_gp(ctx, c["X"], c["y"], gp_ref.MEAN_NEGQUAD)
    a.update(hyp=hyp)
    b.update(hyp=hyp, device=True)
    for p, q in zip(a.posteriors, b.posteriors):
        assert np.array_equal(p.L, q.L) and np.array_equal(p.alpha, q.alpha) and np.array_equal(p.sW, q.sW)
        assert p.L_chol == q.L_chol and p.sn2_mult == q.sn2_mult
    assert device_posterior(mirror_gp(ctx, c["X"], c["y"], gp_ref.MEAN_NEGQUAD), hyp, ctx=ctx) is False
    # the entry point itself
    X, y = _lib.f64(c["X"]), _lib.f64(np.ravel(c["y"]))
    N, D = X.shape
    S, P = hyp.shape
    sn2 = _lib.f64(np.stack([gp_ref.noise_var(h[D + 1 : D + 2], N) for h in hyp]))
    div = _lib.f64(sn2.min(axis=1))
    alpha = np.empty((S, N))
    rc = ctx._lib.vbmc_gp_posterior(ctx._h, N, D, S, P, gp_ref.MEAN_NEGQUAD, _lib.ptr(X), _lib.ptr(y), _lib.ptr(sn2),
                                    _lib.ptr(div), _lib.ptr(_lib.f64(hyp)), _lib.ptr(alpha), None)
    assert rc == _lib.E_UNSUP
    rc = ctx._lib.vbmc_gp_posterior(ctx._h, N, D, S, P + 1, gp_ref.MEAN_NEGQUAD, _lib.ptr(X), _lib.ptr(y), _lib.ptr(sn2),
                                    _lib.ptr(div), _lib.ptr(_lib.f64(hyp)), _lib.ptr(alpha), None)
    assert rc == _lib.E_ARG


def test_not_positive_definite_leaves_the_installed_state(ctx, counting):
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gp import device_posterior

    X, y, hyp, ogp, factors = case(65, 3, 2, gp_ref.MEAN_NEGQUAD)
    good = mirror_gp(ctx, X, y, gp_ref.MEAN_NEGQUAD)
    assert device_posterior(good, hyp, ctx=ctx)
    xs = points(ogp, 32, 3)
    before = good.predict(xs, separate_samples=True)
    bad_hyp = hyp.copy()
    bad_hyp[1, 0] = np.nan  # a length scale: the noise scalars stay finite, the covariance does not
    bad = mirror_gp(ctx, X, y, gp_ref.MEAN_NEGQUAD)
    with pytest.raises(np.linalg.LinAlgError):
        device_posterior(bad, bad_hyp, ctx=ctx)
    assert bad.posteriors is None
    with pytest.raises(np.linalg.LinAlgError):
        bad.update(hyp=bad_hyp, device=True)
    after = good.predict(xs, separate_samples=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # a failed append: a point whose coordinates are not finite
    with pytest.raises(np.linalg.LinAlgError):
        good.append(np.full(3, np.nan), 0.0)
    assert good.X.shape[0] == 65 and len(good.posteriors[0].alpha) == 65
    rc = ctx._lib.vbmc_gp_append(ctx._h, _lib.ptr(np.full(3, np.nan)), 0.0, None, None)
    assert rc == _lib.E_NOTPD
    after = good.predict(xs, separate_samples=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert counting.n_set_gp == 0


def test_append_needs_a_device_built_posterior(ctx):
    from pyvbmc_amd import _lib

    X, y, hyp, ogp, factors = case(63, 3, 2, gp_ref.MEAN_CONST)
    gp = mirror_gp(ctx, X, y, gp_ref.MEAN_CONST)
    gp.update(hyp=hyp)  # host route
    gp.predict(X[:4])   # uploaded through vbmc_set_gp
    rc = ctx._lib.vbmc_gp_append(ctx._h, _lib.ptr(_lib.f64(X[0] + 0.1)), 0.5, None, None)
    assert rc == _lib.E_ARG
    # the Python route then updates on the extended data instead
    gp.append(X[0] + 0.1, 0.5)
    assert gp.X.shape[0] == 64 and gp.posteriors[0].L.shape == (64, 64)
    ogp1 = gp_ref.make_gp(gp.X, gp.y, hyp, gp_ref.MEAN_CONST)
    check_records(gp.posteriors, ogp1, sample_factors(ogp1), "append without a resident device posterior")
    # user noise: the resident state is not appendable
    c_s2 = 0.01 + 0.02 * np.random.default_rng(1).random((63, 1))
    het = mirror_gp(ctx, X, y, gp_ref.MEAN_CONST, s2=c_s2)
    het.update(hyp=hyp, device=True)
    rc = ctx._lib.vbmc_gp_append(ctx._h, _lib.ptr(_lib.f64(X[0] + 0.1)), 0.5, None, None)
    assert rc == _lib.E_UNSUP


# --------------------------------------------------------------------------------------------- 5. reproducibility
def test_bit_reproducible(ctx):
    from pyvbmc_amd.gp import device_posterior

    mean = gp_ref.MEAN_NEGQUAD
    X, y, hyp = gph.make_case(131, 10, 3, mean, seed=11)
    runs = []
    for _ in range(2):
        gp = mirror_gp(ctx, X[:127], y[:127], mean)
        assert device_posterior(gp, hyp, ctx=ctx)
        built = [(p.L.copy(), p.alpha.copy()) for p in gp.posteriors]
        xs = X[:40] + 0.1
        pb = gp.predict(xs, separate_samples=True)
        for n in range(127, 131):
            gp.append(X[n], y[n, 0])
        runs.append((built, pb, [(p.L, p.alpha) for p in gp.posteriors], gp.predict(xs, separate_samples=True)))
    (b0, p0, a0, q0), (b1, p1, a1, q1) = runs
    for (L0, al0), (L1, al1) in zip(b0 + a0, b1 + a1):
        assert np.array_equal(L0, L1) and np.array_equal(al0, al1)
    for u, v in zip(p0 + q0, p1 + q1):
        assert np.array_equal(u, v)
