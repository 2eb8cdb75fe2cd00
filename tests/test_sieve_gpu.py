"""The sieve on the device (pyvbmc_amd/sieve.py, csrc/sieve.hip, csrc/api_sieve.hip) against the NumPy statement
tests/sieve_host.py, against the reference's recorded scores and order (tests/golden/sieve.npz), and -- for the ranking --
against ``np.argsort(kind="stable")`` of the device's own values.

Bounds.  Thetas: ``C_THETA eps A max(1, |theta|)`` with ``A = max(1, |inputs|)``, derived in profiles/sieve.md from the
caps of profiles/fastmath_ulp.md along the longest chain of primitives, one rounding per arithmetic operation and the D-
and K-term sums; the measured maximum is printed (``pytest -s``) and recorded there.  Scores: the project's ELBO parity
bound, 1e-10 relative (README).  Order, types, NumPy's state: exactly.
"""
import numpy as np
import pytest
import sieve_host as sh
from helpers import PlainGP
from width_cases import SWEEP_D

from oracle import gp_ref

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
C_THETA = 4000.0  # profiles/sieve.md, section 1
ATTRS = ("mu", "sigma", "lambd", "w", "eta")


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


@pytest.fixture(scope="module")
def z():
    return np.load(sh.GOLDEN, allow_pickle=False)


def names():
    return sh.case_names(np.load(sh.GOLDEN, allow_pickle=False))


def package_vp(c, ctx, K=None, attrs=None):
    from pyvbmc_amd import VariationalPosterior

    D = int(c["shape"][0])
    K = int(c["shape"][1]) if K is None else K
    vp = VariationalPosterior(D, K)
    for a in ATTRS:
        setattr(vp, a, np.array(c["base_" + a] if attrs is None else attrs[a]))
    vp.optimize_mu, vp.optimize_sigma, vp.optimize_lambd, vp.optimize_weights = (bool(f) for f in c["flags"])
    vp.ctx = ctx
    return vp


def case_gp(c, ctx):
    gp = PlainGP(gp_ref.make_gp(c["X"], c["y"], c["hyp"], gp_ref.MEAN_NEGQUAD))
    gp._ctx = ctx
    return gp


def batch_inputs(c, ctx):
    """``_neg_elcbo_batch``'s arguments for a case's recorded thetas: a posterior of K_new components that carries the
    blocks that are not optimised (they are the same for every candidate: candidate 0's), the GP, the soft bounds."""
    Kn = int(c["shape"][2])
    vp = package_vp(c, ctx, Kn, {a: c["fin_" + a][0] for a in ATTRS})
    return np.array(c["thetas"]), case_gp(c, ctx), vp, vp.get_bounds(c["X"], sh.options_of(c), Kn)


def amplitude(*arrays):
    return max(1.0, *(float(np.max(np.abs(a))) for a in arrays))


def theta_error(got, want, A, what):
    """max |got - want| / (A max(1, |want|)) in eps, printed and returned."""
    err = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) / (A * EPS)
    print(f"{what}: max theta error {err:.2f} eps A max(1, |theta|) (bound {C_THETA:.0f})")
    return err


@pytest.mark.parametrize("name", names())
def test_fixture_cases_numpy_stream(z, ctx, name):
    from pyvbmc_amd import sieve as sv

    c = sh.load_case(z, name)
    D, K, Kn, N, init_N, best_N = (int(v) for v in c["shape"])
    X_star, y_star = sh.get_hpd(c["X"], c["y"], sh.options_of(c)["hpd_frac"])[:2]
    np.random.seed(int(c["seed"]))
    _, want, _, types = sh.candidates_host(sh.base_of(c), c["flags"], sh.split(init_N, best_N), Kn, X_star, y_star,
                                           sh.NumpySource())
    vp, gp = package_vp(c, ctx), case_gp(c, ctx)
    np.random.seed(int(c["seed"]))
    out = sv.sieve(sh.options_of(c), {"entropy_switch": False}, vp, gp, init_N, best_N, Kn, rng="numpy", ctx=ctx,
                   return_candidates=True)
    st = np.random.get_state(legacy=True)
    vps, vtypes, beta, cvar, ns_ent_K, ns_fast, cand, order = out
    assert np.array_equal(st[1], c["mt_key"]) and st[2] == int(c["mt_pos"]) and st[3] == int(c["mt_has_gauss"])
    assert (beta, cvar, ns_ent_K, ns_fast) == (0, False, int(c["ns_ent_K"]), 0)
    assert theta_error(cand.thetas, want, amplitude(c["X"], c["base_mu"]), name) <= C_THETA
    rel = np.abs(cand.F - c["F"]) / np.abs(c["F"])
    print(f"{name}: max relative score error {rel.max():.2e} (bound 1e-10)")
    assert np.all(rel <= 1e-10)
    assert np.array_equal(order, c["order"])
    assert np.array_equal(cand.types, types) and np.array_equal(vtypes, types[order])
    assert vps.dtype == object and len(vps) == len(order) and vp.K == K and vp.bounds is not None


@pytest.mark.parametrize("N_star", [4, 40])
@pytest.mark.parametrize("D", SWEEP_D)
def test_philox_draws_at_every_width(ctx, D, N_star):
    from pyvbmc_amd import VariationalPosterior
    from pyvbmc_amd import sieve as sv

    K, Kn, counts, seed = 3, 5, (3, 3, 1), 0xC0FFEE + D
    r = np.random.default_rng(100 * D + N_star)
    lam = 0.5 + r.random((D, 1))
    base = {"mu": 0.8 * r.standard_normal((D, K)), "sigma": 0.3 + 0.5 * r.random((1, K)),
            "lambd": lam / np.sqrt(np.sum(lam**2) / D), "w": np.array([[0.2, 0.5, 0.3]]), "eta": np.ones((1, K)) / K}
    X_star, y_star = r.standard_normal((N_star, D)), r.standard_normal((N_star, 1))
    vp = VariationalPosterior(D, K)
    for a in ATTRS:
        setattr(vp, a, base[a].copy())
    vp.ctx = ctx
    raw, want, _, _ = sh.candidates_host(base, (1, 1, 1, 1), counts, Kn, X_star, y_star, sh.PhiloxSource(seed, D, K, Kn))
    cand = sv._generate(vp, counts, Kn, X_star, y_star, "philox", seed, True, ctx)
    assert theta_error(cand.thetas, want, amplitude(X_star, base["mu"]), f"D={D} N_star={N_star}") <= C_THETA
    # candidate 0 of types 1 and 2 carries no jitter: its means are the start's, bit for bit (type 1: the K old components)
    assert np.array_equal(cand.thetas[0, : D * K], base["mu"].ravel(order="F"))
    assert np.array_equal(cand.thetas[3, : D * Kn], raw[3]["mu"].ravel(order="F"))
    nl = np.sqrt(np.sum(base["lambd"] ** 2) / D)
    ls = np.log(base["sigma"].ravel() * nl)
    assert np.all(np.abs(cand.thetas[0, D * Kn : D * Kn + K] - ls) <= C_THETA * EPS * np.maximum(1.0, np.abs(ls)))


def test_philox_largest_shape(ctx):
    from pyvbmc_amd import VariationalPosterior
    from pyvbmc_amd import sieve as sv

    D, K, counts, seed, N_star = 32, 128, (1, 1, 1), 99, 40
    r = np.random.default_rng(3)
    base = {"mu": 0.8 * r.standard_normal((D, K)), "sigma": 0.3 + 0.5 * r.random((1, K)), "lambd": np.ones((D, 1)),
            "w": np.ones((1, K)) / K, "eta": np.ones((1, K)) / K}
    X_star, y_star = r.standard_normal((N_star, D)), r.standard_normal((N_star, 1))
    vp = VariationalPosterior(D, K)
    for a in ATTRS:
        setattr(vp, a, base[a].copy())
    vp.ctx = ctx
    _, want, _, _ = sh.candidates_host(base, (1, 1, 1, 1), counts, K, X_star, y_star, sh.PhiloxSource(seed, D, K, K))
    cand = sv._generate(vp, counts, K, X_star, y_star, "philox", seed, True, ctx)
    assert theta_error(cand.thetas, want, amplitude(X_star, base["mu"]), "D=32 K=128") <= C_THETA


def test_rank_is_stable_with_nan_last(z, ctx):
    from pyvbmc_amd import sieve as sv

    c = sh.load_case(z, "d2k2n4_all_7")
    thetas, gp, vp, bnd = batch_inputs(c, ctx)
    r = np.random.default_rng(8)
    rows = thetas[np.arange(70) % 7] + 0.01 * r.standard_normal((70, thetas.shape[1]))
    rows[20], rows[41] = rows[5], rows[5]  # exact duplicates
    nan_rows = [7, 33, 69]
    rows[7, 0] = rows[33, 9] = rows[69, -1] = np.nan
    cand = sv.Candidates(vp, sv._Shape(vp, 4, 16), rows.copy(), np.ones(70), {})
    order, ranked = sv.score(cand, gp, bnd, ctx=ctx, put=True)  # a NaN row is scored NaN: no error
    F = cand.F
    assert np.all(np.isnan(F[nan_rows])) and np.sum(np.isnan(F)) == 3
    assert F[20] == F[5] == F[41]
    assert np.array_equal(order, np.argsort(F, kind="stable"))
    assert list(order[-3:]) == nan_rows and np.all(np.diff(F[order][:-3]) >= 0)
    pos = {int(b): i for i, b in enumerate(order)}
    assert pos[5] < pos[20] < pos[41]
    finite = ~np.isnan(rows).any(axis=1)
    assert np.array_equal(ranked[: 67, :-4], rows[order[:67], :-4]) and finite.sum() == 67  # (the eta tail comes back max-shifted)


@pytest.mark.parametrize("name", names())
def test_batch_evaluator_unchanged_by_the_factoring(z, ctx, name):
    """``vbmc_neg_elcbo_batch`` on the fixture's thetas: bit-identical to the values recorded from the build before its
    scoring part was factored out for ``vbmc_sieve_eval`` (``*_batch_F/G/H`` in the fixture)."""
    from pyvbmc_amd.variational_optimization import _neg_elcbo_batch

    c = sh.load_case(z, name)
    thetas, gp, vp, bnd = batch_inputs(c, ctx)
    F, G, H = _neg_elcbo_batch(thetas, gp, vp, bnd, ctx=ctx, return_parts=True)
    for got, k in ((F, "batch_F"), (G, "batch_G"), (H, "batch_H")):
        assert np.array_equal(got, c[k]), k
    assert np.all(np.abs(F - c["F"]) <= 1e-10 * np.abs(c["F"]))


def test_to_vps_of_a_device_sieve(z, ctx):
    from pyvbmc_amd import sieve as sv

    c = sh.load_case(z, "d2k2n4_all_7")
    vp, gp = package_vp(c, ctx), case_gp(c, ctx)
    np.random.seed(int(c["seed"]))
    out = sv.sieve(sh.options_of(c), {"entropy_switch": False}, vp, gp, 7, 3, 4, rng="numpy", ctx=ctx, return_candidates=True)
    vps, vtypes, cand, order = out[0], out[1], out[6], out[7]
    for i, v in enumerate(vps):
        assert v.K == 4 and v.bounds is None and v.stats is None and v.parameter_transformer is vp.parameter_transformer
        th = v.get_parameters()
        th[-4:] -= np.amax(th[-4:])
        row = cand.thetas[order[i]]
        assert np.all(np.abs(th - row) <= (4 + 2) * EPS * np.maximum(1.0, np.abs(row)))  # (tests/test_sieve_host.py)
    idx = np.where(vtypes == 3)[0][0]  # optimize_vp's idioms (:189-199)
    assert vps[idx].mu.shape == (2, 4)
    assert len(np.delete(vps, idx)) == 6 and len(np.delete(vtypes, idx)) == 6


@pytest.mark.parametrize("rng", ["numpy", "philox"])
def test_host_generated_candidates_are_scored_on_the_device(z, ctx, rng):
    """``device=False``: the candidates come from the package's NumPy generation and go up with ``vbmc_sieve_put``; with
    NumPy's stream the scores and the order are the fixture's, with Philox draws they are the device-generated run's."""
    from pyvbmc_amd import sieve as sv

    c = sh.load_case(z, "d2k2n4_all_7")
    gp, opts, state = case_gp(c, ctx), sh.options_of(c), {"entropy_switch": False}
    vp = package_vp(c, ctx)
    np.random.seed(int(c["seed"]))
    out = sv.sieve(opts, state, vp, gp, 7, 3, 4, rng=rng, seed=77, device=False, ctx=ctx, return_candidates=True)
    cand, order = out[6], out[7]
    if rng == "numpy":
        want_F, want_order = c["F"], c["order"]
    else:
        ref = sv.sieve(opts, state, package_vp(c, ctx), gp, 7, 3, 4, rng=rng, seed=77, device=True, ctx=ctx, return_candidates=True)
        want_F, want_order = ref[6].F, ref[7]
    assert np.all(np.abs(cand.F - want_F) <= 1e-10 * np.abs(want_F))
    assert np.array_equal(order, want_order)
