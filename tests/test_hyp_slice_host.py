"""CPU tests of GP hyper-parameter fitting's host side: the prior (pyvbmc_amd.gp.hyper_log_prior) against SciPy's
densities, the preconditions of the device replay (tests/hyp_slice_host.py: no cap hit, every comparison decided by ten
times what the two sides can differ by), the NumPy route of ``sample_hyperparameters`` against tests/slice_host.py bit for
bit, and ``GP.fit(device=False)`` end to end."""
import numpy as np
import pytest
import scipy.stats as sst

import hyp_slice_host as hs
import slice_host
from oracle import gp_ref
from test_gp_post_gpu import mirror_gp


def some_priors(P, rng):
    pri = {"mu": rng.standard_normal(P), "sigma": 0.3 + rng.random(P), "df": np.full(P, np.inf)}
    pri["df"][::2] = [3.0, 1.0, 7.5, 30.0][: len(pri["df"][::2])]
    pri["sigma"][1] = np.nan  # no prior on parameter 1
    return pri


def scipy_prior(h, pri):
    lp = 0.0
    for p in range(h.size):
        if np.isnan(pri["sigma"][p]):
            continue
        if np.isinf(pri["df"][p]):
            lp += sst.norm.logpdf(h[p], pri["mu"][p], pri["sigma"][p])
        else:
            lp += sst.t.logpdf(h[p], pri["df"][p], pri["mu"][p], pri["sigma"][p])
    return lp


def test_prior_against_scipy():
    from pyvbmc_amd.gp import hyper_log_prior

    rng = np.random.default_rng(5)
    P = 7
    pri = some_priors(P, rng)
    H = np.vstack([rng.standard_normal((20, P)) * 3, pri["mu"][None, :], np.where(np.isnan(pri["mu"]), 0, pri["mu"]) + 40.0])
    batch = hyper_log_prior(H, pri)
    for h, b in zip(H, batch):
        ref = scipy_prior(h, pri)
        assert abs(hyper_log_prior(h, pri) - ref) <= 1e-13 * (1 + abs(ref))
        assert abs(hs.log_prior(h, pri) - ref) <= 1e-13 * (1 + abs(ref))
        assert b == hyper_log_prior(h, pri)
    assert hyper_log_prior(H[0], None) == 0.0
    with pytest.raises(ValueError):
        hyper_log_prior(H[0], {"mu": np.zeros(P), "sigma": -np.ones(P), "df": np.full(P, 3.0)})


def test_prior_gradient_against_central_difference():
    from pyvbmc_amd.gp import hyper_log_prior

    rng = np.random.default_rng(6)
    P = 7
    pri = some_priors(P, rng)
    for h in rng.standard_normal((5, P)) * 2:
        val, g = hyper_log_prior(h, pri, grad=True)
        assert val == hyper_log_prior(h, pri)
        for p in range(P):
            e = np.zeros(P)
            e[p] = 1e-5
            fd = (hyper_log_prior(h + e, pri) - hyper_log_prior(h - e, pri)) / 2e-5
            assert abs(g[p] - fd) <= 1e-8 * (1 + abs(fd)), (p, g[p], fd)
    assert g[1] == 0.0


@pytest.mark.parametrize("key", list(hs.CASES))
def test_replay_preconditions(key):
    """No cap is hit and the smallest |f - ly| is at least ten times the largest bound of a value the chains compared:
    the device and the host each stay within that bound, so the device takes the host's decisions."""
    res = hs.replay(key)
    margin, bound = min(r["margin"] for r in res), max(r["bound"] for r in res)
    print(f"case {key}: margin {margin:.3e}, bound {bound:.3e}, ratio {margin / bound:.0f}, "
          f"evaluations {[int(r['stats'][0]) for r in res]}")
    for r in res:
        assert r["stats"][2] == 0 and r["stats"][3] == 0
        assert r["samples"].shape == (hs.case(key).n, hs.case(key).P)
    assert bound > 0 and margin >= 10 * bound


def package_log_post(gp, cs):
    """f over the package's own host lml and prior, as ``sample_hyperparameters(device=False)`` forms it."""
    from pyvbmc_amd import gp as gpm

    X, y, D = np.ascontiguousarray(gp.X), np.ravel(gp.y), cs.D

    def f(h):
        with np.errstate(all="ignore"):
            sn2 = gpm._noise_var(gp, h[D + 1 : D + 2])
            lml = gpm._host_lml(X, y, cs.mean, h, sn2, np.min(sn2), 0.0, False)[0]
        return lml + gpm.hyper_log_prior(h, cs.priors)

    return f


@pytest.mark.parametrize("key", [63, 65])
def test_host_route_is_slice_host(key):
    from pyvbmc_amd.gp import sample_hyperparameters

    cs = hs.case(key)
    gp = mirror_gp(None, cs.X, cs.y, cs.mean, s2=cs.s2)
    out = sample_hyperparameters(gp, cs.x0[:2], lb=cs.lb, ub=cs.ub, widths=cs.widths, priors=cs.priors, n=cs.n, thin=cs.thin,
                                 burn_in=cs.burn_in, seed=cs.seed, device=False)
    assert out["samples"].shape == (2, cs.n, cs.P) and out["log_post"].shape == (2, cs.n) and out["stats"].shape == (2, 4)
    f = package_log_post(gp, cs)
    for c in range(2):
        ref = slice_host.chain(f, cs.x0[c], cs.widths, cs.lb, cs.ub, cs.n, cs.thin, cs.burn_in, seed=cs.seed, s=c)
        assert np.array_equal(out["samples"][c], ref["samples"])
        assert np.array_equal(out["log_post"][c], ref["f_vals"])
        assert np.array_equal(out["stats"][c], ref["stats"])
        for k in range(cs.n):
            assert out["log_post"][c, k] == f(out["samples"][c, k])
    # the host statement of the tests agrees with the package's to rounding
    assert abs(f(cs.x0[0]) - cs.log_post(cs.x0[0])) <= 1e-9
    # an invalid start, bad arguments
    bad = cs.x0[:2].copy()
    bad[1, 0] = np.nan
    kw = dict(lb=cs.lb, ub=cs.ub, widths=cs.widths, priors=cs.priors, device=False)
    with pytest.raises(ValueError, match="Invalid value."):
        sample_hyperparameters(gp, bad, **kw)
    with pytest.raises(ValueError):
        sample_hyperparameters(gp, cs.x0[:1], **{**kw, "widths": 0 * cs.widths})
    with pytest.raises(ValueError):
        sample_hyperparameters(gp, cs.x0[:1], **{**kw, "ub": np.full(cs.P, np.inf)})
    with pytest.raises(ValueError):
        sample_hyperparameters(gp, cs.x0[:1], n=0, **kw)
    with pytest.raises(ValueError):
        sample_hyperparameters(gp, cs.x0[:1, :-1], **kw)


def test_bounds_and_priors_forms():
    from pyvbmc_amd import gp as gpm

    D = 2
    gp = gpm.GP(D, gpm.SquaredExponential(), gpm.NegativeQuadratic(), gpm.GaussianNoise(constant_add=True))
    P = 3 * D + 3
    assert gp.hyper_priors["mu"].size == P and set(gp.get_bounds()) == {
        "covariance_log_lengthscale", "covariance_log_outputscale", "noise_log_scale", "mean_const", "mean_location",
        "mean_log_scale"}
    gp.set_bounds({"lb": np.full(P, -5.0), "ub": np.full(P, 5.0)})
    b = gp.get_bounds()
    b["noise_log_scale"] = (np.log(0.05), np.nan)  # NaN: the upper bound stays
    b["mean_location"] = (np.array([-1.0, -2.0]), np.array([1.0, 2.0]))
    gp.set_bounds(b)
    arr = gp.get_bounds(as_array=True)
    assert arr["lb"][D + 1] == np.log(0.05) and arr["ub"][D + 1] == 5.0
    assert list(arr["lb"][D + 3 : 2 * D + 3]) == [-1.0, -2.0] and list(arr["ub"][D + 3 : 2 * D + 3]) == [1.0, 2.0]
    pri = gp.get_priors()
    assert all(v is None for v in pri.values())
    pri["covariance_log_lengthscale"] = ("student_t", (np.log(1.5), 1.0, 3))
    pri["mean_const"] = ("gaussian", (0.0, 2.0))
    gp.set_priors(pri)
    hp = gp.hyper_priors
    assert list(hp["df"][:D]) == [3.0, 3.0] and np.isinf(hp["df"][D + 2]) and np.isnan(hp["sigma"][D])
    back = gp.get_priors()
    assert back["mean_const"][0] == "gaussian" and back["covariance_log_lengthscale"][0] == "student_t"
    assert back["noise_log_scale"] is None
    gp.set_priors({"mu": np.full(P, np.nan), "sigma": np.full(P, np.nan), "df": np.full(P, np.nan)})  # all NaN: nothing changes
    assert list(gp.hyper_priors["df"][:D]) == [3.0, 3.0]
    with pytest.raises(ValueError):
        gpm.GP(D, gpm.SquaredExponential(), gpm.ConstantMean(), gpm.GaussianNoise(True)).set_bounds({"mean_location": (0, 1)})


def test_fit_on_the_host():
    import gp_post_host as gph
    from pyvbmc_amd.gp import hyper_log_prior, log_marginal_likelihood

    N, D, mean = 30, 2, gp_ref.MEAN_CONST
    X, y, hyp = gph.make_case(N, D, 2, mean, seed=100 + N)
    gp = mirror_gp(None, X, y, mean)
    P = hyp.shape[1]
    with pytest.raises(ValueError):
        gp.fit(X, y, hyp0=hyp, device=False)  # no finite bounds yet
    lb, ub = hyp.min(0) - 2.0, hyp.max(0) + 2.0
    lb[D + 1] = np.log(0.05)
    gp.set_bounds({"lb": lb, "ub": ub})
    gp.set_priors({"covariance_log_lengthscale": ("student_t", (np.log(1.5), 1.0, 3)),
                   "noise_log_scale": ("student_t", (np.log(0.3), 0.5, 3))})
    assert gp.hyper_priors["mu"].size == P
    opts = {"init_N": 12, "opts_N": 2, "n_samples": 3, "thin": 2, "burn": 1, "widths": None, "tol_opt": 1e-5}
    out, opt, smp = gp.fit(X, y, None, hyp0=hyp, options=opts, device=False, seed=11)
    assert out.shape == (3, P) and smp["samples"].shape == (3, P) and smp["log_post"].shape == (3,)
    assert smp["log_priors"].shape == (3,) and smp["stats"].shape == (3, 4)
    assert opt["candidates"].shape == (2 + 12, P) and opt["candidate_log_post"].shape == (14,)
    assert np.all(out >= lb) and np.all(out <= ub) and np.all(opt["hyp"] >= lb) and np.all(opt["hyp"] <= ub)
    assert opt["log_post"] >= np.max(opt["candidate_log_post"])
    lml = log_marginal_likelihood(gp, out, device=False)
    assert np.array_equal(smp["log_priors"], hyper_log_prior(out, gp.hyper_priors))
    assert np.allclose(smp["log_post"] - smp["log_priors"], lml, rtol=0, atol=1e-12 * np.max(np.abs(lml)))
    assert len(gp.posteriors) == 3 and np.array_equal(gp.get_hyperparameters(), out)
    # the same seed gives the same fit; without sampling the optimum is the result
    again = mirror_gp(None, X, y, mean)
    again.set_bounds({"lb": lb, "ub": ub})
    again.set_priors(gp.get_priors())
    out2, _, _ = again.fit(X, y, None, hyp0=hyp, options=opts, device=False, seed=11)
    assert np.array_equal(out, out2)
    only, opt1, none = again.fit(hyp0=hyp, options={**opts, "n_samples": 0}, device=False, seed=11)
    assert none is None and only.shape == (1, P) and np.array_equal(only[0], opt1["hyp"])
