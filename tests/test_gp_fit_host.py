"""CPU tests of ``GP.fit(optimizer="fused")``'s host route -- the statement of the stages vbmc_gp_fit runs on the device
(pyvbmc_amd/gp.py ``_fit_fused``, ``fit_design``, ``fit_rank``, ``fit_select``) -- of ``get_bounds_info``, and of the two
existing routes, whose results the new one must not change."""
import numpy as np
import pytest

import gp_fit_cases as gfc


@pytest.fixture(scope="module")
def fused():
    """The fused host fit of case 63, computed once and left unchanged."""
    return gfc.fit_package(None, gfc.case(63), False)


# --------------------------------------------------------------------------------------------------------- design
def test_design_is_the_philox_statement(fused):
    from pyvbmc_amd.gp import fit_design

    cs = gfc.case(63)
    dlb, dub = gfc.design_box(cs)
    direct = gfc.design_rows(gfc.INIT_N, dlb, dub, gfc.SEED)
    assert np.array_equal(fit_design(gfc.INIT_N, dlb, dub, gfc.SEED), direct)
    cand = fused[2]["candidates"]
    assert cand.shape == (gfc.H + gfc.INIT_N, cs.P) and np.array_equal(cand[gfc.H :], direct)
    assert np.array_equal(cand[: gfc.H], np.clip(cs.x0[: gfc.H], cs.lb, cs.ub))
    assert np.all(direct >= dlb) and np.all(direct <= dub) and len({tuple(r) for r in direct}) == gfc.INIT_N
    # a row depends on its own index and the seed alone; a degenerate box gives its point
    assert np.array_equal(fit_design(5, dlb, dub, gfc.SEED), direct[:5])
    assert not np.array_equal(fit_design(5, dlb, dub, gfc.SEED + 1), direct[:5])
    assert np.array_equal(fit_design(2, dlb, dlb, 3), np.vstack([dlb, dlb])) and fit_design(0, dlb, dub, 3).shape == (0, cs.P)


# ------------------------------------------------------------------------------------------- ranking and selection
def test_rank_on_hand_made_scores():
    from pyvbmc_amd.gp import fit_rank

    score, order = fit_rank([1.0, -np.inf, 3.0, np.nan, 3.0, 1.0, np.inf])
    assert list(score) == [1.0, -np.inf, 3.0, -np.inf, 3.0, 1.0, -np.inf]  # NaN and +inf count as no finite score
    assert list(order) == [2, 4, 0, 5, 1, 3, 6]  # descending, ties (the -inf ones too) to the lower index
    assert list(fit_rank([-np.inf, -np.inf])[1]) == [0, 1]


def test_select_on_hand_made_results():
    from pyvbmc_amd.gp import fit_select

    assert fit_select(-5.0, [-4.0, -3.0, -3.0], [0, 0, 0]) == (1, -3.0)  # the first of the greatest
    assert fit_select(-5.0, [-4.0, -3.0], [0, 1]) == (0, -4.0)  # an invalid run is never taken
    assert fit_select(-5.0, [-5.0, np.nan, -np.inf], [0, 0, 0]) == (-1, -5.0)  # strictly greater only; not finite: skipped
    assert fit_select(-5.0, [0.0, 0.0], [1, 1]) == (-1, -5.0) and fit_select(-5.0, [], []) == (-1, -5.0)
    assert fit_select(-5.0, [np.inf, -1.0], [0, 0]) == (1, -1.0)


def test_fused_results_follow_the_rules(fused):
    from pyvbmc_amd.gp import fit_rank, fit_select, hyper_log_prior, log_marginal_likelihood

    cs = gfc.case(63)
    gp, hyp, opt, smp = fused
    cand = opt["candidates"]
    score = log_marginal_likelihood(gp, cand, device=False) + hyper_log_prior(cand, cs.priors)
    assert np.array_equal(opt["candidate_log_post"], fit_rank(score)[0])
    assert np.array_equal(opt["starts"], fit_rank(score)[1][: gfc.OPTS_N])
    runs = opt["runs"]
    k, f = fit_select(float(np.max(score)), runs["log_post"], runs["invalid"])
    assert k >= 0 and opt["log_post"] == f and np.array_equal(opt["hyp"], runs["hyp"][k])
    assert opt["n_iterations"] == int(np.sum(runs["stats"][:, 0])) > 0
    assert hyp.shape == (gfc.N_SAMPLES, cs.P) and np.array_equal(smp["samples"], hyp) and np.array_equal(gp.get_hyperparameters(), hyp)
    assert np.all(hyp >= cs.lb) and np.all(hyp <= cs.ub) and len({tuple(r) for r in hyp}) == gfc.N_SAMPLES
    assert np.allclose(smp["log_priors"], hyper_log_prior(hyp, cs.priors), rtol=1e-13, atol=0)
    again = gfc.fit_package(None, cs, False)  # the same seed: the same fit
    assert np.array_equal(again[1], hyp) and again[2]["log_post"] == opt["log_post"]


def test_not_positive_definite_candidate_ranks_last():
    cs = gfc.case(63)
    ub = cs.ub.copy()
    ub[cs.D] = 400.0
    bad = cs.x0[1].copy()
    bad[cs.D] = 400.0  # exp(2 log sf) overflows: the covariance is not finite
    gp = gfc.make_gp(None, cs)
    gp.set_bounds({"lb": cs.lb, "ub": ub})
    gp.set_priors(cs.priors)
    hyp0 = np.vstack([cs.x0[0], bad, cs.x0[0]])
    _, opt, _ = gp.fit(hyp0=hyp0, options=dict(init_N=0, opts_N=3, n_samples=0, tol_opt=1e-2), device=False, seed=1, optimizer="fused")
    assert np.isneginf(opt["candidate_log_post"][1]) and list(opt["starts"]) == [0, 2, 1]
    assert list(opt["runs"]["invalid"]) == [0, 0, 1] and np.array_equal(opt["runs"]["hyp"][0], opt["runs"]["hyp"][1])
    with pytest.raises(ValueError, match="no candidate has a finite log posterior"):
        gp.fit(hyp0=bad[None, :], options=dict(init_N=0, opts_N=1), device=False, seed=1, optimizer="fused")
    with pytest.raises(ValueError, match="design box"):
        gp.fit(hyp0=hyp0, options=dict(init_N=2, design_lb=cs.lb - 1.0), device=False, seed=1, optimizer="fused")


# ------------------------------------------------------------------------------------------------- stage switches
def test_stage_switches_on_the_host(fused):
    from pyvbmc_amd.gp import fit_rank

    cs = gfc.case(63)
    base = fused[2]
    gp, hyp, opt, smp = gfc.fit_package(None, cs, False, opts_N=0, n_samples=0)
    i0 = fit_rank(base["candidate_log_post"])[1][0]
    assert smp is None and hyp.shape == (1, cs.P) and np.array_equal(hyp[0], base["candidates"][i0]) and opt["starts"].size == 0
    assert opt["log_post"] == base["candidate_log_post"][i0] and opt["n_iterations"] == 0 and len(gp.posteriors) == 1
    gp, hyp, opt, smp = gfc.fit_package(None, cs, False, n_samples=0)
    assert smp is None and np.array_equal(hyp[0], base["hyp"]) and opt["log_post"] == base["log_post"] and len(gp.posteriors) == 1
    gp, hyp, opt, smp = gfc.fit_package(None, cs, False, init_N=0, opts_N=1, n_samples=2, burn=1, thin=1)
    assert np.array_equal(opt["candidates"], np.clip(cs.x0[: gfc.H], cs.lb, cs.ub)) and hyp.shape == (2, cs.P)
    assert np.array_equal(opt["candidate_log_post"], base["candidate_log_post"][: gfc.H]) and len(gp.posteriors) == 2


# --------------------------------------------------------------------------------- the two existing routes stand
def test_scipy_and_lockstep_routes_are_what_they_were():
    """``optimizer="scipy"`` and ``"lockstep"`` against their stages recomputed here from the unchanged pieces: the design
    from ``np.random.default_rng(seed)`` in the hard box, one scored batch, the optimiser from the best finite candidates,
    the chains under the sub-seed drawn from the same generator."""
    import scipy.optimize as sopt

    from pyvbmc_amd.gp import hyper_log_prior, log_marginal_likelihood, optimize_hyperparameters, sample_hyperparameters

    cs = gfc.case(63)
    seed, init_N, S = 9, 6, 2
    opts = dict(init_N=init_N, opts_N=2, n_samples=S, thin=1, burn=1, widths=np.full(cs.P, gfc.WIDTH), tol_opt=1e-3)
    rng = np.random.default_rng(seed)
    cand = np.vstack([np.clip(cs.x0[: gfc.H], cs.lb, cs.ub), cs.lb + (cs.ub - cs.lb) * rng.random((init_N, cs.P))])
    sub = int(rng.integers(0, 2**63))
    ref = gfc.make_gp(None, cs)
    score = log_marginal_likelihood(ref, cand, device=False) + hyper_log_prior(cand, cs.priors)
    order = np.argsort(-score, kind="stable")
    assert np.all(np.isfinite(score))
    expect = {}
    res = optimize_hyperparameters(ref, cand[order[:2]], lb=cs.lb, ub=cs.ub, priors=cs.priors, tol_g=1e-3, device=False)
    k = int(np.argmax(res["log_post"]))
    expect["lockstep"] = (res["hyp"][k], float(res["log_post"][k])) if res["log_post"][k] > score[order[0]] else (cand[order[0]], float(score[order[0]]))

    def neg(h):
        lml, dl = log_marginal_likelihood(ref, h[None, :], grad=True, device=False)
        lp, dp = hyper_log_prior(h, cs.priors, grad=True)
        return (-(lml[0] + lp), -(dl[0] + dp)) if np.isfinite(lml[0]) and np.all(np.isfinite(dl[0])) else (1e100, np.zeros(cs.P))

    best = (cand[order[0]], float(score[order[0]]))
    for i in order[:2]:
        r = sopt.minimize(neg, cand[i], jac=True, method="L-BFGS-B", bounds=list(zip(cs.lb, cs.ub)), tol=1e-3)
        h = np.clip(r.x, cs.lb, cs.ub)
        f = float(log_marginal_likelihood(ref, h[None, :], device=False)[0] + hyper_log_prior(h, cs.priors))
        if np.isfinite(f) and f > best[1]:
            best = (h, f)
    expect["scipy"] = best
    for name, (h, f) in expect.items():
        gp = gfc.make_gp(None, cs)
        gp.set_bounds({"lb": cs.lb, "ub": cs.ub})
        gp.set_priors(cs.priors)
        hyp, opt, smp = gp.fit(hyp0=cs.x0[: gfc.H], options=opts, device=False, seed=seed, optimizer=name)
        assert np.array_equal(opt["candidates"], cand) and np.array_equal(opt["candidate_log_post"], score), name
        assert np.array_equal(opt["hyp"], h) and opt["log_post"] == f and "starts" not in opt, name
        chains = sample_hyperparameters(ref, np.tile(h, (S, 1)), lb=cs.lb, ub=cs.ub, widths=opts["widths"], priors=cs.priors, n=1,
                                        thin=1, burn_in=1, seed=sub, device=False)
        assert np.array_equal(hyp, chains["samples"][:, 0, :]) and np.array_equal(smp["log_post"], chains["log_post"][:, 0]), name
    with pytest.raises(ValueError, match="not 'scipy', 'lockstep' or 'fused'"):
        gp.fit(hyp0=cs.x0[: gfc.H], options=opts, device=False, seed=seed, optimizer="other")


# ------------------------------------------------------------------------------------------------ get_bounds_info
def test_get_bounds_info_rule():
    from pyvbmc_amd import gp as gpm

    rng = np.random.default_rng(2)
    X = rng.uniform(-1.0, 3.0, (40, 3))
    X[:, 2] = 0.7  # a zero range counts as 1
    y = rng.standard_normal((40, 1)) * 2.0
    w, h = np.array([np.ptp(X[:, 0]), np.ptp(X[:, 1]), 1.0]), float(np.ptp(y))
    se = gpm.SquaredExponential().get_bounds_info(X, y)
    assert np.allclose(se["LB"], np.log(1e-6 * np.append(w, h))) and np.allclose(se["UB"], np.log(10 * np.append(w, h)))
    assert np.allclose(se["PLB"], np.log(1e-3 * np.append(w, h))) and np.allclose(se["PUB"], np.log(np.append(w, h)))
    assert np.allclose(se["x0"][:2], np.log(np.std(X[:, :2], axis=0))) and se["x0"][2] == 0.0 and np.isclose(se["x0"][3], np.log(np.std(y)))
    nz = gpm.GaussianNoise(constant_add=True).get_bounds_info(X, y)
    assert np.isclose(nz["LB"][0], np.log(1e-3)) and np.isclose(nz["UB"][0], np.log(max(h, 1.0))) and nz["x0"][0] == nz["PLB"][0] == nz["LB"][0]
    assert np.isclose(nz["PUB"][0], np.log(max(np.std(y), 1e-2)))
    cm = gpm.ConstantMean().get_bounds_info(X, y)
    assert np.isclose(cm["LB"][0], y.min() - h / 2) and np.isclose(cm["UB"][0], y.max() + h / 2) and cm["x0"][0] == np.median(y)
    assert np.isclose(cm["PLB"][0], np.quantile(y, 0.1)) and np.isclose(cm["PUB"][0], np.quantile(y, 0.9))
    nq = gpm.NegativeQuadratic().get_bounds_info(X, y)
    assert all(nq[k].shape == (7,) for k in nq) and np.array_equal(nq["LB"][:1], cm["LB"])
    assert np.allclose(nq["LB"][1:4], X.min(0) - w / 2) and np.allclose(nq["UB"][1:4], X.max(0) + w / 2)
    assert np.array_equal(nq["PLB"][1:4], X.min(0)) and np.array_equal(nq["PUB"][1:4], X.max(0)) and np.array_equal(nq["x0"][1:4], np.median(X, 0))
    assert np.allclose(nq["LB"][4:], np.log(1e-3 * w)) and np.allclose(nq["UB"][4:], np.log(10 * w))
    assert np.allclose(nq["PLB"][4:], np.log(1e-2 * w)) and np.allclose(nq["PUB"][4:], np.log(w))
    assert all(v.size == 0 for v in gpm.ZeroMean().get_bounds_info(X, y).values())
    for info in (se, nz, cm, nq):
        assert np.all(info["LB"] <= info["PLB"]) and np.all(info["PLB"] <= info["PUB"]) and np.all(info["PUB"] <= info["UB"])
        assert np.all(np.isfinite(np.concatenate(list(info.values()))))
