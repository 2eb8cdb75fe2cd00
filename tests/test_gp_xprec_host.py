"""CPU tests of tests/gp_xprec.py, the long-double restatement the ill-conditioned GPU tests compare with
(tests/test_gp_illcond_gpu.py): the restatement is gp_ref's mathematics, and the cases sit where that test is honest --
in the condition band, with a truth at least 64 times more accurate than the float64 slack it grants, and (from
cond2(A) = 5e7 on) beyond the project's 1e-10 predict bound."""
import numpy as np
import pytest

import gp_post_host as gph
import gp_xprec as gx
from oracle import gp_ref


def test_longdouble_is_extended():
    gx.require_extended()


def test_restatement_agrees_with_gp_ref_on_a_well_conditioned_case():
    """make_case(65, 3, 2, NEGQUAD, well=True): posterior, predict and gp_log_joint with its variance to 1e-13
    relative (the oracle's own float64 rounding at cond2(A) ~ 1e2 is ~1e-14)."""
    mean = gp_ref.MEAN_NEGQUAD
    X, y, hyp = gph.make_case(65, 3, 2, mean, seed=165)
    d = gx.data("n130_d3_sn1e-3")
    mix, xs = d["mix"], d["xs"]  # (D = 3: the case's mixture and query points serve)
    t = gx._evaluate_ld(mean, X, y, hyp, xs, mix, True)
    o = gx._route_a(mean, X, y, hyp, xs, mix)
    assert set(o) == set(t)
    for k in sorted(o):
        rel = float(np.max(gx.err(o[k], t[k], k)) / np.max(np.abs(t[k])))
        print(f"{k}: {rel:.2e}")
        assert rel <= 1e-13, (k, rel)
    # the device's route in float64 is the same mathematics too
    b = gx._route_b(mean, X, y, hyp, xs, mix)
    for k in sorted(b):
        assert float(np.max(gx.err(b[k], t[k], k)) / np.max(np.abs(t[k]))) <= 1e-13, k


def test_the_case_list_is_what_the_gpu_test_needs():
    assert len(gx.CASES) == 6 and sum(c.D == 10 for c in gx.CASES) == 1 and sum(not c.L_chol for c in gx.CASES) == 1
    assert any(c.mean == gp_ref.MEAN_CONST for c in gx.CASES)
    for c in gx.CASES:
        d = gx.data(c.name)
        assert c.N <= 257 and d["mix"].K == 3 and d["xs"].shape == (gx.M_QUERY, c.D) and d["hyp"].shape[0] == 2
        assert gx.M_SMALL <= 32 < gx.M_QUERY <= 64


@pytest.mark.parametrize("name", gx.NAMES)
def test_case_is_in_the_band_and_the_truth_is_accurate(name):
    c, d = gx.BY_NAME[name], gx.data(name)
    D = c.D
    cond_ill, cond_well = gx.cond2(name)
    print(f"{name}: cond2(A) {cond_ill:.2e} (sample 0), {cond_well:.2e} (sample 1)")
    assert 1e6 <= cond_ill <= 1e9 and cond_well <= 1e3
    # the branch each sample takes, by the posterior's own rule
    posts = [gp_ref.make_posterior(h, d["X"], d["y"], c.mean) for h in d["hyp"]]
    assert posts[0].L_chol is c.L_chol and posts[1].L_chol is True
    t, e = gx.truth(name), gx.e64(name)
    for M in (None, gx.M_SMALL):
        tm, em = (t, e) if M is None else (gx.truth_predict(name, M), gx.e64(name, M))
        for k in tm["corr"]:
            corr, slack = np.atleast_1d(tm["corr"][k]), np.atleast_1d(em[k])
            with np.errstate(divide="ignore"):
                ratio = float(np.min(np.where(corr > 0, slack / corr, np.inf)))
            print(f"  {k} (M={M}): e64 oracle {em['parts']['oracle'][k]}, device route {em['parts']['device_route'][k]}, "
                  f"refinement {tm['corr'][k]}, e64 / refinement >= {ratio:.0f}")
            assert np.all(corr <= slack / 64), (k, corr, slack)
    if cond_ill >= 5e7:
        old = 1e-10 * max(1.0, float(np.max(np.abs(t["mu"]))))
        print(f"  e64 of mu {e['mu'][0]:.2e} against the old bound {old:.2e}")
        assert e["mu"][0] > old
        assert e["mu"][1] < old  # (the well-conditioned sample stays inside it)


@pytest.mark.parametrize("name", gx.NAMES)
def test_tolerance_catches_a_per_term_error_in_kstar(name):
    """What the GPU test exists for: a relative error of 1e-12 per entry of K* (random signs -- a fast exp, a
    cancelling distance; a float32 intermediate is 6e-8) under the oracle's own alpha moves the ill-conditioned sample's
    predictive mean past max(B_mu, 8 e64_mu), while it stays invisible (< 1e-10) on the well-conditioned sample."""
    c, d = gx.BY_NAME[name], gx.data(name)
    D = c.D
    t, e = gx.truth(name), gx.e64(name)
    tol = np.maximum(gx.project_bound("mu", t, gx.sf2_of(d["hyp"], D)), 8.0 * e["mu"])
    rng = np.random.default_rng(1)
    got = []
    for s, h in enumerate(d["hyp"]):
        p = gp_ref.make_posterior(h, d["X"], d["y"], c.mean)
        Ks = gp_ref.se_ard(h[: D + 1], d["X"], d["xs"])
        Ks = Ks * (1.0 + 1e-12 * rng.choice([-1.0, 1.0], size=Ks.shape))
        mu = gp_ref.mean_fn(c.mean, h[D + 2 :], d["xs"]) + Ks.T @ p.alpha.ravel()
        got.append(float(np.max(np.abs(mu.astype(gx.LD) - t["mu"][:, s]))))
    print(f"{name}: error of mu under the perturbed K* {got[0]:.2e} / {got[1]:.2e}, tolerance {tol[0]:.2e} / {tol[1]:.2e}")
    assert got[0] > tol[0]
    assert got[1] < 1e-10


def test_nmant_failure_is_a_failure(monkeypatch):
    class Short:
        nmant = 52

    monkeypatch.setattr(gx.np, "finfo", lambda _: Short)
    with pytest.raises(AssertionError, match="mantissa"):
        gx.require_extended()
