"""GPU tests of the GP hyper-parameter fit as one device call: ``vbmc_gp_fit`` (csrc/gp_fit.hip, csrc/api_gp_fit.hip) and
``GP.fit(optimizer="fused")`` over it.

The stages are the existing entries' kernels on the same inputs, so stage by stage the results must be the same BITS as
``vbmc_gp_hyp_optimize``, ``vbmc_gp_hyp_sample`` and ``vbmc_gp_posterior`` give (``np.array_equal``); what is new -- the
design, the ranking, the selection, the hand-over to the build -- is checked against its NumPy statement.  Then what the
entry promises: independence of the chunking and of the rounds per read, the stage switches, the installed state, the
refusals, and the package's two routes against each other.  The cases are tests/gp_fit_cases.py's."""
import numpy as np
import pytest

import gp_fit_cases as gfc
from oracle import gp_ref
from test_gp_opt_gpu import raw as raw_opt
from test_gp_opt_host import SCIPY_MARGIN
from test_gp_post_gpu import CountingLib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


@pytest.fixture(scope="module")
def base(ctx):
    """The fit of both cases with 16 candidates a chunk (40 candidates: 16 + 16 + 8), computed once and left unchanged."""
    ctx.set_option("gp_lml_chunk", gfc.CHUNK)
    try:
        out = {key: gfc.raw_fit(ctx, gfc.case(key)) for key in gfc.KEYS}
    finally:
        ctx.set_option("gp_lml_chunk", 0)
    for o in out.values():
        assert o.rc == 0 and o.status[0] == 0
    return out


def resident(ctx, S, N):
    from pyvbmc_amd import _lib

    alpha, L = np.empty((S, N)), np.empty((S, N, N))
    ctx.check(ctx._lib.vbmc_gp_fetch(ctx._h, _lib.ptr(alpha), _lib.ptr(L)))
    return alpha, L


# --------------------------------------------------------------------------- 1. stage by stage, the existing entries' bits
@pytest.mark.parametrize("key", gfc.KEYS)
def test_stages_equal_the_existing_entries(ctx, base, key):
    from pyvbmc_amd.gp import fit_rank, fit_select

    cs, o = gfc.case(key), base[key]
    B = gfc.H + gfc.INIT_N
    assert o.cand.shape == (B, cs.P)
    # scores: vbmc_gp_hyp_optimize's log posterior at a start (max_iter = 0), an invalid start where the score is -inf
    rc, _, lpost, _, _, inv, _, _ = raw_opt(ctx, cs, o.cand, trace=False, max_iter=0)
    assert rc == 0
    assert np.array_equal(inv != 0, np.isneginf(o.score))
    assert np.array_equal(o.score[inv == 0], lpost[inv == 0]) and np.all(np.isfinite(o.score[inv == 0]))
    # the starts are the rank's first rows; the optimiser's outputs those of the existing entry from the same starts
    _, order = fit_rank(o.score)
    assert np.array_equal(o.starts, order[: gfc.OPTS_N])
    ref = raw_opt(ctx, cs, o.cand[o.starts], trace=False)
    assert ref[0] == 0 and not np.any(ref[5])
    assert np.array_equal(o.o_hyp, ref[1]) and np.array_equal(o.o_lp, ref[2]) and np.array_equal(o.o_stats, ref[4])
    assert np.array_equal(o.o_inv, ref[5])
    # the optimum by the package's rule
    k, f = fit_select(float(o.score[order[0]]), o.o_lp, o.o_inv)
    assert o.best_lp[0] == f and np.array_equal(o.best, o.o_hyp[k] if k >= 0 else o.cand[order[0]])
    # the chains: the existing entry from the tiled optimum under the same seed
    rc, smp, lpost, lprior, stats, inv = gfc.raw_sample(ctx, cs, np.tile(o.best, (gfc.N_SAMPLES, 1)))
    assert rc == 0 and not np.any(inv)
    assert np.array_equal(o.hyp, smp) and np.array_equal(o.lpost, lpost) and np.array_equal(o.lprior, lprior)
    assert np.array_equal(o.stats, stats)
    assert len({tuple(r) for r in o.hyp}) == gfc.N_SAMPLES  # (the chains differ: each has its own stream)
    # the posterior: vbmc_gp_posterior at the samples, with the noise the fit reports
    assert np.allclose(o.noise, np.exp(2 * o.hyp[:, cs.D + 1]), rtol=4 * np.finfo(np.float64).eps, atol=0)  # (two exps, < 1 ulp each)
    rc, alpha, L = gfc.raw_posterior(ctx, cs, o.hyp, o.noise)
    assert rc == 0 and np.array_equal(o.alpha, alpha) and np.array_equal(o.L, L)
    print(f"case {key}: starts {list(o.starts)}, optimum {o.best_lp[0]:.6f} (best candidate {o.score[order[0]]:.6f}), "
          f"{int(np.sum(np.isneginf(o.score)))} candidates without a finite score")


@pytest.mark.parametrize("key", gfc.KEYS)
def test_design(base, key):
    from pyvbmc_amd.gp import fit_design

    cs, o = gfc.case(key), base[key]
    dlb, dub = gfc.design_box(cs)
    drawn = o.cand[gfc.H :]
    assert np.array_equal(drawn, gfc.design_rows(gfc.INIT_N, dlb, dub, gfc.SEED))
    assert np.array_equal(drawn, fit_design(gfc.INIT_N, dlb, dub, gfc.SEED))
    assert np.all(drawn >= dlb) and np.all(drawn <= dub)
    assert np.array_equal(o.cand[: gfc.H], np.clip(cs.x0[: gfc.H], cs.lb, cs.ub))
    assert len({tuple(r) for r in drawn}) == gfc.INIT_N


# ----------------------------------------------------------------------------------------------------- 2. the ranking
def overflow_case():
    """Case 63 with an output-scale bound that lets exp(2 log sf) overflow: such a row's covariance is not finite."""
    cs = gfc.case(63)
    ub = cs.ub.copy()
    ub[cs.D] = 400.0
    bad = cs.x0[1].copy()
    bad[cs.D] = 400.0
    return cs, ub, bad


def test_rank_non_pd_last_and_ties_by_index(ctx):
    from pyvbmc_amd.gp import fit_rank

    cs, ub, bad = overflow_case()
    B = gfc.H + gfc.INIT_N
    hyp0 = np.vstack([cs.x0[0], bad, cs.x0[0]])  # row 1 not positive definite, row 2 a duplicate of row 0
    o = gfc.raw_fit(ctx, cs, hyp0=hyp0, ub=ub, opts_N=B, max_iter=0, n_samples=0)  # (every candidate a start: the whole order)
    assert o.rc == 0 and o.status[0] == 0
    assert np.isneginf(o.score[1]) and o.score[0] == o.score[2] and np.isfinite(o.score[0])
    assert sorted(o.starts) == list(range(B)) and np.array_equal(o.starts, fit_rank(o.score)[1])
    n_bad = int(np.sum(np.isneginf(o.score)))
    assert list(o.starts[B - n_bad :]) == sorted(np.flatnonzero(np.isneginf(o.score))) and 1 in o.starts[B - n_bad :]
    where = list(o.starts)
    assert where.index(2) == where.index(0) + 1
    assert np.array_equal(o.o_inv != 0, np.isneginf(o.score[o.starts]))  # a start without a finite score is an invalid run
    assert np.all(np.diff(o.score[o.starts]) <= 0)


def test_third_run_invalid_with_two_finite_candidates(ctx):
    cs, ub, bad = overflow_case()
    hyp0 = np.vstack([cs.x0[0], bad, cs.x0[1]])
    o = gfc.raw_fit(ctx, cs, hyp0=hyp0, ub=ub, init_N=0, n_samples=0)
    assert o.rc == 0 and o.status[0] == 0
    assert np.isneginf(o.score[1]) and o.starts[2] == 1 and list(o.o_inv) == [0, 0, 1]
    assert not np.any(o.o_hyp[2]) and o.o_lp[2] == 0 and not np.any(o.o_stats[2])
    ref = raw_opt(ctx, cs, hyp0[o.starts[:2]], trace=False, ub=ub)
    assert ref[0] == 0 and np.array_equal(o.o_hyp[:2], ref[1]) and np.array_equal(o.o_lp[:2], ref[2])
    assert np.array_equal(o.o_stats[:2], ref[4])
    assert o.best_lp[0] == np.max(o.o_lp[:2]) and o.hyp.shape == (1, cs.P) and np.array_equal(o.hyp[0], o.best)


# -------------------------------------------------------------------------------------------------- 3. independence
def test_independent_of_chunks_and_rounds(ctx, base):
    cs, o = gfc.case(63), base[63]
    unforced = gfc.raw_fit(ctx, cs)
    assert gfc.same_fit(o, unforced)
    try:
        ctx.set_option("gp_lml_chunk", gfc.CHUNK)
        ctx.set_option("gp_opt_rounds", 1)
        ctx.set_option("gp_hyp_rounds", 1)
        one = gfc.raw_fit(ctx, cs)
    finally:
        ctx.set_option("gp_lml_chunk", 0)
        ctx.set_option("gp_opt_rounds", 4)
        ctx.set_option("gp_hyp_rounds", 4)
    assert gfc.same_fit(o, one)
    try:
        ctx.set_option("gp_lml_chunk", 2)  # fewer candidates a chunk than samples to install
        two = gfc.raw_fit(ctx, cs)
    finally:
        ctx.set_option("gp_lml_chunk", 0)
    assert gfc.same_fit(o, two)


# ------------------------------------------------------------------------------------------------ 4. stage switches
def test_stage_switches(ctx, base):
    from pyvbmc_amd.gp import fit_rank

    cs, o = gfc.case(130), base[130]
    N = cs.X.shape[0]
    # no optimiser: the optimum is the best candidate
    a = gfc.raw_fit(ctx, cs, opts_N=0)
    i0 = fit_rank(a.score)[1][0]
    assert a.rc == 0 and a.status[0] == 0 and np.array_equal(a.cand, o.cand) and np.array_equal(a.score, o.score)
    assert np.array_equal(a.best, a.cand[i0]) and a.best_lp[0] == a.score[i0] and a.hyp.shape == (gfc.N_SAMPLES, cs.P)
    got = resident(ctx, gfc.N_SAMPLES, N)
    assert np.array_equal(got[0], a.alpha) and np.array_equal(got[1], a.L) and np.all(np.isfinite(a.alpha))
    # no chains: the optimum alone is installed
    b = gfc.raw_fit(ctx, cs, n_samples=0)
    assert b.rc == 0 and b.status[0] == 0 and np.array_equal(b.best, o.best) and np.array_equal(b.hyp[0], o.best)
    assert b.lpost[0] == b.best_lp[0] == o.best_lp[0]
    got = resident(ctx, 1, N)
    ref = gfc.raw_posterior(ctx, cs, b.hyp, b.noise)
    assert np.array_equal(got[0], b.alpha) and np.array_equal(ref[1], b.alpha) and np.array_equal(ref[2], b.L)
    # no drawn candidates: the rows of hyp0 alone
    c = gfc.raw_fit(ctx, cs, init_N=0)
    assert c.rc == 0 and c.status[0] == 0 and np.array_equal(c.cand, o.cand[: gfc.H]) and np.array_equal(c.score, o.score[: gfc.H])
    assert sorted(c.starts) == [0, 1, 2] and not np.any(c.o_inv)
    got = resident(ctx, gfc.N_SAMPLES, N)
    assert np.array_equal(got[0], c.alpha) and np.all(np.isfinite(c.alpha))
    # nothing downloaded where no buffer is given: the same state stays installed
    d = gfc.raw_fit(ctx, cs, init_N=0, want_post=False)
    assert d.rc == 0 and np.array_equal(d.hyp, c.hyp)
    got = resident(ctx, gfc.N_SAMPLES, N)
    assert np.array_equal(got[0], c.alpha) and np.array_equal(got[1], c.L)


# ----------------------------------------------------------------------------------------------- 5. installed state
def test_installed_state(ctx):
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gp import upload_gp

    cs = gfc.case(63)
    gp, hyp, opt, smp = gfc.fit_package(ctx, cs, True)
    assert len(gp.posteriors) == gfc.N_SAMPLES and np.array_equal(gp.get_hyperparameters(), hyp)
    real = ctx._lib
    ctx._lib = CountingLib(real)
    try:  # the fit left its posterior installed: the upload and the predict that follow ship nothing
        upload_gp(gp, ctx)
        before = gp.predict(cs.X[:5], separate_samples=True)
        assert ctx._lib.n_set_gp == 0 and np.all(np.isfinite(before[0])) and np.all(before[1] > 0)
        # no candidate has a finite score: ValueError, and the installed GP is what it was
        _, ub, bad = overflow_case()
        other = gfc.make_gp(ctx, cs)
        other.set_bounds({"lb": cs.lb, "ub": ub})
        other.set_priors(cs.priors)
        with pytest.raises(ValueError, match="no candidate has a finite log posterior"):
            other.fit(hyp0=bad[None, :], options={"init_N": 0, "opts_N": 2, "n_samples": 2}, seed=1, optimizer="fused")
        o = gfc.raw_fit(ctx, cs, hyp0=bad[None, :], ub=ub, init_N=0)
        assert o.rc == 0 and o.status[0] == 1 and np.isneginf(o.score[0]) and list(o.o_inv) == [1]
        # a refused call
        assert gfc.raw_fit(ctx, cs, thin=0).rc == _lib.E_ARG
        after = gp.predict(cs.X[:5], separate_samples=True)
        assert ctx._lib.n_set_gp == 0
    finally:
        ctx._lib = real
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


# ------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(ctx):
    from pyvbmc_amd import _lib

    cs = gfc.case(63)
    dlb, dub = gfc.design_box(cs)
    low, high = dlb.copy(), dub.copy()
    low[2], high[0] = cs.lb[2] - 0.1, cs.ub[0] + 0.1
    for bad in (dict(dlb=low), dict(dub=high), dict(dlb=dub, dub=dlb), dict(hyp0=np.zeros((0, cs.P)), init_N=0),
                dict(init_N=-1), dict(opts_N=-1), dict(n_samples=-1), dict(thin=0), dict(burn=-1), dict(m=0), dict(m=17),
                dict(max_iter=-1), dict(tol_g=-1.0), dict(tol_f=np.nan), dict(widths=np.zeros(cs.P)),
                dict(ub=np.full(cs.P, np.inf)), dict(lb=cs.ub + 1.0), dict(mean=gp_ref.MEAN_ZERO)):
        assert gfc.raw_fit(ctx, cs, **bad).rc == _lib.E_ARG, bad
    # a noise bound below 1e-6 (without the case's s2): VBMC_E_UNSUP -- and VBMC_E_ARG where an argument is bad as well
    lb = cs.lb.copy()
    lb[cs.D + 1] = np.log(1e-4)
    assert gfc.raw_fit(ctx, cs, lb=lb, no_s2=True).rc == _lib.E_UNSUP
    assert gfc.raw_fit(ctx, cs, lb=lb, no_s2=True, dlb=low).rc == _lib.E_ARG
    assert gfc.raw_fit(ctx, cs, lb=lb, init_N=2, opts_N=1, n_samples=1, max_iter=1).rc == 0  # (min s2 keeps sn2_div above 1e-6)


# --------------------------------------------------------------------------- 7. the package's two routes, device vs host
@pytest.mark.parametrize("key", gfc.KEYS)
def test_fused_device_against_fused_host(ctx, key):
    cs = gfc.case(key)
    host = gfc.fit_package(None, cs, False)
    dev = gfc.fit_package(ctx, cs, True)
    ho, do = host[2], dev[2]
    assert np.array_equal(do["candidates"], ho["candidates"])
    # candidate scores: the bound tests/test_gp_lml_gpu.py uses for device against host lml (f vabs), plus the prior's
    fin = np.isfinite(ho["candidate_log_post"])
    assert np.array_equal(fin, np.isfinite(do["candidate_log_post"]))
    worst = 0.0
    for j in np.flatnonzero(fin):
        v = cs.evaluate(do["candidates"][j])
        err = abs(do["candidate_log_post"][j] - ho["candidate_log_post"][j])
        assert abs(-do["candidate_log_post"][j] - v["phi"]) <= v["e_phi"] and err <= v["e_phi"], (key, j, err, v["e_phi"])
        worst = max(worst, err / v["e_phi"])
    diff = do["log_post"] - ho["log_post"]
    print(f"case {key}: candidate scores differ by at most {worst:.2e} of the bound; optimum {do['log_post']:.10f} on the "
          f"device, {ho['log_post']:.10f} on the host: {diff:+.3e}")
    assert abs(diff) <= SCIPY_MARGIN
    assert dev[1].shape == host[1].shape == (gfc.N_SAMPLES, cs.P)
    assert np.all(dev[1] >= cs.lb) and np.all(dev[1] <= cs.ub) and dev[3]["samples"].shape == (gfc.N_SAMPLES, cs.P)


# ------------------------------------------------------------------------------------- 8. train_gp, end to end
def test_train_gp_on_the_device_twice(ctx):
    """The reference-named function over the fused fit at D = 2, N = 63, on stand-ins (tests/train_gp_cases.py): twice in
    a row, the second call with the first call's GP in the history."""
    import train_gp_cases as tc
    from pyvbmc_amd.gp import upload_gp
    from test_train_gp_host import check_results, run_twice

    opts, first, second, gp1, _ = run_twice(True, ctx)
    check_results(opts, first, second, gp1)
    gp = second[0][0]
    X, _, _ = tc.data()
    real = ctx._lib
    ctx._lib = CountingLib(real)
    try:  # the second fit's posterior is the installed one: predicting at the training inputs uploads nothing
        upload_gp(gp, ctx)
        fmu, fs2 = gp.predict(X, separate_samples=True)
        assert ctx._lib.n_set_gp == 0
    finally:
        ctx._lib = real
    assert fmu.shape == (tc.N, 3) and np.all(np.isfinite(fmu)) and np.all(fs2 > 0)
    assert all(p.L is not None and p.L_chol for p in gp.posteriors)
