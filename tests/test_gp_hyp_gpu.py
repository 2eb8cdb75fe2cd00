"""GPU tests of GP hyper-parameter sampling on the device: ``vbmc_gp_hyp_sample`` (csrc/gp_hyp.hip, csrc/api_gp_hyp.hip)
and ``pyvbmc_amd.gp.sample_hyperparameters`` / ``GP.fit`` over it.  The chains are replayed against tests/slice_host.py
over the host statement of the target (tests/hyp_slice_host.py), whose cases are certain to take the same decisions
(tests/test_hyp_slice_host.py asserts the margins); then what the entry point promises: independence of C, of the
chunking and of the rounds per read, the installed GP untouched, an invalid start, the refusals, and ``GP.fit``."""
import ctypes as C

import numpy as np
import pytest

import hyp_slice_host as hs
from oracle import gp_ref
from test_gp_post_gpu import CountingLib, mirror_gp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


def raw(ctx, cs, x0, *, lb=None, ub=None, widths=None, n=None, thin=None, burn_in=None, seed=None, X=None, y=None,
        mean=None):
    """The entry point itself on a case: ``(rc, samples, log_post, log_priors, stats, invalid)``."""
    from pyvbmc_amd import _lib

    X = _lib.f64(cs.X if X is None else X)
    y = _lib.f64(np.ravel(cs.y if y is None else y))
    N, D = X.shape
    x0 = _lib.f64(np.atleast_2d(x0))
    Cn, P = x0.shape
    n = cs.n if n is None else n
    s2 = None if cs.s2 is None else _lib.f64(np.ravel(cs.s2))
    arr = [_lib.f64(cs.widths if widths is None else widths), _lib.f64(cs.lb if lb is None else lb),
           _lib.f64(cs.ub if ub is None else ub), _lib.f64(cs.priors["mu"]), _lib.f64(cs.priors["sigma"]),
           _lib.f64(cs.priors["df"])]
    smp, lpost, lpri = np.full((Cn, n, P), 7.0), np.full((Cn, n), 7.0), np.full((Cn, n), 7.0)
    stats, inv = np.full((Cn, 4), 7, dtype=np.int64), np.full(Cn, 7, dtype=np.int32)
    rc = ctx._lib.vbmc_gp_hyp_sample(
        ctx._h, N, D, P, cs.mean if mean is None else mean, _lib.ptr(X), _lib.ptr(y), _lib.ptr(s2), Cn, _lib.ptr(x0),
        *[_lib.ptr(a) for a in arr], n, cs.thin if thin is None else thin, cs.burn_in if burn_in is None else burn_in,
        C.c_uint64(cs.seed if seed is None else seed), _lib.ptr(smp), _lib.ptr(lpost), _lib.ptr(lpri),
        stats.ctypes.data_as(C.POINTER(C.c_int64)), inv.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, smp, lpost, lpri, stats, inv


def same(a, b, rows=slice(None)):
    return all(np.array_equal(u[rows], v[rows]) for u, v in zip(a[1:], b[1:]))


def within_host_bound(cs, h, f_dev, what):
    """|f_dev - host f(h)| <= factor_of(h) vabs + 16 eps sum_p (|c_p| + |v_p|), the host statement evaluated AT h."""
    v = cs.value(h)
    bound = v["lml_bound"] + v["prior_bound"]
    err = abs(f_dev - v["f"])
    print(f"{what}: |f_dev - f_host| = {err:.3e} uses {err / bound:.2e} of its bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


# ---------------------------------------------------------------------------------------------------- 1. the replay
@pytest.mark.parametrize("key", list(hs.CASES))
def test_replay(ctx, key):
    cs, ref = hs.case(key), hs.replay(key)
    rc, smp, lpost, lpri, stats, inv = raw(ctx, cs, cs.x0)
    assert rc == 0 and not np.any(inv)
    for c, r in enumerate(ref):
        assert np.array_equal(stats[c], r["stats"]), (c, stats[c], r["stats"])
        d = np.abs(smp[c] - r["samples"]) / (cs.ub - cs.lb)
        print(f"case {key} chain {c}: stats {list(stats[c])}, samples differ by at most {np.max(d):.2e} of the box")
        assert np.all(d <= 1e-12)
        for k in range(cs.n):
            within_host_bound(cs, smp[c, k], lpost[c, k], f"case {key} chain {c} sample {k}")
            assert abs(lpri[c, k] - hs.log_prior(smp[c, k], cs.priors)) <= hs.prior_bound(smp[c, k], cs.priors)
    # through the package: the same call
    from pyvbmc_amd.gp import sample_hyperparameters

    gp = mirror_gp(ctx, cs.X, cs.y, cs.mean, s2=cs.s2)
    out = sample_hyperparameters(gp, cs.x0, lb=cs.lb, ub=cs.ub, widths=cs.widths, priors=cs.priors, n=cs.n, thin=cs.thin,
                                 burn_in=cs.burn_in, seed=cs.seed, ctx=ctx)
    assert np.array_equal(out["samples"], smp) and np.array_equal(out["log_post"], lpost)
    assert np.array_equal(out["log_priors"], lpri) and np.array_equal(out["stats"], stats)


# ------------------------------------------------------------------------------------------------- 2. independence
def test_independent_of_batch_chunks_and_rounds(ctx):
    cs = hs.case(65)
    base = raw(ctx, cs, cs.x0)
    assert base[0] == 0
    extra = np.vstack([cs.x0, cs.x0[0] + 0.05, cs.x0[1] - 0.05])
    five = raw(ctx, cs, extra)
    assert five[0] == 0 and same(base, tuple(a[:3] if i else a for i, a in enumerate(five)))
    try:
        ctx.set_option("gp_lml_chunk", 2)  # chunks of 2 + 2 + 1 inside every round
        chunked = raw(ctx, cs, extra)
    finally:
        ctx.set_option("gp_lml_chunk", 0)
    assert chunked[0] == 0 and same(five, chunked)
    try:
        ctx.set_option("gp_hyp_rounds", 1)
        one = raw(ctx, cs, cs.x0)
        ctx.set_option("gp_hyp_rounds", 7)
        seven = raw(ctx, cs, cs.x0)
    finally:
        ctx.set_option("gp_hyp_rounds", 4)
    assert one[0] == 0 and seven[0] == 0 and same(base, one) and same(base, seven)


def test_more_chains_than_the_count_kernel_has_threads(ctx):
    """C = 257: the count of unfinished chains (one workgroup of 256 threads, csrc/lockstep.hip) takes a second trip of
    its strided loop.  A count that saw the first 256 chains alone would let the host stop while chain 256 still runs,
    and its outputs would be the zeros they start as."""
    cs = hs.case(65)
    kw = dict(n=1, thin=1, burn_in=0)
    rng = np.random.default_rng(257)
    jit = cs.x0[np.arange(254) % 3] + 0.05 * rng.standard_normal((254, cs.P))
    x0 = np.vstack([cs.x0, np.minimum(np.maximum(jit, cs.lb), cs.ub)])
    assert x0.shape == (257, cs.P)
    three = raw(ctx, cs, cs.x0, **kw)
    rc, smp, lpost, lpri, stats, inv = out = raw(ctx, cs, x0, **kw)
    assert three[0] == 0 and rc == 0 and not np.any(inv)
    assert np.all(stats[:, 0] > 0)
    assert same(three, tuple(a[:3] if i else a for i, a in enumerate(out)))
    assert np.all(smp[256, 0] >= cs.lb) and np.all(smp[256, 0] <= cs.ub)
    within_host_bound(cs, smp[256, 0], lpost[256, 0], "chain 256 of 257")


# ------------------------------------------------------------------------------------------- 3. the installed GP
def test_installed_gp_untouched(ctx):
    import gp_post_host as gph
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gp import fetch_posteriors, sample_hyperparameters

    N, D, mean = 70, 2, gp_ref.MEAN_CONST
    X, y, hyp = gph.make_case(N, D, 2, mean, seed=100 + N)
    gp = mirror_gp(ctx, X, y, mean)
    gp.update(hyp=hyp, device=True, fetch=False)
    key = list(ctx._gp_dev)

    def resident():
        alpha, L = np.empty((2, N)), np.empty((2, N, N))
        ctx.check(ctx._lib.vbmc_gp_fetch(ctx._h, _lib.ptr(alpha), _lib.ptr(L)))
        return alpha, L

    before = resident()
    cs = hs.case(65)  # another N, D and mean than the installed GP's
    other = mirror_gp(ctx, cs.X, cs.y, cs.mean)
    out = sample_hyperparameters(other, cs.x0, lb=cs.lb, ub=cs.ub, widths=cs.widths, priors=cs.priors, n=1, seed=3, ctx=ctx)
    assert np.all(np.isfinite(out["log_post"]))
    assert ctx._gp_dev == key and ctx._gp_key == key
    after = resident()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    posts = fetch_posteriors(gp, ctx)  # (the records' L, left on the device so far)
    for s in range(2):
        assert np.array_equal(posts[s].L, before[1][s]) and np.array_equal(np.ravel(posts[s].alpha), before[0][s])


# ----------------------------------------------------------------------------------------------- 4. invalid start
def test_invalid_start(ctx):
    from pyvbmc_amd.gp import sample_hyperparameters

    cs = hs.case(65)
    bad = cs.x0.copy()
    bad[1, 2] = np.nan
    rc, smp, lpost, lpri, stats, inv = raw(ctx, cs, bad)
    assert rc == 0 and list(inv) == [0, 1, 0]
    assert not np.any(smp[1]) and not np.any(lpost[1]) and not np.any(lpri[1]) and not np.any(stats[1])
    # (the chain index is part of the stream, so the comparison is with a run that keeps the indices)
    keep = raw(ctx, cs, cs.x0)
    for a, b in zip((smp, lpost, lpri, stats), keep[1:5]):
        assert np.array_equal(a[[0, 2]], b[[0, 2]])
    gp = mirror_gp(ctx, cs.X, cs.y, cs.mean)
    with pytest.raises(ValueError, match="Invalid value."):
        sample_hyperparameters(gp, bad, lb=cs.lb, ub=cs.ub, widths=cs.widths, priors=cs.priors, seed=cs.seed, ctx=ctx)


# --------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals(ctx):
    import gp_post_host as gph
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gp import sample_hyperparameters

    cs = hs.case(63)
    ctx.set_timing(1)
    try:
        assert raw(ctx, cs, cs.x0[:1], n=1, thin=1, burn_in=0)[0] == 0
        assert ctx.last_kernel_ms(_lib.T_GP_HYP) > 0
        # a noise bound below 1e-6 (with the case's s2 >= 0.01 the bound is on their sum: take the s2 away)
        lb = cs.lb.copy()
        lb[cs.D + 1] = np.log(1e-4)
        plain = hs.Case(63, 3, gp_ref.MEAN_CONST, False, 2)
        assert raw(ctx, plain, plain.x0[:1], lb=lb)[0] == _lib.E_UNSUP
        with pytest.raises(ValueError, match="no timed launch"):
            ctx.last_kernel_ms(_lib.T_GP_HYP)
        assert raw(ctx, cs, cs.x0[:1], lb=lb)[0] == 0  # (min s2 keeps sn2_div above 1e-6)
        # D = 33
        N, D, mean = 40, 33, gp_ref.MEAN_CONST
        X, y, hyp = gph.make_case(N, D, 1, mean, seed=100 + N)
        big = hs.Case.__new__(hs.Case)
        big.X, big.y, big.s2, big.mean, big.seed, big.n, big.thin, big.burn_in = X, y, None, mean, 1, 1, 1, 0
        big.lb, big.ub, big.widths = hyp[0] - 1.0, hyp[0] + 1.0, np.full(hyp.shape[1], 0.5)
        big.lb[D + 1] = np.log(0.05)
        big.priors = {k: np.full(hyp.shape[1], np.nan) for k in ("mu", "sigma", "df")}
        assert raw(ctx, big, hyp)[0] == _lib.E_UNSUP
        with pytest.raises(ValueError, match="no timed launch"):
            ctx.last_kernel_ms(_lib.T_GP_HYP)
    finally:
        ctx.set_timing(0)
    # both take the host route through the package, with the host route's bits
    gp33 = mirror_gp(ctx, X, y, mean)
    kw = dict(lb=big.lb, ub=big.ub, widths=big.widths, n=1, seed=4)
    dev = sample_hyperparameters(gp33, hyp, ctx=ctx, **kw)
    host = sample_hyperparameters(gp33, hyp, device=False, **kw)
    assert all(np.array_equal(dev[k], host[k]) for k in host) and np.all(np.isfinite(dev["log_post"]))
    small = mirror_gp(ctx, plain.X[:20], plain.y[:20], plain.mean)
    kw = dict(lb=lb, ub=plain.ub, widths=plain.widths, priors=plain.priors, n=1, seed=4)
    dev = sample_hyperparameters(small, plain.x0[:1], ctx=ctx, **kw)
    host = sample_hyperparameters(small, plain.x0[:1], device=False, **kw)
    assert all(np.array_equal(dev[k], host[k]) for k in host)
    # bad arguments
    for bad in (dict(n=0), dict(thin=0), dict(burn_in=-1), dict(widths=0 * cs.widths), dict(ub=np.full(cs.P, np.inf)),
                dict(lb=cs.ub + 1.0), dict(mean=gp_ref.MEAN_ZERO)):
        assert raw(ctx, cs, cs.x0[:1], **bad)[0] == _lib.E_ARG, bad
    gp = mirror_gp(ctx, cs.X, cs.y, cs.mean, s2=cs.s2)
    with pytest.raises(ValueError):
        sample_hyperparameters(gp, cs.x0[:1], lb=cs.lb, ub=cs.ub, widths=-cs.widths, ctx=ctx)


# ------------------------------------------------------------------------------------------------------ 6. GP.fit
def test_fit_on_the_device(ctx):
    from pyvbmc_amd.gp import upload_gp

    cs = hs.case(65)
    gp = mirror_gp(ctx, cs.X, cs.y, cs.mean)
    gp.set_bounds({"lb": cs.lb, "ub": cs.ub})
    gp.set_priors(cs.priors)
    opts = {"init_N": 16, "opts_N": 1, "n_samples": 3, "thin": 1, "burn": 1, "widths": cs.widths, "tol_opt": 1e-4}
    hyp, opt, smp = gp.fit(cs.X, cs.y, None, hyp0=cs.x0, options=opts, device=True, seed=9)
    assert hyp.shape == (3, cs.P) and opt["candidates"].shape == (3 + 16, cs.P)
    assert np.all(hyp >= cs.lb) and np.all(hyp <= cs.ub)
    assert opt["log_post"] >= np.max(opt["candidate_log_post"])
    for s in range(3):
        within_host_bound(cs, hyp[s], smp["log_post"][s], f"fit sample {s}")
    # the posterior of the samples is left installed: the upload that follows ships nothing
    assert len(gp.posteriors) == 3 and np.array_equal(gp.get_hyperparameters(), hyp)
    real = ctx._lib
    ctx._lib = CountingLib(real)
    try:
        upload_gp(gp, ctx)
        assert ctx._lib.n_set_gp == 0
        fmu, _ = gp.predict(cs.X[:4], separate_samples=True)
        assert ctx._lib.n_set_gp == 0 and np.all(np.isfinite(fmu))
    finally:
        ctx._lib = real
