"""GPU tests of hyper-parameter optimisation on the device: ``vbmc_gp_hyp_optimize`` (csrc/gp_opt.hip,
csrc/api_gp_opt.hip) and ``pyvbmc_amd.gp.optimize_hyperparameters`` / ``GP.fit(optimizer="lockstep")`` over it.

The trace check is teacher-forced: every step of every run is recomputed on the host from the device's OWN trace rows
(tests/gp_opt_host.py's pieces), so it does not rest on two trajectories staying close.  Then what the entry point
promises: the results, independence of R, of the chunking, of the rounds per read and of the trace, the installed GP
untouched, invalid starts, the refusals, and ``GP.fit``."""
import ctypes as C

import numpy as np
import pytest

import gp_opt_host as goh
from oracle import gp_ref
from test_gp_opt_host import SCIPY_MARGIN, projected_gradient_ok
from test_gp_post_gpu import CountingLib, mirror_gp

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


def raw(ctx, cs, x0, *, trace=True, lb=None, ub=None, max_iter=None, m=None, tol_g=None, tol_f=None, mean=None, X=None,
        y=None):
    """The entry point itself on a case: ``(rc, hyp, log_post, grad, stats, invalid, trace_iter, trace_eval)``."""
    from pyvbmc_amd import _lib

    X = _lib.f64(cs.X if X is None else X)
    y = _lib.f64(np.ravel(cs.y if y is None else y))
    N, D = X.shape
    x0 = _lib.f64(np.atleast_2d(x0))
    R, P = x0.shape
    s2 = None if cs.s2 is None else _lib.f64(np.ravel(cs.s2))
    max_iter = cs.max_iter if max_iter is None else max_iter
    arr = [_lib.f64(cs.lb if lb is None else lb), _lib.f64(cs.ub if ub is None else ub), _lib.f64(cs.priors["mu"]),
           _lib.f64(cs.priors["sigma"]), _lib.f64(cs.priors["df"])]
    cap = max(max_iter, 0) + 1
    hyp, lpost, grad = np.full((R, P), 7.0), np.full(R, 7.0), np.full((R, P), 7.0)
    stats, inv = np.full((R, 4), 7, dtype=np.int64), np.full(R, 7, dtype=np.int32)
    t_it = np.full((R, cap, 3 * P + 3), 7.0) if trace else None
    t_ev = np.full((R, 1 + 31 * cap, 4), 7.0) if trace else None
    rc = ctx._lib.vbmc_gp_hyp_optimize(
        ctx._h, N, D, P, cs.mean if mean is None else mean, _lib.ptr(X), _lib.ptr(y), _lib.ptr(s2), R, _lib.ptr(x0),
        *[_lib.ptr(a) for a in arr], max_iter, cs.m if m is None else m, cs.tol_g if tol_g is None else tol_g,
        cs.tol_f if tol_f is None else tol_f, cap if trace else 0, _lib.ptr(hyp), _lib.ptr(lpost), _lib.ptr(grad),
        stats.ctypes.data_as(C.POINTER(C.c_int64)), inv.ctypes.data_as(C.POINTER(C.c_int32)), _lib.ptr(t_it), _lib.ptr(t_ev))
    return rc, hyp, lpost, grad, stats, inv, t_it, t_ev


def same(a, b, rows=slice(None)):
    return all(np.array_equal(u[rows], v[rows]) for u, v in zip(a[1:6], b[1:6]))


def split_row(row, P):
    return row[:P], row[P], row[P + 1 : 2 * P + 1], row[2 * P + 1 : 3 * P + 1], int(row[3 * P + 1]), int(row[3 * P + 2])


def check_run(cs, key, r, stats, rows, evals):
    """One run's trace, step by step, every step from the traced numbers alone."""
    P, m, lb, ub = cs.P, cs.m, cs.lb, cs.ub
    n_it, n_ev, _, reason = (int(v) for v in stats)
    assert len(rows) == n_it + 1 and len(evals) == n_ev
    assert list(evals[0]) == [0.0, 0.0, rows[0][P], 1.0]
    pairs, e = [], 1
    worst_d, worst_v = 0.0, 0.0
    for i in range(n_it + 1):
        x, phi, g, d, held, reset = split_row(rows[i], P)
        # ---- the value and the gradient at the traced x
        v = cs.evaluate(x)
        assert abs(phi - v["phi"]) <= v["e_phi"], (key, r, i, phi, v["phi"], v["e_phi"])
        assert np.all(np.abs(g - v["g"]) <= v["e_g"]), (key, r, i)
        worst_v = max(worst_v, abs(phi - v["phi"]) / v["e_phi"], float(np.max(np.abs(g - v["g"]) / v["e_g"])))
        assert np.all(x >= lb) and np.all(x <= ub)
        in_b = goh.in_bound_set(x, g, lb, ub)
        pg = np.where(in_b, 0.0, g)
        last = i == n_it
        if last and reason != goh.STOP_SEARCH:  # the row of the point the run ended at
            assert not np.any(d) and reset == 0
            gmax = float(np.max(np.abs(pg)))
            if reason == goh.STOP_TOL_G:
                assert gmax <= cs.tol_g
            elif reason == goh.STOP_MAX_ITER:
                assert n_it == cs.max_iter and gmax > cs.tol_g
            else:
                assert reason == goh.STOP_TOL_F and i > 0
                assert rows[i - 1][P] - phi <= cs.tol_f * max(1.0, abs(phi))
            break
        assert float(np.max(np.abs(pg))) > cs.tol_g and i < cs.max_iter
        # ---- the direction from the history the rows before imply
        if reset:
            pairs = []
            assert held == 0 and np.array_equal(d, -pg)
        else:
            assert held == len(pairs) > 0
            d_host, e_d = goh.two_loop(pg, np.zeros(P), pairs, in_b, m)
            err = np.abs(d - d_host)
            assert np.all(err <= e_d), (key, r, i, err, e_d)
            with np.errstate(divide="ignore", invalid="ignore"):
                worst_d = max(worst_d, float(np.nanmax(np.where(e_d > 0, err / e_d, 0.0))))
            assert not np.any(d[in_b]) and float(g @ d) < 0.0
        # ---- the trials of this iteration
        t = goh.first_step(pg, not reset)
        accepted = False
        for k in range(goh.HALVINGS + 1):
            it_e, t_e, phit, acc = evals[e]
            e += 1
            assert it_e == i
            if k == 0:
                assert abs(t_e - t) <= 4 * P * EPS * t
            else:
                assert t_e == 0.5 * evals[e - 2][1]
            step = x + t_e * d
            xt = np.maximum(np.minimum(step, ub), lb)
            if acc:  # the point itself is the next row's x: 1 ulp per component, exactly the bound where clipped
                x_next, phi_next = rows[i + 1][:P], rows[i + 1][P]
                assert np.all(np.abs(x_next - xt) <= np.spacing(np.abs(xt)))
                assert np.array_equal(x_next[step > ub], ub[step > ub]) and np.array_equal(x_next[step < lb], lb[step < lb])
                assert phit == phi_next
                xt = x_next
            s = xt - x
            gs = float(g @ s)
            rhs = phi + goh.ARMIJO * gs
            slack = goh.ARMIJO * (goh.dot_bound(g, s, P, m) + float(np.abs(g) @ np.spacing(np.abs(xt))))
            if not np.isfinite(phit):
                assert phit == np.inf and not acc
            elif abs(phit - rhs) > slack:  # the Armijo decision on the traced numbers
                assert bool(acc) == bool(phit <= rhs), (key, r, i, k, phit, rhs)
            if acc:
                accepted = True
                break
        if not accepted:
            assert last and reason == goh.STOP_SEARCH and e == n_ev
            break
        # ---- the pair of this step, by the curvature rule
        y = rows[i + 1][P + 1 : 2 * P + 1] - g
        sy = float(s @ y)
        if sy > goh.CURV * (np.sqrt(float(s @ s)) * np.sqrt(float(y @ y))):
            pairs = (pairs[1:] if len(pairs) == m else pairs) + [(s, y)]
    assert e == n_ev
    print(f"case {key} run {r}: stats {list(stats)}; values and gradients use at most {worst_v:.2e} of their bounds, "
          f"directions {worst_d:.2e} of the carried bound")


# ------------------------------------------------------------------------------------- 1. the teacher-forced trace
@pytest.mark.parametrize("key", list(goh.CASES))
def test_trace_step_by_step(ctx, key):
    cs, ref = goh.case(key), goh.runs(key)
    rc, hyp, lpost, grad, stats, inv, t_it, t_ev = raw(ctx, cs, cs.x0)
    assert rc == 0
    assert list(inv) == [int(r["invalid"]) for r in ref]
    for r, res in enumerate(ref):
        if res["invalid"]:
            assert not np.any(hyp[r]) and not np.any(stats[r]) and not np.any(t_it[r]) and lpost[r] == 0
            continue
        n_it, n_ev = int(stats[r, 0]), int(stats[r, 1])
        assert 0 <= n_it <= cs.max_iter and 1 <= n_ev <= 1 + 31 * cs.max_iter
        check_run(cs, key, r, stats[r], t_it[r, : n_it + 1], t_ev[r, :n_ev])
        assert not np.any(t_it[r, n_it + 1 :]) and not np.any(t_ev[r, n_ev:])
        # the result is the last row
        x, phi, g = t_it[r, n_it, : cs.P], t_it[r, n_it, cs.P], t_it[r, n_it, cs.P + 1 : 2 * cs.P + 1]
        if stats[r, 3] != goh.STOP_SEARCH:
            assert np.array_equal(hyp[r], x) and lpost[r] == -phi and np.array_equal(grad[r], -g)
        # no steering comparison of these cases sits inside its bound (tests/test_gp_opt_host.py): the same decisions
        assert np.array_equal(stats[r], res["stats"]), (key, r, stats[r], res["stats"])
        d = np.abs(hyp[r] - res["x"]) / np.where(cs.ub > cs.lb, cs.ub - cs.lb, 1.0)
        print(f"case {key} run {r}: x differs from the host statement's by at most {np.max(d):.2e} of the box")


# ------------------------------------------------------------------------------------------------------ 2. results
@pytest.mark.parametrize("key", [k for k in goh.CASES if k != "invalid"])
def test_results(ctx, key):
    from pyvbmc_amd.gp import optimize_hyperparameters

    cs = goh.case(key)
    rc, hyp, lpost, grad, stats, inv, _, _ = raw(ctx, cs, cs.x0, trace=False)
    assert rc == 0 and not np.any(inv)
    for r in range(cs.x0.shape[0]):
        projected_gradient_ok(cs, hyp[r], stats[r], f"case {key} run {r}")
        v = cs.evaluate(hyp[r])
        assert abs(-lpost[r] - v["phi"]) <= v["e_phi"] and np.all(np.abs(-grad[r] - v["g"]) <= v["e_g"])
        assert np.all(hyp[r] >= cs.lb) and np.all(hyp[r] <= cs.ub)
    # through the package: the same call
    gp = mirror_gp(ctx, cs.X, cs.y, cs.mean, s2=cs.s2)
    out = optimize_hyperparameters(gp, cs.x0, lb=cs.lb, ub=cs.ub, priors=cs.priors, max_iter=cs.max_iter, history=cs.m,
                                   tol_g=cs.tol_g, tol_f=cs.tol_f, ctx=ctx)
    assert np.array_equal(out["hyp"], hyp) and np.array_equal(out["log_post"], lpost)
    assert np.array_equal(out["grad"], grad) and np.array_equal(out["stats"], stats) and "trace" not in out


def test_converged_on_the_device(ctx):
    cs = goh.OptCase(*goh.CASES[63]["args"], max_iter=200, tol_g=1e-3, tol_f=0.0)
    rc, hyp, lpost, grad, stats, inv, _, _ = raw(ctx, cs, cs.x0, trace=False)
    assert rc == 0 and not np.any(inv)
    for r in range(3):
        assert stats[r, 3] == goh.STOP_TOL_G, stats[r]
        projected_gradient_ok(cs, hyp[r], stats[r], f"converged run {r}")


# ------------------------------------------------------------------------------------------------- 3. independence
def test_independent_of_batch_chunks_rounds_and_trace(ctx):
    cs = goh.case(65)
    base = raw(ctx, cs, cs.x0)
    assert base[0] == 0
    extra = np.vstack([cs.x0, cs.x0[0] + 0.05, cs.x0[1] - 0.05])
    five = raw(ctx, cs, extra)
    assert five[0] == 0 and same(base, tuple(a[:3] if i else a for i, a in enumerate(five)))
    assert np.array_equal(base[6], five[6][:3]) and np.array_equal(base[7], five[7][:3])
    try:
        ctx.set_option("gp_lml_chunk", 2)  # chunks of 2 + 2 + 1 inside every round
        chunked = raw(ctx, cs, extra)
    finally:
        ctx.set_option("gp_lml_chunk", 0)
    assert chunked[0] == 0 and same(five, chunked) and np.array_equal(five[6], chunked[6])
    try:
        ctx.set_option("gp_opt_rounds", 1)
        one = raw(ctx, cs, cs.x0)
        ctx.set_option("gp_opt_rounds", 7)
        seven = raw(ctx, cs, cs.x0)
    finally:
        ctx.set_option("gp_opt_rounds", 4)
    assert one[0] == 0 and seven[0] == 0 and same(base, one) and same(base, seven)
    plain = raw(ctx, cs, cs.x0, trace=False)
    assert plain[0] == 0 and same(base, plain)


def test_more_runs_than_the_count_kernel_has_threads(ctx):
    """R = 257: the count of unfinished runs (one workgroup of 256 threads, csrc/lockstep.hip) takes a second trip of its
    strided loop.  Run 256 starts where run 0 does and the runs draw nothing, so it ends where run 0 does; a count that
    saw the first 256 runs alone could let the host stop before it has, with the zeros its outputs start as."""
    cs = goh.case(63)
    rng = np.random.default_rng(257)
    jit = cs.x0[np.arange(253) % 3] + 0.05 * rng.standard_normal((253, cs.P))
    x0 = np.vstack([cs.x0, np.minimum(np.maximum(jit, cs.lb), cs.ub), cs.x0[:1]])
    assert x0.shape == (257, cs.P)
    rc, hyp, lpost, grad, stats, inv, _, _ = raw(ctx, cs, x0, trace=False, max_iter=3)
    assert rc == 0
    assert np.array_equal(hyp[256], hyp[0]) and lpost[256] == lpost[0] and np.array_equal(grad[256], grad[0])
    assert np.array_equal(stats[256], stats[0])
    assert np.all(stats[:, 3] != 0), np.flatnonzero(stats[:, 3] == 0)


# ------------------------------------------------------------------------------------------- 4. the installed GP
def test_installed_gp_untouched(ctx):
    import gp_post_host as gph
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gp import fetch_posteriors, optimize_hyperparameters, upload_gp

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
    cs = goh.case(65)  # another N, D and mean than the installed GP's
    other = mirror_gp(ctx, cs.X, cs.y, cs.mean)
    out = optimize_hyperparameters(other, cs.x0, lb=cs.lb, ub=cs.ub, priors=cs.priors, max_iter=3, ctx=ctx)
    assert np.all(np.isfinite(out["log_post"]))
    assert ctx._gp_dev == key and ctx._gp_key == key
    after = resident()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    real = ctx._lib
    ctx._lib = CountingLib(real)
    try:  # the installed posterior is still the context's: the predict that follows uploads nothing
        upload_gp(gp, ctx)
        fmu, _ = gp.predict(X[:4], separate_samples=True)
        assert ctx._lib.n_set_gp == 0 and np.all(np.isfinite(fmu))
    finally:
        ctx._lib = real
    posts = fetch_posteriors(gp, ctx)  # (the records' L, left on the device so far)
    for s in range(2):
        assert np.array_equal(posts[s].L, before[1][s]) and np.array_equal(np.ravel(posts[s].alpha), before[0][s])


# ------------------------------------------------------------------------------------- 5. invalid starts, refusals
def test_invalid_start(ctx):
    from pyvbmc_amd.gp import optimize_hyperparameters

    cs = goh.case("invalid")  # run 1 does not factorise
    keep = raw(ctx, cs, cs.x0)
    assert keep[0] == 0 and list(keep[5]) == [0, 1, 0]
    good = cs.x0.copy()
    good[1] = cs.x0[0]
    ref = raw(ctx, cs, good)
    assert ref[0] == 0 and not np.any(ref[5]) and same(keep, ref, rows=[0, 2])
    bad = good.copy()
    bad[1, 2] = np.nan  # ... and a start that is not a number is invalid without an evaluation
    rc, hyp, lpost, grad, stats, inv, t_it, t_ev = nan = raw(ctx, cs, bad)
    assert rc == 0 and list(inv) == [0, 1, 0] and same(nan, ref, rows=[0, 2])
    assert not np.any(hyp[1]) and not np.any(grad[1]) and lpost[1] == 0 and not np.any(stats[1]) and not np.any(t_ev[1])
    gp = mirror_gp(ctx, cs.X, cs.y, cs.mean)
    for x0 in (cs.x0, bad):
        with pytest.raises(ValueError, match="Invalid value."):
            optimize_hyperparameters(gp, x0, lb=cs.lb, ub=cs.ub, priors=cs.priors, max_iter=cs.max_iter, ctx=ctx)


def test_refusals(ctx):
    import gp_post_host as gph
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gp import optimize_hyperparameters

    cs = goh.case(63)
    ctx.set_timing(1)
    try:
        assert raw(ctx, cs, cs.x0[:1], max_iter=1)[0] == 0
        assert ctx.last_kernel_ms(_lib.T_GP_OPT) > 0
        # a noise bound below 1e-6 (with the case's s2 >= 0.01 the bound is on their sum: take the s2 away)
        lb = cs.lb.copy()
        lb[cs.D + 1] = np.log(1e-4)
        plain = goh.OptCase(63, 3, gp_ref.MEAN_CONST, False, max_iter=2)
        assert raw(ctx, plain, plain.x0[:1], lb=lb)[0] == _lib.E_UNSUP
        with pytest.raises(ValueError, match="no timed launch"):
            ctx.last_kernel_ms(_lib.T_GP_OPT)
        assert raw(ctx, cs, cs.x0[:1], lb=lb, max_iter=1)[0] == 0  # (min s2 keeps sn2_div above 1e-6)
        # D = 33
        N, D, mean = 40, 33, gp_ref.MEAN_CONST
        X, y, hyp = gph.make_case(N, D, 1, mean, seed=100 + N)
        big = goh.OptCase.__new__(goh.OptCase)
        big.X, big.y, big.s2, big.mean, big.P = X, y, None, mean, hyp.shape[1]
        big.lb, big.ub = hyp[0] - 1.0, hyp[0] + 1.0
        big.lb[D + 1] = np.log(0.05)
        big.priors = {k: np.full(hyp.shape[1], np.nan) for k in ("mu", "sigma", "df")}
        big.max_iter, big.m, big.tol_g, big.tol_f = 2, 8, 1e-5, 1e-9
        assert raw(ctx, big, hyp)[0] == _lib.E_UNSUP
    finally:
        ctx.set_timing(0)
    # both take the host route through the package, with the host route's bits
    gp33 = mirror_gp(ctx, X, y, mean)
    kw = dict(lb=big.lb, ub=big.ub, max_iter=2)
    dev = optimize_hyperparameters(gp33, hyp, ctx=ctx, **kw)
    host = optimize_hyperparameters(gp33, hyp, device=False, **kw)
    assert all(np.array_equal(dev[k], host[k]) for k in host) and np.all(np.isfinite(dev["log_post"]))
    small = mirror_gp(ctx, plain.X[:20], plain.y[:20], plain.mean)
    kw = dict(lb=lb, ub=plain.ub, priors=plain.priors, max_iter=2)
    dev = optimize_hyperparameters(small, plain.x0[:1], ctx=ctx, **kw)
    host = optimize_hyperparameters(small, plain.x0[:1], device=False, **kw)
    assert all(np.array_equal(dev[k], host[k]) for k in host)
    # bad arguments
    for bad in (dict(max_iter=-1), dict(m=0), dict(m=17), dict(tol_g=-1.0), dict(tol_f=-1.0), dict(tol_g=np.nan),
                dict(ub=np.full(cs.P, np.inf)), dict(lb=cs.ub + 1.0), dict(mean=gp_ref.MEAN_ZERO)):
        assert raw(ctx, cs, cs.x0[:1], **bad)[0] == _lib.E_ARG, bad


# ------------------------------------------------------------------------------------------------------ 6. GP.fit
def test_fit_lockstep_on_the_device(ctx):
    from pyvbmc_amd.gp import upload_gp

    cs = goh.case(65)
    opts = {"init_N": 8, "opts_N": 2, "n_samples": 0, "tol_opt": 1e-4}

    def fit(device):
        gp = mirror_gp(ctx, cs.X, cs.y, cs.mean)
        gp.set_bounds({"lb": cs.lb, "ub": cs.ub})
        gp.set_priors(cs.priors)
        return (gp,) + gp.fit(cs.X, cs.y, None, hyp0=cs.x0, options=opts, device=device, seed=9, optimizer="lockstep")

    host = fit(False)
    gp, hyp, opt, smp = fit(True)
    assert smp is None and hyp.shape == (1, cs.P) and np.all(hyp >= cs.lb) and np.all(hyp <= cs.ub)
    assert opt["candidates"].shape == (3 + 8, cs.P) and opt["n_iterations"] > 0
    assert opt["log_post"] >= np.max(opt["candidate_log_post"])
    diff = opt["log_post"] - host[2]["log_post"]
    print(f"fit: log posterior {opt['log_post']:.10f} on the device, {host[2]['log_post']:.10f} on the host: {diff:+.3e}")
    assert abs(diff) <= SCIPY_MARGIN
    v = cs.evaluate(hyp[0])
    assert abs(-opt["log_post"] - v["phi"]) <= v["e_phi"]
    # the posterior of the optimum is left installed: the upload that follows ships nothing
    assert len(gp.posteriors) == 1 and np.array_equal(gp.get_hyperparameters(), hyp)
    real = ctx._lib
    ctx._lib = CountingLib(real)
    try:
        upload_gp(gp, ctx)
        assert ctx._lib.n_set_gp == 0
        fmu, _ = gp.predict(cs.X[:4], separate_samples=True)
        assert ctx._lib.n_set_gp == 0 and np.all(np.isfinite(fmu))
    finally:
        ctx._lib = real
