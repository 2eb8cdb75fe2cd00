"""The CMA-ES refinement of the acquisition search on the device (csrc/cmaes.hip, csrc/api_cmaes.hip,
pyvbmc_amd.active_search.refine) against the NumPy statement tests/cmaes_host.py.

What makes the replay certain is asserted on the CPU (tests/test_cmaes_host.py): over every whole run the ranked values lie
at least 1000 acquisition parity bounds apart, so the device ranks every generation as the host does and ``stats`` must be
EQUAL.  The state then differs only by the few ulp of exp, 1 / sqrt, 1 / sigma and the normals, amplified by the
recursion: the tolerance per quantity is 100 times the deviation of the statement's own twin (cmaes_host.drift_bounds,
computed here, not hard-coded; profiles/search_cmaes.md records the figures) -- ``x_best`` and ``mean`` in units of the box,
``sigma`` relative, ``C`` relative to max |C|.  A quantity the twin reproduces exactly keeps a floor of 4 eps before the
factor.  An integer column of ``x_best`` comes out of the transformer pair, which the twin does not perturb: it is held
to the device transformer's own bound, rtol 1e-12 (tests/test_transform_gpu.py, tests/test_search_gpu.py).  Values:
1e-9 max(1, |value|), the project's acquisition parity bound.
"""
import ctypes as C
from types import SimpleNamespace

import cmaes_host as ch
import numpy as np
import pytest
import search_host as sh
from helpers import PlainGP

pytestmark = pytest.mark.gpu

CASES = list(ch.SPECS)


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def device_setup(k, ctx):
    """The package's objects for a replay case, and the scoring arguments with everything uploaded."""
    from pyvbmc_amd import acquisition, active_search

    gp = PlainGP(k.ogp)
    gp._ctx = ctx
    gp.temporary_data["X_rescaled"] = k.X_rescaled
    gp.temporary_data["sn2_new"] = k.sn2_new
    vp = sh.package_vp(k.case, ctx)
    c = k.case
    flog = SimpleNamespace(X=c.flog.X, y=c.flog.y, X_flag=c.flog.X_flag, parameter_transformer=c.pt, y_max=k.y_max)
    state = dict(k.state)
    if k.ais is not None:
        state["active_importance_sampling"] = k.ais
    acq = getattr(acquisition, k.acq)()
    args = active_search._scoring_args(acq, gp, vp, flog, state, ctx, k.D)
    return SimpleNamespace(gp=gp, vp=vp, flog=flog, state=state, acq=acq, args=args,
                           int_bits=active_search._int_bits(state["integer_vars"], k.D))


def device_run(k, s, ctx, x0=None, max_fevals=None, seed=None):
    from pyvbmc_amd import active_search

    kind, y_max, tol_var, u, noise, use_xf = s.args
    return active_search.cmaes_resident(ctx, k.D, kind, y_max, tol_var, u, noise, use_xf, s.state["lb_eps_orig"],
                                        s.state["ub_eps_orig"], k.x0 if x0 is None else x0, k.sigma0, k.lb, k.ub,
                                        int_bits=s.int_bits, lam=k.lam, max_fevals=k.max_fevals if max_fevals is None else max_fevals,
                                        tol_fun=k.tol_fun, seed=k.seed if seed is None else seed)


@pytest.fixture(scope="module")
def host(golden):
    """Every replay case with its run of the statement and its drift bounds, computed once."""
    out = {}
    for name in CASES:
        k = ch.build_case(name, golden)
        es = ch.replay(k)
        bounds, dev, same = ch.drift_bounds(k, es)
        assert same and es.gap >= 1000 * ch.PARITY and es.tied_rows_only  # (tests/test_cmaes_host.py)
        out[name] = (k, es, bounds)
    return out


def value_close(a, b):
    return abs(a - b) <= 1e-9 * max(1.0, abs(b))


def check_state(tag, k, s, out, r, es, bounds):
    """Run r of a device result against a run of the statement."""
    np.testing.assert_array_equal(out.stats[r], es.stats, err_msg=tag)
    box = k.ub - k.lb
    iv = s.state["integer_vars"]
    iv = np.zeros(k.D, dtype=bool) if iv is None else np.asarray(iv, dtype=bool)
    err = {"x_best": float(np.max(np.abs(out.x_best[r] - es.x_best)[~iv] / box[~iv])),
           "mean": float(np.max(np.abs(out.mean[r] - es.mean) / box)),
           "sigma": abs(out.sigma[r] - es.sigma) / es.sigma,
           "C": float(np.max(np.abs(out.C[r] - es.C)) / np.max(np.abs(es.C)))}
    print(tag, "stats", out.stats[r].tolist(), "error / bound",
          {q: f"{err[q]:.2e} / {bounds[q]:.2e}" for q in err})
    for q in err:
        assert err[q] <= bounds[q], (tag, q, err[q], bounds[q])
    if iv.any():
        np.testing.assert_allclose(out.x_best[r][iv], es.x_best[iv], rtol=1e-12, atol=0)
    assert value_close(out.f0[r], es.f0) and value_close(out.f_best[r], es.f_best), (tag, out.f0[r], es.f0, out.f_best[r], es.f_best)


def check_properties(tag, k, s, out, r):
    assert out.f_best[r] <= out.f0[r], tag
    assert np.all(out.x_best[r] >= k.lb) and np.all(out.x_best[r] <= k.ub), tag
    assert not sh.hard_bound_mask(out.x_best[r][None, :], k.case.pt, s.state)[0], tag
    iv = s.state["integer_vars"]
    if iv is not None and np.any(iv):
        xo = k.case.pt.inverse(out.x_best[r][None, :])[0][np.asarray(iv, dtype=bool)]
        assert np.max(np.abs(xo - np.around(xo))) < 1e-9, tag


# ---------------------------------------------------------------------------------------------- 1. first generations
@pytest.mark.parametrize("name", ["d5", "b_int"])
def test_first_generations(ctx, host, name):
    k, _, _ = host[name]
    s = device_setup(k, ctx)
    f0_host = float(ch.objective(k)(ch.evaluated(k)(k.x0[None, :].copy()))[0])
    for g in (1, 2, 3):
        kg = SimpleNamespace(**{**vars(k), "max_fevals": 1 + g * k.lam})
        es = ch.replay(kg)
        bounds, _, same = ch.drift_bounds(kg, es)
        assert same and es.generations == g and es.stop == 3
        out = device_run(kg, s, ctx)
        check_state(f"{name} g={g}", kg, s, out, 0, es, bounds)
        assert value_close(out.f0[0], f0_host)


# ---------------------------------------------------------------------------------------------- 2. whole runs
@pytest.mark.parametrize("name", CASES)
def test_replay(ctx, host, name):
    k, es, bounds = host[name]
    s = device_setup(k, ctx)
    L0 = fetch_L(ctx, s)
    pdf0 = s.vp.pdf(k.x0[None, :], orig_flag=False)
    out = device_run(k, s, ctx)
    check_state(name, k, s, out, 0, es, bounds)
    check_properties(name, k, s, out, 0)
    # the value of the best point: the statement's acquisition and the package's own call at the device's point
    xb = out.x_best[[0]]
    v_host = float(ch.objective(k)(xb.copy())[0])
    v_own = float(np.ravel(s.acq(xb.copy(), s.gp, s.vp, s.flog, s.state))[0])
    print(name, "f_best", out.f_best[0], "host", v_host, "own", v_own)
    assert value_close(out.f_best[0], v_host) and value_close(out.f_best[0], v_own)
    # the installed GP and the mixture are untouched
    assert np.array_equal(bits(fetch_L(ctx, s)), bits(L0))
    assert np.array_equal(bits(s.vp.pdf(k.x0[None, :], orig_flag=False)), bits(pdf0))


def fetch_L(ctx, s):
    from pyvbmc_amd import _lib

    S, N = len(s.gp.posteriors), s.gp.X.shape[0]
    al, L = np.empty((S, N)), np.empty((S, N, N))
    ctx.check(ctx._lib.vbmc_gp_fetch(ctx._h, _lib.ptr(al), _lib.ptr(L)))
    return np.concatenate((al.ravel(), L.ravel()))


# ---------------------------------------------------------------------------------------------- 3. independence
def test_runs_are_independent_and_reproducible(ctx, host):
    k, es, _ = host["d5"]
    s = device_setup(k, ctx)
    r = np.random.default_rng(4)
    starts = np.vstack([k.x0] + [np.minimum(np.maximum(k.x0 + 0.3 * r.standard_normal(k.D), k.lb), k.ub) for _ in range(4)])
    kk = SimpleNamespace(**{**vars(k), "max_fevals": 1 + 12 * k.lam})
    together = device_run(kk, s, ctx, x0=starts)
    assert together.stats.shape == (5, 4)
    box = k.ub - k.lb
    identical = True
    for i in range(5):
        # run i of five = the same start alone under the key of run i: seed + i * step as run 0's seed
        alone = device_run(kk, s, ctx, x0=starts[i], seed=(k.seed + i * ch.KEY_STEP) % 2**64)
        np.testing.assert_array_equal(together.stats[i], alone.stats[0])
        for q in ("x_best", "mean"):
            assert np.max(np.abs(getattr(together, q)[i] - getattr(alone, q)[0]) / box) <= 1e-12
        identical = identical and all(np.array_equal(bits(getattr(together, q)[i]), bits(getattr(alone, q)[0]))
                                      for q in ("x_best", "mean", "sigma", "C", "f_best", "f0"))
    print("run r of R = 5 bit-identical to the start run alone:", identical)
    assert len({tuple(row) for row in np.round(together.mean, 6)}) == 5  # five different runs
    # rounds queued per read of the count: 1 against 8; and a second call
    ctx.set_option("cmaes_rounds", 1)
    one = device_run(kk, s, ctx, x0=starts)
    ctx.set_option("cmaes_rounds", 8)
    again = device_run(kk, s, ctx, x0=starts)
    for q in ("x_best", "f_best", "f0", "mean", "sigma", "C"):
        assert np.array_equal(bits(getattr(one, q)), bits(getattr(together, q))), q
        assert np.array_equal(bits(getattr(again, q)), bits(getattr(together, q))), q
    assert np.array_equal(one.stats, together.stats) and np.array_equal(again.stats, together.stats)
    for i in range(5):
        check_properties(f"run {i}", k, s, together, i)


# ---------------------------------------------------------------------------------------------- 4. the resident set
def test_resident_search_set_is_preserved(ctx, host):
    """vbmc_search_cmaes keeps its candidates in a buffer of its own: a vbmc_search_eval after it gives what it gave
    before (csrc/api_cmaes.hip's header states it)."""
    from pyvbmc_amd import active_search

    k, _, _ = host["noisy"]
    s = device_setup(k, ctx)
    kind, y_max, tol_var, u, noise, use_xf = s.args
    r = np.random.default_rng(3)
    X = k.lb + (k.ub - k.lb) * r.random((37, k.D))
    active_search.put_points(ctx, X)
    ev = lambda: active_search.evaluate_resident(ctx, 37, k.D, kind, y_max, tol_var, u, noise, use_xf,  # noqa: E731
                                                 s.state["lb_eps_orig"], s.state["ub_eps_orig"])
    before = ev()
    device_run(SimpleNamespace(**{**vars(k), "max_fevals": 1 + 4 * k.lam}), s, ctx)
    after = ev()
    assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(before[1], after[1])
    assert np.array_equal(bits(before[2]), bits(after[2]))


# ---------------------------------------------------------------------------------------------- 5. refine
def search_and_options(k, s, ctx, **kw):
    from pyvbmc_amd import active_search

    c = k.case
    options = dict(c.options, ns_search=c.number_of_points, search_optimizer="cmaes", search_cmaes_vp_init=True,
                   search_max_fun_evals=1 + 25 * k.lam, **kw)
    state = dict(s.state)
    res = active_search.search(s.acq, s.gp, s.vp, s.flog, state, options, rng="philox", seed=31, ctx=ctx)
    return res, state, options


def test_refine(ctx, host):
    from pyvbmc_amd import active_search

    k, _, bounds = host["b_int"]
    s = device_setup(k, ctx)
    res, state, options = search_and_options(k, s, ctx)
    idx = int(res.order[0])
    f_old = float(res.acq_fast[idx])
    ref = active_search.refine(res, s.acq, s.gp, s.vp, s.flog, state, options, seed=7, ctx=ctx)
    print("refine: f_val_old", f_old, "f_val", ref.f_val, "accepted", ref.accepted, "stats", ref.stats.tolist())
    assert ref.f_val_old == f_old and ref.stats.shape == (1, 4)
    if ref.accepted:
        assert ref.f_val < f_old and np.isnan(ref.idx_cache_acq)
        xo = k.case.pt.inverse(ref.X_acq)[0]
        assert abs(xo[1] - round(xo[1])) < 1e-9
        own = float(np.ravel(s.acq(ref.X_acq.copy(), s.gp, s.vp, s.flog, state))[0])
        assert value_close(ref.f_val, own)
    else:
        assert np.array_equal(bits(ref.X_acq), bits(res.X_acq)) and ref.f_val == f_old
    assert ref.runs[0].f_best <= ref.runs[0].f0 and value_close(ref.runs[0].f0, f_old)
    # three starts from the same seed: run 0 is the single start's run, so the best of three is never worse
    ref3 = active_search.refine(res, s.acq, s.gp, s.vp, s.flog, state, options, n_starts=3, seed=7, ctx=ctx)
    assert ref3.stats.shape == (3, 4) and ref3.f_val <= ref.f_val
    np.testing.assert_array_equal(ref3.stats[0], ref.stats[0])
    # "none" is the identity
    none = active_search.refine(res, s.acq, s.gp, s.vp, s.flog, state, dict(options, search_optimizer="none"), ctx=ctx)
    assert np.array_equal(bits(none.X_acq), bits(res.X_acq)) and none.f_val == f_old and not none.accepted
    # the host route: the same algorithm around the package's batched acquisition call.  Its drift bounds are those of
    # this very run: the statement and its twin driven by the same call.
    hostr = active_search.refine(res, s.acq, s.gp, s.vp, s.flog, state, options, seed=7, device=False, ctx=ctx)
    np.testing.assert_array_equal(hostr.stats, ref.stats)

    def obj(X):
        return np.ravel(s.acq(np.array(X), s.gp, s.vp, s.flog, state))

    def stated(twin):
        es = ch.CMAES(res.X_acq[0], ref.sigma0, ref.lb, ref.ub, max_fevals=options["search_max_fun_evals"], tol_fun=ref.tol_fun,
                      seed=7, twin=twin)
        return ch.run(es, obj, lambda X: sh.real2int(X, k.case.pt, state["integer_vars"]))

    es, tw = stated(None), stated(np.random.default_rng(20261020))
    kb = SimpleNamespace(lb=ref.lb, ub=ref.ub)
    rb = {q: 100.0 * max(v, 4.0 * ch.EPS) for q, v in ch.drift(es, tw, kb).items()}
    assert np.array_equal(es.stats, tw.stats) and np.array_equal(es.stats, hostr.stats[0])
    assert np.array_equal(bits(hostr.runs[0].mean), bits(es.mean)) and hostr.runs[0].sigma == es.sigma  # product == statement
    box = ref.ub - ref.lb
    iv = np.asarray(state["integer_vars"], dtype=bool)
    d, h = ref.runs[0], hostr.runs[0]
    err = {"mean": float(np.max(np.abs(h.mean - d.mean) / box)), "x_best": float(np.max((np.abs(h.x_best - d.x_best) / box)[~iv])),
           "sigma": abs(h.sigma - d.sigma) / d.sigma, "C": float(np.max(np.abs(h.C - d.C)) / np.max(np.abs(d.C)))}
    print("refine host route vs device: error / bound", {q: f"{err[q]:.2e} / {rb[q]:.2e}" for q in err})
    for q in err:
        assert err[q] <= rb[q], (q, err[q], rb[q])
    np.testing.assert_allclose(h.x_best[iv], d.x_best[iv], rtol=1e-12, atol=0)
    assert hostr.accepted == ref.accepted and value_close(hostr.f_val, ref.f_val)


def test_refine_takes_nelder_mead_at_d1(ctx, golden, monkeypatch):
    import scipy.optimize

    from pyvbmc_amd import _lib, acquisition, active_search

    c = sh.load_case(golden("search"), "f")  # D = 1
    assert c.D == 1
    ogp, length, sn2_new = sh.gp_fixture(c, 2)
    gp = PlainGP(ogp)
    gp._ctx = ctx
    vp = sh.package_vp(c, ctx)
    y = c.flog.y[c.flog.X_flag]
    flog = SimpleNamespace(X=c.flog.X, y=c.flog.y, X_flag=c.flog.X_flag, parameter_transformer=c.pt, y_max=float(np.max(y)))
    state = dict(c.optim_state, integer_vars=None, gp_length_scale=length, tol_gp_var=1e-4, variance_regularized_acq_fcn=False,
                 lb_eps_orig=np.full(1, -1e3), ub_eps_orig=np.full(1, 1e3))
    options = dict(c.options, ns_search=c.number_of_points, search_optimizer="cmaes", search_cmaes_vp_init=True,
                   search_max_fun_evals=500 * 3)
    acq = acquisition.AcqFcnLog()
    res = active_search.search(acq, gp, vp, flog, state, options, rng="philox", seed=5, ctx=ctx)
    calls = []
    real = scipy.optimize.minimize

    def spy(fun, x0, **kw):
        calls.append(kw.get("method"))
        return real(fun, x0, **kw)

    monkeypatch.setattr(scipy.optimize, "minimize", spy)
    ref = active_search.refine(res, acq, gp, vp, flog, state, options, ctx=ctx)
    assert calls == ["Nelder-Mead"] and ref.stats is None
    with pytest.raises(_lib.UnsupportedShape):  # the library refuses D = 1 itself
        active_search.cmaes_resident(ctx, 1, 1, flog.y_max, 0.0, 0.0, (None, None, None), 0, state["lb_eps_orig"],
                                     state["ub_eps_orig"], np.zeros((1, 1)), 1.0, [-1.0], [1.0], max_fevals=100, tol_fun=1e-2)
    f_old = float(res.acq_fast[int(res.order[0])])
    assert ref.f_val <= f_old and (ref.accepted == (ref.f_val < f_old))


# ---------------------------------------------------------------------------------------------- 6. refusals
class CountingLib:
    """The library handle with every call counted by name (tests/test_gp_post_gpu.py's pattern)."""

    def __init__(self, lib):
        self._lib_real, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib_real, name)
        if name.startswith("vbmc_") and name != "vbmc_last_error":
            self.calls.append(name)
        return fn


def test_refusals_launch_nothing(ctx, host):
    from pyvbmc_amd import _lib, active_search

    k, _, _ = host["noisy"]
    s = device_setup(k, ctx)
    kind, y_max, tol_var, u, noise, use_xf = s.args
    ctx.set_timing(1)
    ok = device_run(SimpleNamespace(**{**vars(k), "max_fevals": 1 + 2 * k.lam}), s, ctx)
    assert ok.stats[0, 0] == 2 and ctx.last_kernel_ms(_lib.T_SEARCH_CMAES) > 0.0

    def call(**kw):
        a = dict(x0=k.x0, sigma0=k.sigma0, lb=k.lb, ub=k.ub, lam=k.lam, max_fevals=k.max_fevals, noise=noise, kind=kind)
        a.update(kw)
        return active_search.cmaes_resident(ctx, k.D, a["kind"], y_max, tol_var, u, a["noise"], use_xf, s.state["lb_eps_orig"],
                                            s.state["ub_eps_orig"], a["x0"], a["sigma0"], a["lb"], a["ub"], lam=a["lam"],
                                            max_fevals=a["max_fevals"], tol_fun=k.tol_fun, seed=1)

    outside = k.x0.copy()
    outside[0] = k.ub[0] + 1.0
    flipped = k.lb.copy()
    flipped[1] = k.ub[1] + 1.0
    refused = [(ValueError, dict(lam=3)), (ValueError, dict(sigma0=0.0)), (ValueError, dict(sigma0=-1.0)),
               (ValueError, dict(lb=flipped)), (ValueError, dict(x0=outside)), (ValueError, dict(max_fevals=k.lam)),
               (ValueError, dict(noise=(None, None, None))), (ValueError, dict(x0=np.empty((0, k.D)))),
               (_lib.UnsupportedShape, dict(lam=65)), (_lib.UnsupportedShape, dict(kind=9))]
    real = ctx._lib
    try:
        for exc, kw in refused:
            ctx._lib = CountingLib(real)
            with pytest.raises(exc):
                call(**kw)
            assert ctx._lib.calls == ["vbmc_search_cmaes"], kw  # the wrapper made the one call
            ctx._lib = real
            # nothing was launched: the call left no timed interval (the interval opens before the first launch)
            with pytest.raises(ValueError, match="no timed launch"):
                ctx.last_kernel_ms(_lib.T_SEARCH_CMAES)
    finally:
        ctx._lib = real
        ctx.set_timing(0)
    # R lambda above the search set's row cap; D = 1; GP not set
    with pytest.raises(_lib.UnsupportedShape):
        big = np.broadcast_to(k.x0, (16385, k.D))
        call(x0=big, lam=64)
    c2 = _lib.Context(0)
    try:
        opts = _lib.CmaesOpts(0, 100, 1e-2, 0.0, 1)
        z = np.zeros(2)
        rc = c2._lib.vbmc_search_cmaes(c2._h, 1, 0.0, 0.0, 0.0, 0, None, None, None, 0, _lib.ptr(z), _lib.ptr(z), 1, _lib.ptr(z),
                                       _lib.ptr(np.ones(1)), _lib.ptr(z - 1), _lib.ptr(z + 1), 0, C.byref(opts), None, None, None,
                                       None, None, None, None)
        assert rc == _lib.E_ARG  # GP not set
    finally:
        c2.close()
