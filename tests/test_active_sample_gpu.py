"""GPU tests of the active-sampling loop (pyvbmc_amd/active_sample.py): the reference's recorded trajectories
(tests/golden/active_sample.npz) through the device calls, refined runs under Philox seeds, and the loop on a noisy target
with an importance-sampled acquisition.  Shapes are the golden file's: D = 3 (and 2), N = 24 .. 27, S = 2, ns_search = 256,
search_max_fun_evals = 200.

Bounds: the acquired X equal the reference's exactly (a, b) -- the device's acquisition values are correct to ~1e-10 and
the recorded gap between the two best values is >= 0.1 relative -- and to 1e-12 absolute for c, whose cache rows pass the
device transformer; derived scalars to 1e-12; the returned GP's alpha and predict to 1e-9 of their scale against a host
rebuild from its data (the project's predict bound is 1e-10 sf^2 for a well-conditioned GP).
"""
import numpy as np
import pytest

import active_sample_host as ash
from test_active_sample_host import check_trajectory

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
def g(golden):
    return golden("active_sample")


def package_view(gp, ctx):
    """This package's GP around the data and records of a duck (for ``predict``)."""
    from pyvbmc_amd import gp as gpm

    if isinstance(gp, gpm.GP):
        return gp
    v = gpm.GP(gp.D, gpm.SquaredExponential(), gpm.NegativeQuadratic(),
               gpm.GaussianNoise(constant_add=True, user_provided_add=gp.s2 is not None))
    v.ctx, v.X, v.y, v.s2, v.posteriors = ctx, gp.X, gp.y, gp.s2, gp.posteriors
    return v


def check_gp_against_host_rebuild(c, gp, ctx, seed):
    from pyvbmc_amd.gp import upload_gp

    s2 = gp.s2
    ogp = ash.gp_ref.make_gp(gp.X, gp.y, c.hyp, ash.gp_ref.MEAN_NEGQUAD, s2=s2, noise_user=s2 is not None)
    for p, q in zip(gp.posteriors, ogp.posteriors):
        e = np.max(np.abs(np.ravel(p.alpha) - np.ravel(q.alpha))) / np.max(np.abs(q.alpha))
        print(f"alpha rel {e:.2e}")
        assert e <= 1e-9 and np.array_equal(p.hyp, q.hyp)
    r = np.random.default_rng(seed)
    xs = gp.X[r.integers(0, gp.X.shape[0], 32)] + 0.3 * r.standard_normal((32, c.D))
    v = package_view(gp, ctx)
    upload_gp(v, ctx)
    fmu, fs2 = v.predict(xs, separate_samples=True)
    omu, os2 = ash.gp_ref.predict(ogp, xs, separate_samples=True)
    sf2 = float(np.max(np.exp(2 * c.hyp[:, c.D])))
    e_m, e_v = np.max(np.abs(fmu - omu)) / max(np.max(np.abs(omu)), sf2), np.max(np.abs(fs2 - os2)) / sf2
    print(f"predict dmu {e_m:.2e}, ds2 {e_v:.2e}")
    assert e_m <= 1e-9 and e_v <= 1e-9


# ------------------------------------------------------------------------------------------ the recorded trajectories
@pytest.mark.parametrize("duck", ["package", "plain"])
@pytest.mark.parametrize("name", ash.TRAJECTORIES)
def test_trajectory_on_the_device(ctx, g, name, duck):
    from pyvbmc_amd import active_sample
    from pyvbmc_amd.gp import device_posterior, fetch_posteriors

    c = ash.load_case(g, name)
    log = ash.make_logger(c)
    if duck == "package":
        gp = ash.make_gp(c, log, ctx=ctx, device=True, fetch=False)
    else:
        gp = ash.make_plain_gp(c, log)
        assert device_posterior(gp, c.hyp, ctx=ctx, fetch=False)
    vp, st, options = ash.make_vp(c, ctx), ash.make_optim_state(c), ash.make_options(c)
    np.random.seed(c.np_seed)
    flog, st, vp_out, gp_out = active_sample(gp, c.sample_count, st, log, ash.iteration_history(), vp, options, rng="numpy",
                                             fetch=False, ctx=ctx)
    next_rand = np.random.rand()
    assert flog is log and vp_out is vp and gp_out is gp
    check_trajectory(c, log, st, next_rand, x_tol=1e-12 if name == "c" else 0.0)
    assert gp.X.shape[0] == (c.X0.shape[0] + c.sample_count - 1 if name != "c" else int(c.ref.N))
    if duck == "package":  # fetch=False, this package's class: L stays on the device until it is asked for
        assert all(p.L is None for p in gp.posteriors)
        fetch_posteriors(gp, ctx)
    assert all(p.L is not None and p.L.shape == (gp.X.shape[0],) * 2 for p in gp.posteriors)  # (a duck is fetched on return)
    check_gp_against_host_rebuild(c, gp, ctx, seed=len(name))


def test_default_fetch_returns_full_records(ctx, g):
    from pyvbmc_amd import active_sample

    c = ash.load_case(g, "a")
    log = ash.make_logger(c)
    gp = ash.make_gp(c, log, ctx=ctx, device=True, fetch=False)
    vp = ash.make_vp(c, ctx)  # (before the seed: the constructor draws its starting means)
    np.random.seed(c.np_seed)
    out = active_sample(gp, c.sample_count, ash.make_optim_state(c), log, ash.iteration_history(), vp,
                        ash.make_options(c), rng="numpy", ctx=ctx)
    assert all(p.L is not None for p in out[3].posteriors)
    assert np.array_equal(log.X[c.X0.shape[0] : log.Xn + 1], c.ref.X)


# ------------------------------------------------------------------------------------------------------ refined runs
def refined_run(ctx, D, n_starts, seed, acq="AcqFcnLog()", first_only=False):
    """3 points with CMA-ES refinement under Philox seed ``seed``; returns the case, the logger and what ``trace`` saw."""
    from pyvbmc_amd import active_sample
    from pyvbmc_amd.acquisition import string_to_acq

    c = ash.synthetic_case(D)
    log = ash.make_logger(c)
    gp = ash.make_gp(c, log, ctx=ctx, device=True, fetch=False)
    vp, st = ash.make_vp(c, ctx), ash.make_optim_state(c)
    if D == 3:
        st["integer_vars"] = np.array([False, False, True])
    acq_obj = string_to_acq(acq)
    options = ash.make_options(c, search_acq_fcn=[acq_obj], search_optimizer="cmaes", search_max_fun_evals=200)
    seen = []

    def trace(i, res, ref, gp_, vp_, optim_state):
        x = np.array(ref.X_acq, dtype=np.float64)
        f_here = float(acq_obj(x.copy(), gp_, vp_, log, optim_state)[0])
        seen.append(dict(i=i, X=x.copy(), f_val=float(ref.f_val), f_val_old=float(ref.f_val_old), accepted=bool(ref.accepted),
                         lb=np.array(ref.lb), ub=np.array(ref.ub), f_here=f_here, stats=np.array(ref.stats), n_gp=gp_.X.shape[0]))

    np.random.seed(c.np_seed)
    active_sample(gp, 1 if first_only else c.sample_count, st, log, ash.iteration_history(), vp, options, rng="philox",
                  seed=seed, n_starts=n_starts, ctx=ctx, trace=trace)
    return c, log, seen, st


@pytest.mark.parametrize("n_starts", [1, 3])
@pytest.mark.parametrize("D", [2, 3])
def test_refined_run(ctx, D, n_starts):
    c, log, seen, st = refined_run(ctx, D, n_starts, seed=1234)
    assert len(seen) == 3 and [s["n_gp"] for s in seen] == [c.X0.shape[0] + i for i in range(3)]
    for s in seen:
        print(f"D={D} starts={n_starts} point {s['i']}: f_val {s['f_val']:.6g} old {s['f_val_old']:.6g} accepted {s['accepted']} "
              f"here {s['f_here']:.6g} evaluations {s['stats'][:, 1].tolist()}")
        assert np.all(s["X"] >= s["lb"]) and np.all(s["X"] <= s["ub"])  # inside the refine box
        assert not s["accepted"] or s["f_val"] < s["f_val_old"]
        assert s["accepted"] or s["f_val"] == s["f_val_old"]
        assert abs(s["f_here"] - s["f_val"]) <= 1e-9 * abs(s["f_val"])  # the acquisition of that moment at the point
        assert s["stats"].shape == (n_starts, 4) and np.all(s["stats"][:, 1] <= 200)
        if D == 3:
            k = c.pt.inverse(s["X"])[0, 2]
            assert abs(k - np.round(k)) <= 1e-9  # the integer dimension is rounded
    n = c.X0.shape[0]
    assert np.array_equal(log.X[n : n + 3], np.vstack([s["X"] for s in seen])) and np.all(np.isfinite(log.y[n : n + 3]))
    # the same seed again: the same bits
    c2, log2, seen2, st2 = refined_run(ctx, D, n_starts, seed=1234)
    assert np.array_equal(log.X[: n + 3], log2.X[: n + 3]) and np.array_equal(log.y[: n + 3], log2.y[: n + 3])
    assert all(a["f_val"] == b["f_val"] and np.array_equal(a["stats"], b["stats"]) for a, b in zip(seen, seen2))
    assert np.array_equal(st["lb_search"], st2["lb_search"]) and np.array_equal(st["ub_search"], st2["ub_search"])


def test_first_step_is_search_then_refine(ctx):
    """Point 0 of the driver under seed s is ``search(seed=s)`` followed by ``refine(seed=s + 1)``."""
    from pyvbmc_amd import active_search
    from pyvbmc_amd.acquisition import string_to_acq

    s = 77
    c, log, seen, st = refined_run(ctx, 3, 1, seed=s, first_only=True)
    log2 = ash.make_logger(c)
    gp = ash.make_gp(c, log2, ctx=ctx, device=True, fetch=False)
    vp, st2 = ash.make_vp(c, ctx), ash.make_optim_state(c)
    st2["integer_vars"] = np.array([False, False, True])
    acq = string_to_acq("AcqFcnLog()")
    options = ash.make_options(c, search_acq_fcn=[acq], search_optimizer="cmaes", search_max_fun_evals=200)
    res = active_search.search(acq, gp, vp, log2, st2, options, rng="philox", seed=s, ctx=ctx)
    ref = active_search.refine(res, acq, gp, vp, log2, st2, options, n_starts=1, seed=s + 1, ctx=ctx)
    assert np.array_equal(np.ravel(ref.X_acq), np.ravel(seen[0]["X"])) and float(ref.f_val) == seen[0]["f_val"]
    assert np.array_equal(log.X[c.X0.shape[0]], np.ravel(ref.X_acq))


# ------------------------------------------------------------------------------------- noisy target, importance sampling
def test_viqr_on_the_noisy_target(ctx):
    from pyvbmc_amd import active_sample

    c = ash.synthetic_case(3, noisy=True)
    log = ash.make_logger(c)
    gp = ash.make_gp(c, log, ctx=ctx, device=True, fetch=False)
    vp, st = ash.make_vp(c, ctx), ash.make_optim_state(c)
    options = ash.make_options(c, search_acq_fcn=["AcqFcnVIQR()"], active_importance_sampling_mcmc_samples=60)
    states, rows = [], []

    def trace(i, res, ref, gp_, vp_, optim_state):
        states.append(optim_state.get("active_importance_sampling"))
        rows.append((gp_.X.shape[0], None if gp_.s2 is None else gp_.s2.shape[0]))

    np.random.seed(c.np_seed)
    real, names = ctx._lib, []
    ctx._lib = type("CallLog", (), {"__getattr__": lambda self, k: (names.append(k), getattr(real, k))[1]})()
    try:
        flog, st, vp, gp = active_sample(gp, c.sample_count, st, log, ash.iteration_history(), vp, options, rng="philox",
                                         seed=5, ctx=ctx, trace=trace)
    finally:
        ctx._lib = real
    n = c.X0.shape[0]
    # every update went to the noisy append; where the new point's noise is below the sample's minimum it refuses and
    # the posterior is rebuilt, so between them the two entries were called once per update
    assert names.count("vbmc_gp_append_noisy") == 2 and "vbmc_gp_append" not in names
    print("noisy appends refused and rebuilt:", names.count("vbmc_gp_posterior"))
    assert len(states) == 3 and all(s is not None for s in states) and len({id(s) for s in states}) == 3
    assert rows == [(n + i, n + i) for i in range(3)]  # gp.s2 grows by a row per point
    assert log.Xn + 1 == n + 3 and np.all(np.isfinite(log.y[: n + 3])) and np.all(log.S[n : n + 3] > 0)
    assert np.all(np.isfinite(log.X[: n + 3])) and all(np.all(np.isfinite(p.alpha)) for p in gp.posteriors)
    assert np.array_equal(np.ravel(gp.s2), np.ravel(log.S[: n + 2] ** 2))
    check_gp_against_host_rebuild(c, gp, ctx, seed=9)
