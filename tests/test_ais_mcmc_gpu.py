"""GPU tests of the device MCMC step of ``active_importance_sampling`` (``vbmc_is_mcmc``, csrc/acq_is_mcmc.hip, selected
by ``sampler="device"``) against tests/slice_host.py, the same sampler in NumPy, over ``gp_ref.predict``.

The replay cases keep a margin |f - ly| >= 1e-6 at every comparison and hit no cap (asserted on the CPU,
tests/test_slice_host.py), so the device chain takes the host's decisions and the two can be compared point by point:
counters exactly, X at 1e-12 of the box (a kept coordinate is a few additions of box-sized numbers; at most 72 updates
per coordinate), f_mu / f_s2 at the project's predict bounds (1e-10 max(1, |f_mu|), 1e-10 sf^2) and log_p at those two
bounds carried through f = [f_mu] + u f_s + log1p(-exp(-2 u f_s)), f_s = sqrt(f_s2 + noise):
|d log_p| <= [d f_mu] + u coth(u f_s) / (2 f_s) d f_s2, evaluated at the host's values.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import ais_host
import ais_mcmc_cases as cases
import slice_host
from helpers import PlainGP, PlainVP
from test_ais_gpu import CTMP_REL_MEASURED, CountingLib, check_state, mirror_acq, nearest_sn2, optim_state, plain_gp
from test_ais_host import sf2_max

pytestmark = pytest.mark.gpu

E2E_SEED = 5  # the chains' key of the end-to-end case: host margin 1.0e-5, no cap (asserted below)


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


@pytest.fixture(scope="module")
def larger():
    return ais_host.larger_case()


def device_chains(ctx, ogp, kind, seed, x0, widths, lb, ub, u_q=ais_host.U75):
    """``vbmc_is_mcmc`` on the GP ``ogp``: (X, log_p, f_mu, f_s2, stats, invalid)."""
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gp import upload_gp

    upload_gp(PlainGP(ogp), ctx)
    S, D, n = len(ogp.posteriors), ogp.D, cases.N_KEEP
    X, lp = np.full((S, n, D), np.nan), np.full((S, n), np.nan)
    mu, s2 = np.full((n, S), np.nan), np.full((n, S), np.nan)
    stats, invalid = np.zeros((S, 4), dtype=np.int64), C.c_int(-1)
    ctx.check(ctx._lib.vbmc_is_mcmc(ctx._h, int(kind == ais_host.IMIQR), float(u_q), _lib.ptr(_lib.f64(x0)),
                                    _lib.ptr(_lib.f64(widths)), _lib.ptr(_lib.f64(lb)), _lib.ptr(_lib.f64(ub)), n, cases.THIN,
                                    cases.BURN, C.c_uint64(seed), _lib.ptr(X), _lib.ptr(lp), _lib.ptr(mu), _lib.ptr(s2),
                                    stats.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(invalid)))
    return X, lp, mu, s2, stats, invalid.value


# ------------------------------------------------------------------------------------------------ 1. replay
@pytest.mark.parametrize("name,kind", cases.CASES)
def test_replay_vs_slice_host(ctx, name, kind):
    ogp, _ = cases.gp_of(name)
    with np.errstate(all="ignore"):
        chains, h_mu, h_s2 = cases.host_replay(name, kind)
    x0, widths, lb, ub = cases.chain_args(ogp)
    X, lp, mu, s2, stats, invalid = device_chains(ctx, ogp, kind, cases.SEEDS[(name, kind)], x0, widths, lb, ub)
    assert invalid == 0
    sf2, u = sf2_max(ogp), ais_host.U75
    worst = dict(x=0.0, mu=0.0, s2=0.0, lp=0.0)
    for s, c in enumerate(chains):
        assert stats[s].tolist() == c["stats"].tolist(), f"chain {s}: counters {stats[s]} != host {c['stats']}"
        e_x = np.max(np.abs(X[s] - c["samples"]) / (ub - lb))
        e_mu = np.max(np.abs(mu[:, s] - h_mu[:, s]) / np.maximum(1.0, np.abs(h_mu[:, s])))
        e_s2 = np.max(np.abs(s2[:, s] - h_s2[:, s])) / sf2
        # log_p's bound from the two predict bounds, at the host's values
        post = ogp.posteriors[s]
        noise = np.exp(2 * post.hyp[ogp.D + 1]) * post.sn2_mult
        f_s = np.sqrt(h_s2[:, s] + noise)
        bound = (1e-10 * np.maximum(1.0, np.abs(h_mu[:, s])) if kind == ais_host.IMIQR else 0.0) \
            + u / np.tanh(u * f_s) / (2 * f_s) * 1e-10 * sf2
        e_lp = np.max(np.abs(lp[s] - c["f_vals"]) / bound)
        worst = dict(x=max(worst["x"], e_x), mu=max(worst["mu"], e_mu), s2=max(worst["s2"], e_s2), lp=max(worst["lp"], e_lp))
        assert e_x <= 1e-12 and e_mu <= 1e-10 and e_s2 <= 1e-10 and e_lp <= 1.0, (s, e_x, e_mu, e_s2, e_lp)
    print(f"replay {name} {kind}: evaluations {stats[:, 0].tolist()}, draws {stats[:, 1].tolist()}; X {worst['x']:.2e} of the "
          f"box, f_mu {worst['mu']:.2e} max(1, |f_mu|), f_s2 {worst['s2']:.2e} sf2, log_p {worst['lp']:.2e} of its bound")


def test_workgroup_sizes_agree(ctx):
    """The three workgroup sizes split the rows of a column differently (1, 2 or 4 stripes at N = 150), so their sums
    differ in rounding only: same decisions, same counters, same points."""
    name, kind = "larger", ais_host.IMIQR
    ogp, _ = cases.gp_of(name)
    x0, widths, lb, ub = cases.chain_args(ogp)
    outs = []
    try:
        for nt in (256, 512, 768):
            ctx.check(ctx._lib.vbmc_set_option(ctx._h, b"is_mcmc_threads", nt))
            outs.append(device_chains(ctx, ogp, kind, cases.SEEDS[(name, kind)], x0, widths, lb, ub))
    finally:
        ctx.check(ctx._lib.vbmc_set_option(ctx._h, b"is_mcmc_threads", 512))
    for o in outs[1:]:
        assert np.array_equal(o[4], outs[0][4])
        assert np.max(np.abs(o[0] - outs[0][0]) / (ub - lb)) <= 1e-12
        assert np.max(np.abs(o[1] - outs[0][1])) <= 1e-9


# ------------------------------------------------------------------------------------------------ 2. end to end
def e2e_opts():
    return ais_host.Opts(active_importance_sampling_vp_samples=30, active_importance_sampling_box_samples=18,
                         active_importance_sampling_mcmc_samples=24, active_importance_sampling_mcmc_thin=2)


def test_imiqr_end_to_end_vs_host(ctx, larger):
    from pyvbmc_amd.acquisition import _is_state_key
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    ogp, mix, Xs, sn2_new = larger
    gp, length = plain_gp(ogp, sn2_new)
    vp, acq = PlainVP(mix), mirror_acq(ais_host.IMIQR)
    cls = slice_host.sampler_class(E2E_SEED)
    np.random.seed(7)
    with np.errstate(all="ignore"):
        host = ais_host.ais(mix, ogp, ais_host.IMIQR, e2e_opts(), sampler=cls)
    assert min(r["margin"] for r in cls.results) >= 1e-6 and not any(r["stats"][2:].any() for r in cls.results)
    np.random.seed(7)
    out = active_importance_sampling(vp, gp, acq, e2e_opts(), sampler="device", seed=E2E_SEED)
    assert out["X"].shape == (3, 24, 4) and "mcmc_stats" not in out
    diam = ogp.X.max(0) - ogp.X.min(0)
    e_x = float(np.max(np.abs(out["X"] - host["X"]) / (2 * diam)))
    print(f"end to end: X {e_x:.2e} of the box")
    assert e_x <= 1e-12
    with np.errstate(all="ignore"):
        host["K_Xa_X"], host["C_tmp"] = ais_host.products(ogp, out["X"])  # (C_tmp entry by entry: at the device's points)
    assert check_state(out, host, ogp, "end to end imiqr, device chains") <= 10 * CTMP_REL_MEASURED
    # the call left the state installed: the acquisition uploads nothing
    assert ctx.__dict__["_acq_is_key"] == _is_state_key(out, ctx)[0]
    counting = CountingLib(ctx._lib)
    ctx._lib = counting
    try:
        v = acq(Xs.copy(), gp, vp, SimpleNamespace(y_max=0.0), optim_state(ogp.X, length, out))
    finally:
        ctx._lib = counting._lib_real
    assert counting.n_set == 0 and counting.n_build == 0
    sn2 = nearest_sn2(Xs, ogp.X, length, sn2_new)
    with np.errstate(all="ignore"):
        ref = ais_host.quantile_acq(ogp, Xs, sn2, host, ais_host.IMIQR)
    err = float(np.max(np.abs(v - ref)))
    print(f"acq at 200 points: max |device - host| = {err:.2e}")
    assert err <= 1e-9


def test_env_switch_and_host_loop_with_the_same_sampler(ctx, larger, monkeypatch):
    """``VBMC_HIP_AIS_SAMPLER=device`` selects the launch when ``sampler`` is None; the mirror's host loop handed
    ``slice_host.sampler_class`` (the same algorithm, device ``predict`` per evaluation) reaches the same points."""
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    ogp, mix, _, sn2_new = larger
    gp, _ = plain_gp(ogp, sn2_new)
    vp, acq = PlainVP(mix), mirror_acq(ais_host.IMIQR)
    np.random.seed(7)
    a = active_importance_sampling(vp, gp, acq, e2e_opts(), sampler="device", seed=E2E_SEED, products=False)
    monkeypatch.setenv("VBMC_HIP_AIS_SAMPLER", "device")
    np.random.seed(7)
    b = active_importance_sampling(vp, gp, acq, e2e_opts(), seed=E2E_SEED, products=False)
    assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["ln_weights"], b["ln_weights"])
    monkeypatch.delenv("VBMC_HIP_AIS_SAMPLER")
    np.random.seed(7)
    c = active_importance_sampling(vp, gp, acq, e2e_opts(), sampler=slice_host.sampler_class(E2E_SEED), products=False)
    diam = ogp.X.max(0) - ogp.X.min(0)
    assert np.max(np.abs(a["X"] - c["X"]) / (2 * diam)) <= 1e-12
    assert np.max(np.abs(a["ln_weights"] - c["ln_weights"])) <= 1e-9


# ------------------------------------------------------------------------------------------------ 3. reproducibility
def test_same_seed_is_bit_identical_and_another_seed_is_not(ctx, larger):
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    ogp, mix, _, sn2_new = larger
    gp, _ = plain_gp(ogp, sn2_new)
    vp, acq = PlainVP(mix), mirror_acq(ais_host.IMIQR)
    runs = []
    for seed in (E2E_SEED, E2E_SEED, E2E_SEED + 1):
        np.random.seed(7)
        runs.append(active_importance_sampling(vp, gp, acq, e2e_opts(), sampler="device", seed=seed))
    for k in ("X", "f_s2", "ln_weights", "K_Xa_X", "C_tmp"):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    assert not np.array_equal(runs[0]["X"], runs[2]["X"])
    assert np.all(np.isfinite(runs[2]["X"])) and np.all(np.isfinite(runs[2]["ln_weights"]))


# ------------------------------------------------------------------------------------------------ 4. errors
def test_step0_refuses_the_device_sampler_before_any_draw(ctx, larger):
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    ogp, mix, _, sn2_new = larger
    gp, _ = plain_gp(ogp, sn2_new)
    vp, acq = PlainVP(mix), mirror_acq(ais_host.VIQR)
    acq.acq_info["mcmc_importance_sampling"] = True
    opts = ais_host.Opts(active_importance_sampling_mcmc_samples=40, active_importance_sampling_mcmc_thin=2,
                         active_importance_sampling_fess_thresh=1.5)
    np.random.seed(13)
    state = np.random.get_state()
    with pytest.raises(NotImplementedError, match="step 0"):
        active_importance_sampling(vp, gp, acq, opts, sampler="device")
    after = np.random.get_state()
    assert np.array_equal(after[1], state[1]) and after[2:] == state[2:]


def test_nonfinite_start_is_invalid_and_leaves_the_state(ctx, larger):
    """A chain whose target is not finite at its start: the launch flags it and writes nothing for it, the mirror raises
    the reference's ValueError and the importance state installed before stays installed and unchanged."""
    from pyvbmc_amd.acquisition import AcqFcnIMIQR
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    ogp, mix, Xs, sn2_new = larger
    gp, length = plain_gp(ogp, sn2_new)
    vp, acq = PlainVP(mix), mirror_acq(ais_host.IMIQR)
    np.random.seed(7)
    good = active_importance_sampling(vp, gp, acq, e2e_opts(), sampler="device", seed=E2E_SEED, products=False)
    flog, ostate = SimpleNamespace(y_max=0.0), optim_state(ogp.X, length, good)
    v0 = acq(Xs.copy(), gp, vp, flog, ostate)
    key = ctx.__dict__["_acq_is_key"]

    class NanQuantile(AcqFcnIMIQR):
        """Finite resampling weights (host side), but the quantile factor the chains receive is NaN."""

        def is_log_added(self, **kwargs):
            f_s = np.sqrt(kwargs["f_s2"])
            return ais_host.U75 * f_s + np.log1p(-np.exp(-2 * ais_host.U75 * f_s))

    bad = NanQuantile()
    bad.u = float("nan")
    np.random.seed(7)
    with pytest.raises(ValueError, match="Invalid value."):
        active_importance_sampling(vp, gp, bad, e2e_opts(), sampler="device", seed=E2E_SEED, products=False)
    assert ctx.__dict__["_acq_is_key"] == key
    counting = CountingLib(ctx._lib)
    ctx._lib = counting
    try:
        v1 = acq(Xs.copy(), gp, vp, flog, ostate)
    finally:
        ctx._lib = counting._lib_real
    assert counting.n_set == 0 and counting.n_build == 0 and np.array_equal(v0, v1)
    # the entry point itself: the flag, and nothing written for the chains
    x0, widths, lb, ub = cases.chain_args(ogp)
    X, lp, mu, s2, stats, invalid = device_chains(ctx, ogp, ais_host.IMIQR, 1, x0, widths, lb, ub, u_q=float("nan"))
    assert invalid == 1 and not X.any() and not lp.any() and not mu.any() and not s2.any()
    assert stats[:, 0].tolist() == [1, 1, 1] and not stats[:, 1:].any()


def test_unsupported_shapes_are_refused_before_the_launch(ctx):
    from pyvbmc_amd import _lib
    from oracle import gp_ref

    rng = np.random.default_rng(2)
    D, N = 33, 40
    X = rng.standard_normal((N, D))
    y = -0.5 * np.sum(X**2, axis=1, keepdims=True)
    hyp = np.concatenate([np.zeros(D), [0.5], [np.log(0.1)], [0.0], np.zeros(D), np.zeros(D)])
    ogp = gp_ref.make_gp(X, y, hyp, gp_ref.MEAN_NEGQUAD)
    with pytest.raises(_lib.UnsupportedShape):
        device_chains(ctx, ogp, ais_host.IMIQR, 1, X[:1], np.ones(D), X.min(0) - 1, X.max(0) + 1)
