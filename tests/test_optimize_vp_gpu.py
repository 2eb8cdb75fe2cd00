"""``optimize_vp``'s last stage on the device (pyvbmc_amd/optimize_vp.py, csrc/elcbo_full.hip, csrc/api_elcbo_full.hip)
against the NumPy statement tests/optimize_vp_host.py and the reference's recorded run (tests/golden/optimize_vp.npz).

Bounds.
  The re-weighting kernel alone: a sum of n terms evaluated in float64 in any order, each term a product of at most
  three factors, is within (n + 2) eps sum|term| of the exact sum to first order; the kernel and the statement are both
  such evaluations, so they differ by at most F (n + 2) eps sum|term| with F = 2, and F = 4 is asserted: what is left
  covers second-order terms and the weights of a trial, which the library forms in C++ and the statement in NumPy
  (the same statements; ``log`` / ``exp`` may differ by an ulp).  The statistics over the GP samples propagate the
  per-sample bounds (``stat_bounds``).  Derivation and the measured ratio: profiles/optimize_vp.md.
  G, varG, varF, var_ss, I_sk against the reference: 1e-10 relative, the project's GP parity figure (a recorded 0 --
  var_ss at S = 1 -- has to be met within 1e-10 sf^2).  J_sjk: 1e-10 of its largest entry, and every entry within
  1e-10 sf^2, the scale that figure is stated on for the variance terms (tests/test_gpu_parity.py):
  J_jk = sf^2 [exp(..) - z_j' K^-1 z_k] is a difference of O(sf^2) quantities, so a small entry's error floor is eps sf^2
  and not eps |J_jk|; sf^2 is the largest signal variance of the GP samples.  H and nelbo on the reference's own draws:
  the project's 1e-6 max(1, |.|).
  Choices, decisions, ``pruned``, shapes, NumPy's state: exactly.
"""
import ctypes as C
import importlib

import numpy as np
import optimize_vp_host as oh
import pytest
from helpers import PlainGP

from oracle import gp_ref

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
F_BOUND = 4.0
REL_GP, REL_MC = 1e-10, 1e-6


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
    return np.load(oh.GOLDEN, allow_pickle=False)


def names():
    return oh.case_names(np.load(oh.GOLDEN, allow_pickle=False))


def ov():
    return importlib.import_module("pyvbmc_amd.optimize_vp")


def package_vp(c, ctx, K=None):
    from pyvbmc_amd import VariationalPosterior

    D = int(c["shape"][0])
    K0 = int(c["shape"][1])
    vp = VariationalPosterior(D, K0)
    for a in oh.ATTRS:
        setattr(vp, a, np.array(c["base_" + a]))
    vp.optimize_mu, vp.optimize_sigma, vp.optimize_lambd, vp.optimize_weights = (bool(f) for f in c["flags"])
    vp.ctx = ctx
    return vp


def case_gp(c, ctx):
    gp = PlainGP(gp_ref.make_gp(c["X"], c["y"], c["hyp"], gp_ref.MEAN_NEGQUAD))
    gp._ctx = ctx
    return gp


def set_state(c, e):
    np.random.set_state(("MT19937", c["eval_mt_key"][e], int(c["eval_mt_pos"][e]), int(c["eval_mt_has_gauss"][e]),
                         float(c["eval_mt_gauss"][e])))


def state_is_final(c):
    st = np.random.get_state(legacy=True)
    return (np.array_equal(st[1], c["mt_key"]) and st[2] == int(c["mt_pos"]) and st[3] == int(c["mt_has_gauss"])
            and (st[3] == 0 or st[4] == float(c["mt_gauss"])))


def close(got, want, tol, floor=0.0):
    return abs(got - want) <= tol * max(floor, abs(want))


def close_var(got, want, sf2):
    """1e-10 relative; a recorded 0 within 1e-10 sf^2 (module docstring)."""
    return abs(got - want) <= (REL_GP * abs(want) if want != 0 else REL_GP * sf2)


def sf2_of(c):
    return float(np.max(np.exp(2 * c["hyp"][:, int(c["shape"][0])])))


# ---- the kernel alone, through vbmc_elcbo_put ----------------------------------------------------------------------------

def stat_bounds(t, S, has_var):
    """Bounds on |G|, |varG|, |var_ss| errors at F = 1 from the per-sample term sums (module docstring)."""
    bG = (t["nG"] + 2) * EPS * t["absG"]
    bV = (t["nV"] + 2) * EPS * np.maximum(t["absV"], oh.TINY)
    if S == 1:
        return bG[0], bV[0] if has_var else 0.0, 0.0
    G, v = t["G_s"], t["vG_s"]
    d = np.abs(G - G.mean())
    b_mean = bG.mean() + (S + 2) * EPS * np.abs(G).mean()
    dd = 2 * bG.max()
    b_vss = np.sum(2 * d * dd + dd**2) / (S - 1) + (S + 4) * EPS * np.sum(d**2) / (S - 1)
    b_std = 2 * bV.max() * np.sqrt(S / (S - 1)) + (S + 6) * EPS * np.std(v, ddof=1)
    b_varG = bV.mean() + b_vss + (S + 3) * EPS * (v.mean() + np.sum(d**2) / (S - 1))
    if not has_var:
        return b_mean, 0.0, 0.0
    return b_mean, b_varG, b_vss + b_std + 2 * EPS * (np.sum(d**2) / (S - 1) + np.std(v, ddof=1))


def put_record(ctx, D, K0, S, I, J, rng):
    """A random K0-component mixture as the context's, then the record; returns the mixture as the statement's dict."""
    lam = 0.5 + rng.random((D, 1))
    w = rng.dirichlet(np.ones(K0)).reshape(1, -1)
    m = {"mu": rng.standard_normal((D, K0)), "sigma": 0.3 + rng.random((1, K0)), "lambd": lam / np.sqrt(np.sum(lam**2) / D),
         "w": w, "eta": np.log(w) - np.max(np.log(w))}
    ctx.set_mixture(m["mu"], m["sigma"], m["lambd"], m["w"], m["eta"])
    ctx.mixture_changed(D, K0)
    from pyvbmc_amd import _lib

    ctx.check(ctx._lib.vbmc_elcbo_put(ctx._h, S, K0, _lib.ptr(_lib.f64(I)), _lib.ptr(None if J is None else _lib.f64(J))))
    return m


def trial(ctx, drop, ns=2, seed=1):
    from pyvbmc_amd import _lib

    out = np.empty(7)
    ctx.check(ctx._lib.vbmc_elcbo_prune_trial(ctx._h, drop, ns, _lib.EPS_PHILOX, C.c_uint64(seed), _lib.ptr(out)))
    return out


def info(ctx):
    v = (C.c_int64 * 5)()
    alive = np.zeros(128, dtype=np.int32)
    ctx.check(ctx._lib.vbmc_elcbo_record_info(ctx._h, v, alive.ctypes.data_as(C.POINTER(C.c_int32))))
    return [int(x) for x in v], alive[: int(v[2])].copy()


def check_out(out, I, J, alive, w, S, what, worst):
    G, varG, var_ss, t = oh.reweight(I, J, alive, w, terms=True)
    bG, bV, bS = stat_bounds(t, S, J is not None)
    errs = (abs(out[1] - G), abs(out[4] - varG), abs(out[6] - var_ss))
    for e, b, name in zip(errs, (bG, bV, bS), ("G", "varG", "var_ss")):
        ratio = e / b if b > 0 else (0.0 if e == 0 else np.inf)
        worst[0] = max(worst[0], ratio)
        assert ratio <= F_BOUND, (what, name, e, b)
    assert out[0] == -out[1] - out[2] and out[3] == out[4] and out[5] == 0.0  # nelbo, varF, varH (:1179-1183)


@pytest.mark.parametrize("S", [1, 2, 8])
@pytest.mark.parametrize("K0", [1, 2, 5, 63, 64, 65, 128])
def test_reweighting_kernel_on_chosen_records(ctx, K0, S):
    D = 2
    r = np.random.default_rng(1000 * K0 + S)
    I = -5.0 + 3.0 * r.standard_normal((S, K0))
    A = r.standard_normal((S, K0, K0))
    J = 0.05 * (A @ np.transpose(A, (0, 2, 1))) / K0 + 0.01 * r.standard_normal((S, K0, K0))  # (read on the upper triangle only)
    worst = [0.0]
    # drop the first, the last and a middle component, one after the other, each accepted
    m = put_record(ctx, D, K0, S, I, J, r)
    alive = list(range(K0))
    check_out(trial(ctx, -1), I, J, alive, m["w"], S, (K0, S, "all"), worst)
    w0 = info(ctx)[0][4]
    trial(ctx, -1)  # (a repeat: no buffer grows any more)
    assert info(ctx)[0][:3] == [S, K0, K0] and info(ctx)[0][4] - w0 == 1  # ONE stream wait per trial
    for pick in ("first", "last", "middle"):
        if len(alive) < 2:
            break
        pos = {"first": 0, "last": len(alive) - 1, "middle": len(alive) // 2}[pick]
        m, _ = oh.prune_mixture(m, pos)
        alive = alive[:pos] + alive[pos + 1 :]
        out = trial(ctx, pos)
        check_out(out, I, J, alive, m["w"], S, (K0, S, pick), worst)
        before = info(ctx)
        assert before[0][2] == len(alive) + 1  # a trial alone changes nothing
        ctx.check(ctx._lib.vbmc_elcbo_prune_accept(ctx._h))
        got, al = info(ctx)
        assert got[2] == len(alive) and np.array_equal(al, alive) and got[3] == 0
    # all but one: go on dropping the first until one component is left
    while len(alive) > 1:
        m, _ = oh.prune_mixture(m, 0)
        alive = alive[1:]
        out = trial(ctx, 0)
        ctx.check(ctx._lib.vbmc_elcbo_prune_accept(ctx._h))
    if K0 > 1:
        check_out(out, I, J, alive, m["w"], S, (K0, S, "one left"), worst)
        assert np.allclose(m["w"], 1.0)
    # both clamps: non-positive diagonal entries; a total below tiny
    Jd = J.copy()
    k = np.arange(K0)
    Jd[:, k[::2], k[::2]] = -np.abs(Jd[:, k[::2], k[::2]])
    m = put_record(ctx, D, K0, S, I, Jd, r)
    check_out(trial(ctx, -1), I, Jd, list(range(K0)), m["w"], S, (K0, S, "diagonal clamp"), worst)
    Jn = -np.ones((S, K0, K0))
    m = put_record(ctx, D, K0, S, I, Jn, r)
    out = trial(ctx, -1)
    check_out(out, I, Jn, list(range(K0)), m["w"], S, (K0, S, "total clamp"), worst)
    if K0 > 1:  # (K0 = 1: the diagonal clamp leaves w^2 tiny = tiny)
        G_s = oh.reweight(I, Jn, range(K0), m["w"], terms=True)[3]["G_s"]
        assert np.all(oh.reweight(I, Jn, range(K0), m["w"], terms=True)[3]["vG_s"] == oh.TINY)
        if S == 1:
            assert out[4] == oh.TINY
        else:
            assert abs(out[4] - (oh.TINY + np.var(G_s, ddof=1))) <= 1e-13 * max(1.0, out[4])
    # without variance (skip_elbo_variance)
    m = put_record(ctx, D, K0, S, I, None, r)
    out = trial(ctx, -1)
    check_out(out, I, None, list(range(K0)), m["w"], S, (K0, S, "no variance"), worst)
    assert out[4] == 0.0 and out[6] == 0.0
    print(f"K0={K0} S={S}: worst error / bound at F=1: {worst[0]:.3f} (asserted <= {F_BOUND})")


def test_entries_refuse_what_they_do_not_cover(ctx):
    from pyvbmc_amd import _lib

    r = np.random.default_rng(3)
    put_record(ctx, 2, 3, 2, r.standard_normal((2, 3)), None, r)
    with pytest.raises(ValueError):
        trial(ctx, 3)
    with pytest.raises(ValueError):
        trial(ctx, 0, ns=3)
    with pytest.raises(ValueError):  # no trial to accept
        ctx.check(ctx._lib.vbmc_elcbo_prune_accept(ctx._h))
    I = r.standard_normal((1, 4))
    with pytest.raises(ValueError):  # the context's mixture has 3 components, not 4
        ctx.check(ctx._lib.vbmc_elcbo_put(ctx._h, 1, 4, _lib.ptr(I), None))


# ---- vbmc_elcbo_full at the fixture's thetas -------------------------------------------------------------------------------

def full_at(c, ctx, e, device=True, stage=None):
    o = ov()
    ev = oh.eval_of(c, e)
    K = ev["K"]
    vp = package_vp(c, ctx)
    if K != vp.K:  # a trial's evaluation: a posterior of K components (every block is optimised: theta sets them all)
        from pyvbmc_amd import VariationalPosterior

        vp = VariationalPosterior(vp.D, K)
        vp.ctx = ctx
    gp = case_gp(c, ctx)
    stage = stage or o._Stage(ctx, gp, oh.options_of(c), "numpy", o._Seeds(None), device)
    set_state(c, e)
    theta = ev["theta"].copy()
    out, I, J = stage.full(ev["slot"], theta, vp)
    return ev, out, I, J, theta


@pytest.mark.parametrize("name", names())
def test_full_evaluation_matches_the_reference_and_the_composed_route(z, ctx, name):
    c = oh.load_case(z, name)
    worst = {"gp": 0.0, "mc": 0.0, "var": 0.0, "var_rel": 0.0}
    sf2 = sf2_of(c)
    for e in range(int(c["n_evals"])):
        ev, out, I, J, theta = full_at(c, ctx, e)
        _, out_c, I_c, J_c, _ = full_at(c, ctx, e, device=False)
        got = dict(zip(("nelbo", "G", "H", "varF", "varG", "varH", "var_ss"), out))
        comp = dict(zip(("nelbo", "G", "H", "varF", "varG", "varH", "var_ss"), out_c))
        for ref, ref_I, ref_J, tag in ((ev, ev["I_sk"], ev["J_sjk"], "reference"), (comp, I_c, J_c, "composed")):
            worst["gp"] = max(worst["gp"], abs(got["G"] - ref["G"]) / abs(ref["G"]))
            assert close(got["G"], ref["G"], REL_GP), (tag, e, got["G"], ref["G"])
            for k in ("varG", "varF", "var_ss"):
                worst["var"] = max(worst["var"], abs(got[k] - ref[k]) / sf2)
                if ref[k] != 0:
                    worst["var_rel"] = max(worst["var_rel"], abs(got[k] - ref[k]) / abs(ref[k]))
                assert close_var(got[k], ref[k], sf2), (tag, e, k, got[k], ref[k])
            for k in ("H", "nelbo"):
                worst["mc"] = max(worst["mc"], abs(got[k] - ref[k]) / max(1.0, abs(ref[k])))
                assert close(got[k], ref[k], REL_MC, 1.0), (tag, e, k, got[k], ref[k])
            assert np.all(np.abs(I - ref_I) <= REL_GP * np.abs(ref_I)), (tag, e)
            assert np.max(np.abs(J - ref_J)) <= REL_GP * min(sf2, np.max(np.abs(ref_J))), (tag, e)
        assert got["varH"] == 0.0 and np.array_equal(theta, ev["theta"])
    print(f"{name}: {int(c['n_evals'])} evaluations, worst G error {worst['gp']:.2e} (bound {REL_GP:.0e}), worst variance "
          f"error {worst['var']:.2e} sf^2 (bound {REL_GP:.0e}; {worst['var_rel']:.2e} of the value), "
          f"worst H / nelbo error {worst['mc']:.2e} max(1, |.|) (bound {REL_MC:.0e})")


def test_full_evaluation_without_variance(z, ctx):
    c = oh.load_case(z, "d2k6n20s3_reject")
    o = ov()
    opts = oh.options_of(c)
    opts["skip_elbo_variance"] = True
    stage = o._Stage(ctx, case_gp(c, ctx), opts, "numpy", o._Seeds(None), True)
    ev, out, I, J, _ = full_at(c, ctx, 0, stage=stage)
    assert J is None and out[3] == out[4] == out[6] == 0.0 and close(out[1], ev["G"], REL_GP)
    assert np.all(np.abs(I - ev["I_sk"]) <= REL_GP * np.abs(ev["I_sk"]))


# ---- the last stage from the recorded iterates ---------------------------------------------------------------------------------

def last_stage(c, ctx, device):
    """Every slow start's full evaluations at the recorded ``theta_opt`` / midpoint, then selection, pruning and stats, on
    the reference's stream: returns optimize_vp's triple, the trials seen and the record info after each."""
    o = ov()
    D, K, N, S, fast_N, slow_N = (int(v) for v in c["shape"])
    opts = oh.options_of(c)
    vp, gp = package_vp(c, ctx), case_gp(c, ctx)
    stage = o._Stage(ctx, gp, opts, "numpy", o._Seeds(None), device)
    stats = o._initialize_full_elcbo(2 * slow_N, int(c["eval_ntheta"][0]), K, S)
    slots = {}
    n_start = int(c["n_start_evals"])
    ns_ent_K = int(c["ns_ent_K"])
    for i in range(slow_N):
        es = [e for e in range(n_start) if int(c["eval_slot"][e]) // 2 == i]
        vp0 = package_vp(c, ctx)  # (before the state is set: the constructor draws its initial means)
        set_state(c, es[0])
        th = {int(c["eval_slot"][e]) % 2: np.array(c["eval_theta"][e]) for e in es}
        o.optimize_one(opts, {"warmup": False, "entropy_switch": False}, vp, gp, vp0, ns_ent_K, None, stats, i, stage,
                       theta_opt=th[1], theta_mid=th.get(0), slots=slots)
    seen, infos = [], []

    def on_trial(t):
        seen.append(t)
        if device:
            infos.append(stage.record_info())

    out = o.finish(opts, slots, stats, K, stage, choose=lambda n: int(np.random.randint(0, n)), on_trial=on_trial)
    return out, seen, infos, stats


def check_last_stage(c, out, seen, stats):
    vp, var_ss, pruned = out
    sf2 = sf2_of(c)
    trials = oh.trials_of(c)
    assert int(np.argmin(stats["nelcbo"])) == int(c["best_slot"])
    assert len(seen) == len(trials)
    for got, want in zip(seen, trials):
        assert np.array_equal(got["cand"], want["cand"]) and got["idx"] == want["idx"] and got["accept"] == want["accept"]
        assert got["threshold"] == want["threshold"]
        ev = oh.eval_of(c, want["eval"])
        assert close(got["out"][1], ev["G"], REL_GP) and close_var(got["out"][4], ev["varG"], sf2)
        assert close_var(got["out"][6], ev["var_ss"], sf2) and close_var(got["out"][3], ev["varF"], sf2)
        assert close(got["out"][2], ev["H"], REL_MC, 1.0) and close(got["out"][0], ev["nelbo"], REL_MC, 1.0)
    assert pruned == int(c["pruned"]) and vp.K == int(c["fin_K"])
    for a in oh.ATTRS:
        want = np.asarray(c["fin_" + a])
        got = np.asarray(getattr(vp, a)).reshape(want.shape)
        assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))), a
    assert set(vp.stats) == {"elbo", "elbo_sd", "e_log_joint", "e_log_joint_sd", "entropy", "entropy_sd", "stable", "I_sk", "J_sjk"}
    assert vp.stats["stable"] is False
    assert close(vp.stats["elbo"], float(c["stats_elbo"]), REL_MC, 1.0) and close(vp.stats["entropy"], float(c["stats_entropy"]), REL_MC, 1.0)
    assert close(vp.stats["e_log_joint"], float(c["stats_e_log_joint"]), REL_GP)
    assert close(vp.stats["elbo_sd"], float(c["stats_elbo_sd"]), REL_GP)
    assert close(vp.stats["e_log_joint_sd"], float(c["stats_e_log_joint_sd"]), REL_GP)
    assert vp.stats["entropy_sd"] == 0.0
    assert close_var(var_ss, float(c["var_ss"]), sf2)
    assert vp.stats["I_sk"].shape == c["stats_I_sk"].shape and vp.stats["J_sjk"].shape == c["stats_J_sjk"].shape  # (S, K0, K')
    assert np.all(np.abs(vp.stats["I_sk"] - c["stats_I_sk"]) <= REL_GP * np.abs(c["stats_I_sk"]))
    assert np.max(np.abs(vp.stats["J_sjk"] - c["stats_J_sjk"])) <= REL_GP * min(sf2, np.max(np.abs(c["stats_J_sjk"])))
    assert state_is_final(c)


@pytest.mark.parametrize("name", names())
def test_last_stage_from_the_recorded_iterates(z, ctx, name):
    c = oh.load_case(z, name)
    out, seen, infos, stats = last_stage(c, ctx, True)
    check_last_stage(c, out, seen, stats)
    K0, S = int(c["shape"][1]), int(c["shape"][3])
    alive = list(range(K0))
    for t, i in zip(seen, infos):  # after each trial: the record as before it, and no GP launch since it was made
        assert (i["S"], i["K0"], i["K_alive"]) == (S, K0, len(alive)) and np.array_equal(i["alive"], alive)
        assert i["gp_launches"] == 0
        if t["accept"]:
            alive.pop(t["idx"])


def test_device_false_equals_device_true(z, ctx):
    c = oh.load_case(z, "d2k6n20s3_mixed")
    a, seen_a, _, stats_a = last_stage(c, ctx, True)
    b, seen_b, _, stats_b = last_stage(c, ctx, False)
    check_last_stage(c, b, seen_b, stats_b)
    assert a[2] == b[2] and [t["idx"] for t in seen_a] == [t["idx"] for t in seen_b]
    sf2 = sf2_of(c)
    for ta, tb in zip(seen_a, seen_b):
        for k, tol, floor in ((1, REL_GP, 0.0), (2, REL_MC, 1.0), (0, REL_MC, 1.0)):
            assert close(ta["out"][k], tb["out"][k], tol, floor), k
        for k in (3, 4, 6):
            assert close_var(ta["out"][k], tb["out"][k], sf2), k
    for attr in oh.ATTRS:
        assert np.allclose(getattr(a[0], attr), getattr(b[0], attr), rtol=1e-12, atol=0)
    assert close_var(a[1], b[1], sf2)


# ---- the whole call ----------------------------------------------------------------------------------------------------------------

def test_whole_call_with_the_device_optimiser(z, ctx):
    """Checks the ASSEMBLY (sieve -> device Adam -> full ELCBO -> selection -> pruning -> stats), not parity: the device
    Adam draws from Philox, so its iterates are not the reference's.  The final ELBO has to lie within the reference's
    recorded range over 8 seeds, widened by that range on each side."""
    from pyvbmc_amd import optimize_vp

    c = oh.load_case(z, "d3k5n30s1_accept")
    D, K, N, S, fast_N, slow_N = (int(v) for v in c["shape"])
    lo, hi = float(np.min(c["elbo_seeds"])), float(np.max(c["elbo_seeds"]))
    vp, gp = package_vp(c, ctx), case_gp(c, ctx)
    base_w = vp.w.copy()
    vp1, var_ss, pruned = optimize_vp(oh.options_of(c), {"warmup": False, "entropy_switch": False}, vp, gp, fast_N, slow_N, K,
                                      rng="philox", seed=12345, ctx=ctx)
    print(f"final elbo {vp1.stats['elbo']:.4f}, reference over 8 seeds [{lo:.4f}, {hi:.4f}], pruned {pruned}")
    assert lo - (hi - lo) <= vp1.stats["elbo"] <= hi + (hi - lo)
    assert vp1 is not vp and np.array_equal(vp.w, base_w) and vp.bounds is not None
    assert vp1.K == K - pruned and vp1.mu.shape == (D, vp1.K) and abs(np.sum(vp1.w) - 1.0) < 1e-12
    assert vp1.stats["I_sk"].shape == (S, vp1.K) and vp1.stats["J_sjk"].shape == (S, K, vp1.K)
    assert var_ss == 0.0 and np.isfinite(vp1.stats["elbo_sd"])  # (S = 1)
    # the same seed gives the same call
    vp2, _, pruned2 = optimize_vp(oh.options_of(c), {"warmup": False, "entropy_switch": False}, package_vp(c, ctx), gp, fast_N,
                                  slow_N, K, rng="philox", seed=12345, ctx=ctx)
    assert pruned2 == pruned and vp2.stats["elbo"] == vp1.stats["elbo"]


def test_whole_call_takes_the_scipy_branch_at_one_component(z, ctx):
    from pyvbmc_amd import optimize_vp

    c = oh.load_case(z, "d3k1n20s1_scipy")
    D, K, N, S, fast_N, slow_N = (int(v) for v in c["shape"])
    vp = package_vp(c, ctx)  # (before the seed: the constructor draws its initial means)
    np.random.seed(int(c["seed"]))
    vp1, var_ss, pruned = optimize_vp(oh.options_of(c), {"warmup": False, "entropy_switch": False}, vp, case_gp(c, ctx), fast_N,
                                      slow_N, K, rng="numpy", ctx=ctx)
    assert pruned == 0 and vp1.K == 1
    # K = 1 has no stochastic stage: the whole call is on the reference's stream and ends where it ended
    assert state_is_final(c)
    assert close(vp1.stats["elbo"], float(c["stats_elbo"]), 1e-3, 1.0)  # (SciPy's iterates at det_entropy_tol_opt = 1e-3)


def assembled(vp1, D, K, S, pruned):
    assert vp1.K == K - pruned and vp1.mu.shape == (D, vp1.K) and abs(np.sum(vp1.w) - 1.0) < 1e-12
    assert vp1.stats["I_sk"].shape == (S, vp1.K) and vp1.stats["J_sjk"].shape == (S, K, vp1.K)
    assert all(np.isfinite(vp1.stats[k]) for k in ("elbo", "elbo_sd", "e_log_joint", "e_log_joint_sd", "entropy"))
    assert vp1.stats["elbo"] == vp1.stats["e_log_joint"] + vp1.stats["entropy"]


@pytest.mark.parametrize("name", ["d4k9n40s2_accept", "d2k6n20s3_mixed"])
def test_whole_call_with_several_slow_starts(z, ctx, name):
    """The choice of the starts by type (:187-199) through the public function: three slow starts (one of each type) and
    two (type 1, then type 2 or 3).  Assembly, not parity: the device Adam draws from Philox, so the iterates are not the
    reference's; asserted are the number of starts, that each has its own posterior, and the structure of the result."""
    o = ov()
    c = oh.load_case(z, name)
    D, K, N, S, fast_N, slow_N = (int(v) for v in c["shape"])
    assert slow_N in (2, 3)
    seen = []
    orig = o.optimize_one

    def spy(*a, **kw):
        seen.append(a[4])  # vp0
        return orig(*a, **kw)

    o.optimize_one = spy
    try:
        vp1, var_ss, pruned = o.optimize_vp(oh.options_of(c), {"warmup": False, "entropy_switch": False}, package_vp(c, ctx),
                                            case_gp(c, ctx), fast_N, slow_N, K, rng="philox", seed=77, ctx=ctx)
    finally:
        o.optimize_one = orig
    assert len(seen) == slow_N and len({id(v) for v in seen}) == slow_N
    assembled(vp1, D, K, S, pruned)
    assert np.isfinite(var_ss) and var_ss > 0  # (S > 1)
    ref = float(c["stats_elbo"])
    print(f"{name}: elbo {vp1.stats['elbo']:.4f} (the reference's seeded run: {ref:.4f}), pruned {pruned}")


def test_whole_call_with_the_host_optimiser_and_in_warm_up(z, ctx):
    """``adam="host"`` (``minimize_adam`` around ``_neg_elcbo`` on the call's stream) and the warm-up switch (:142-143)
    through the public function, on the smallest case.  Assembly: with warm-up the weights are not optimised, nothing is
    pruned and the caller's posterior has its flag switched off, as the reference leaves it."""
    from pyvbmc_amd import optimize_vp

    c = oh.load_case(z, "d2k2n20s2_to_one")
    D, K, N, S, fast_N, slow_N = (int(v) for v in c["shape"])
    gp = case_gp(c, ctx)
    vp = package_vp(c, ctx)
    np.random.seed(int(c["seed"]))
    vp1, var_ss, pruned = optimize_vp(oh.options_of(c), {"warmup": False, "entropy_switch": False}, vp, gp, fast_N, slow_N, K,
                                      rng="numpy", adam="host", ctx=ctx)
    assembled(vp1, D, K, S, pruned)
    print(f"adam=host on the reference's stream: elbo {vp1.stats['elbo']:.6f} (reference {float(c['stats_elbo']):.6f}), "
          f"pruned {pruned} (reference {int(c['pruned'])}), stream ends where the reference's ends: {state_is_final(c)}")
    # every draw of this call is the reference's, in its order (sieve, Adam's entropy draws, the full evaluations, the
    # trial): the run is the recorded one -- the same trial, the stream where the reference left it, the ELBO to the
    # project's Monte-Carlo parity bound
    assert pruned == int(c["pruned"]) and state_is_final(c)
    assert close(vp1.stats["elbo"], float(c["stats_elbo"]), REL_MC, 1.0)
    assert vp.optimize_weights is True
    vp = package_vp(c, ctx)
    vp2, _, pruned2 = optimize_vp(oh.options_of(c), {"warmup": True, "entropy_switch": False}, vp, gp, fast_N, slow_N, K,
                                  rng="philox", seed=3, ctx=ctx)
    assert vp.optimize_weights is False and vp2.optimize_weights is False and pruned2 == 0
    assembled(vp2, D, K, S, 0)
    assert np.allclose(vp2.w, 1.0 / K)  # (the sieve's candidates carry equal weights when they are not optimised, :969-985)
