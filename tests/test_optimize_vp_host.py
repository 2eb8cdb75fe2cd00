"""``optimize_vp``'s last stage without a GPU: the NumPy statement tests/optimize_vp_host.py against the reference's
recorded evaluations and trials (tests/golden/optimize_vp.npz, tools/make_optimize_vp_golden.py), the package's own NumPy
re-weighting (``pyvbmc_amd.optimize_vp.reweight``) against that statement, the refusals, ``patch_optimize_vp``.

Bounds.  The re-weighting identity: 1e-10 relative, the project's GP parity figure (the reference alone gives ~4e-13 on
these shapes: the renormalisation's rounding).  Choices, decisions, ``pruned``, shapes: exactly.  The final arrays: the
statement makes the reference's own NumPy calls, so ``np.array_equal``.
"""
import importlib
from types import SimpleNamespace

import numpy as np
import optimize_vp_host as oh
import pytest

from pyvbmc_amd import VariationalPosterior, _lib, dropin

ov = importlib.import_module("pyvbmc_amd.optimize_vp")
REL = 1e-10


@pytest.fixture(scope="module")
def z():
    return np.load(oh.GOLDEN, allow_pickle=False)


def names():
    return oh.case_names(np.load(oh.GOLDEN, allow_pickle=False))


def rel(a, b):
    return abs(a - b) / max(abs(b), np.finfo(np.float64).tiny)


def winner(c):
    e = oh.eval_of(c, int(c["best_eval"]))
    D, K = int(c["shape"][0]), int(c["shape"][1])
    vp = VariationalPosterior(D, K)
    for a in oh.ATTRS:
        setattr(vp, a, np.array(c["base_" + a]))
    vp.set_parameters(e["theta"])
    m = {a: np.array(getattr(vp, a), dtype=np.float64) for a in oh.ATTRS}
    m["eta"] = e["theta"][-K:].reshape(1, -1)
    return e, m


def replay(c):
    """The statement's pruning loop fed the recorded trial evaluations; returns its outputs and the (alive, mixture) of
    every trial."""
    e, m = winner(c)
    o = oh.options_of(c)
    K = int(c["shape"][1])
    trials = oh.trials_of(c)
    seen = []
    it = iter(trials)
    rs = iter(trials)

    def trial(m_pruned, alive, pos):
        t = next(it)
        seen.append((t, list(alive), m_pruned))
        return {k: v for k, v in oh.eval_of(c, t["eval"]).items() if k in oh.OUT11}

    thr = o["tol_improvement"] * o.eval("pruning_threshold_multiplier", {"K": K})
    out = oh.prune_loop(m, -e["nelbo"], np.sqrt(e["varF"]), e["I_sk"], e["J_sjk"], o["tol_weight"], thr, o["elcbo_impro_weight"],
                        trial, lambda n: next(rs)["r"])
    return e, out, seen, trials


def test_fixture_has_the_kinds_of_run_the_issue_names(z):
    acc = {n: int(np.sum(oh.load_case(z, n)["trial_accept"])) for n in names()}
    rej = {n: int(oh.load_case(z, n)["n_trials"]) - acc[n] for n in names()}
    assert any(acc[n] >= 3 for n in names()) and any(acc[n] == 0 and rej[n] > 0 for n in names())
    assert any(acc[n] > 0 and rej[n] > 0 for n in names())
    assert int(oh.load_case(z, "d2k2n20s2_to_one")["fin_K"]) == 1
    assert int(oh.load_case(z, "d3k1n20s1_scipy")["adam_iters"].size) == 0


@pytest.mark.parametrize("name", names())
def test_reweighting_identity_against_the_recorded_trials(z, name):
    c = oh.load_case(z, name)
    e, out, seen, trials = replay(c)
    worst = 0.0
    for t, alive, m_pruned in seen:
        want = oh.eval_of(c, t["eval"])
        for fn in (oh.reweight, ov.reweight):
            G, varG, var_ss = fn(e["I_sk"], e["J_sjk"], alive, m_pruned["w"])
            errs = (rel(G, want["G"]), rel(varG, want["varG"]), rel(var_ss, want["var_ss"]) if want["var_ss"] else abs(var_ss))
            worst = max(worst, *errs)
            assert max(errs) <= REL, (name, t, errs)
    # the winner's own evaluation is the identity on all columns
    K = e["K"]
    _, m = winner(c)
    G, varG, var_ss = ov.reweight(e["I_sk"], e["J_sjk"], range(K), m["w"])
    assert max(rel(G, e["G"]), rel(varG, e["varG"])) <= REL and abs(var_ss - e["var_ss"]) <= REL * max(1.0, e["var_ss"])
    print(f"{name}: {len(seen)} trials, worst relative error {worst:.2e} (bound {REL:.0e})")


@pytest.mark.parametrize("name", names())
def test_pruning_loop_reproduces_the_recorded_run(z, name):
    c = oh.load_case(z, name)
    e, (m, kept, pruned, I_fin, J_fin, alive, log), seen, trials = replay(c)
    S, K0 = int(c["shape"][3]), int(c["shape"][1])
    assert len(log) == len(trials) == int(c["n_trials"])
    for got, want in zip(log, trials):
        assert np.array_equal(got["cand"], want["cand"]) and got["idx"] == want["idx"] and got["accept"] == want["accept"]
        assert got["delta"] == want["delta"] and got["threshold"] == want["threshold"]
    assert pruned == int(c["pruned"]) and np.array_equal(alive, c["alive"])
    for a in oh.ATTRS:
        assert np.array_equal(np.ravel(m[a]), np.ravel(c["fin_" + a])), a
    Kf = K0 - pruned
    assert I_fin.shape == (S, Kf) and J_fin.shape == (S, K0, Kf) == c["stats_J_sjk"].shape  # (axis 2 only, :376)
    assert np.array_equal(I_fin, c["stats_I_sk"]) and np.array_equal(J_fin, c["stats_J_sjk"])
    # the square block of the survivors, as optimize_vp's docstring says to take it
    assert np.array_equal(J_fin[:, alive, :], e["J_sjk"][:, alive][:, :, alive])
    if kept is not None:
        assert -kept["nelbo"] == float(c["stats_elbo"]) and kept["var_ss"] == float(c["var_ss"])
    # ns_ent_fine_K is recomputed at every trial's K'
    o = oh.options_of(c)
    for t, al, _ in seen:
        assert oh.ns_ent_fine_K(o["ns_ent_fine"], len(al)) == int(c["eval_ns"][t["eval"]])


def test_package_prune_vp_is_the_statement(z):
    c = oh.load_case(z, "d4k9n40s2_accept")
    _, m = winner(c)
    vp = VariationalPosterior(4, 9)
    for a in oh.ATTRS:
        setattr(vp, a, m[a].copy())
    for idx in (0, 8, 4):
        v, theta = ov._prune_vp(vp, idx)
        want, th = oh.prune_mixture(m, idx)
        assert v.K == 8 and vp.K == 9
        for a in oh.ATTRS:
            assert np.array_equal(np.ravel(getattr(v, a)), np.ravel(want[a])), (idx, a)


# ---- refusals ------------------------------------------------------------------------------------------------------------

OPTIONS = {"hpd_frac": 0.8, "tol_length": 1e-6, "tol_weight": 1e-2, "tol_con_loss": 0.01, "weight_penalty": 0.1,
           "ns_ent": lambda K: 100 * K ** (2 / 3), "ns_ent_fast": 0, "ns_elbo": lambda K: 50 * K,
           "ns_ent_fine": lambda K: 2**12 * K, "stochastic_optimizer": "adam", "sgd_step_size": 0.005,
           "tol_fun_stochastic": 1e-3, "max_iter_stochastic": 400, "elcbo_midpoint": True, "det_entropy_tol_opt": 1e-3,
           "elcbo_impro_weight": 3, "tol_improvement": 0.01, "pruning_threshold_multiplier": lambda K: 1 / np.sqrt(K)}


def refusal_cases():
    def vp_of(D, K, **flags):
        v = VariationalPosterior(D, K)
        for k, x in flags.items():
            setattr(v, k, x)
        return v

    return {
        "D>32": (lambda: vp_of(33, 2), None, {}, _lib.UnsupportedShape),
        "K>128": (lambda: vp_of(2, 2), 129, {}, _lib.UnsupportedShape),
        "sigma off": (lambda: vp_of(2, 2, optimize_sigma=False), None, {}, _lib.UnsupportedShape),
        "K_new<K": (lambda: vp_of(2, 3), 2, {}, _lib.UnsupportedShape),
        "ns_ent_fast": (lambda: vp_of(2, 2), None, {"ns_ent_fast": 10}, _lib.UnsupportedShape),
        "no device": (lambda: vp_of(2, 2), None, {}, _lib.NoDeviceError),
        "N too large": (lambda: vp_of(2, 2), None, {}, _lib.UnsupportedShape),
        "optimizer": (lambda: vp_of(2, 2), None, {"stochastic_optimizer": "sgd"}, ValueError),
        "rng": (lambda: vp_of(2, 2), None, {}, ValueError),
    }


@pytest.mark.parametrize("what", list(refusal_cases()))
@pytest.mark.parametrize("warmup", [False, True])
def test_refusals_leave_numpy_and_vp_untouched(what, warmup):
    make, K, opts, exc = refusal_cases()[what]
    host = _lib.Context(-1)
    try:
        vp = make()
        before = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vp.__dict__.items() if k != "_ctx"}
        r = np.random.default_rng(1)
        n = 19200 if what == "N too large" else 10  # (8 (2 D + N + 5) bytes against the GP sums' 150 KiB of LDS)
        gp = SimpleNamespace(X=r.standard_normal((n, vp.D)), y=r.standard_normal((n, 1)), posteriors=[None])
        np.random.seed(7)
        st = np.random.get_state(legacy=True)
        with pytest.raises(exc) as info:
            ov.optimize_vp(dict(OPTIONS, **opts), {"entropy_switch": False, "warmup": warmup}, vp, gp, 7, 3, K,
                           rng="mt" if what == "rng" else "philox", ctx=host)
        if what == "optimizer":
            assert str(info.value) == "Unknown stochastic optimizer!"  # the reference's (:295)
        st1 = np.random.get_state(legacy=True)
        assert np.array_equal(st[1], st1[1]) and st[2:] == st1[2:]
        after = {k: v for k, v in vp.__dict__.items() if k != "_ctx"}
        assert before.keys() == after.keys()
        for k, v in before.items():
            assert np.array_equal(v, after[k]) if isinstance(v, np.ndarray) else v is after[k], k
        assert vp.bounds is None and vp.optimize_weights is True
    finally:
        host.close()


# ---- patch_optimize_vp -----------------------------------------------------------------------------------------------------

def test_patch_optimize_vp_binds_restores_and_falls_back():
    calls = []

    def ref_optimize_vp(options, optim_state, vp, gp, fast_opts_N, slow_opts_N, K=None):
        calls.append((fast_opts_N, slow_opts_N, K))
        return "reference"

    vo = SimpleNamespace(optimize_vp=ref_optimize_vp)
    assert dropin.patch_optimize_vp(vo) is vo and vo.optimize_vp is not ref_optimize_vp
    assert vo.optimize_vp.__wrapped__ is ov.optimize_vp
    first = vo.optimize_vp
    dropin.patch_optimize_vp(vo)  # idempotent: the saved binding is still the reference's
    assert vo.optimize_vp is not first and getattr(vo, dropin._SAVED_OPTIMIZE_VP) is ref_optimize_vp
    # a refused shape (optimize_sigma off) reaches the previous binding, with the reference's arguments
    vp = VariationalPosterior(2, 2)
    vp.optimize_sigma = False
    gp = SimpleNamespace(X=np.zeros((4, 2)), y=np.zeros((4, 1)), posteriors=[None])
    state = {"entropy_switch": False, "warmup": True}
    assert vo.optimize_vp(OPTIONS, state, vp, gp, 5, 3) == "reference" and calls == [(5, 3, None)]
    assert vp.optimize_weights is True  # (the mirror refused before the warm-up switch)
    dropin.unpatch_optimize_vp(vo)
    assert vo.optimize_vp is ref_optimize_vp and not hasattr(vo, dropin._SAVED_OPTIMIZE_VP)
    dropin.unpatch_optimize_vp(vo)  # a second time changes nothing
    assert vo.optimize_vp is ref_optimize_vp


def test_patch_does_not_bind_optimize_vp():
    def ref_optimize_vp(*a):
        return "reference"

    vo = SimpleNamespace(optimize_vp=ref_optimize_vp, _neg_elcbo=lambda *a, **k: None)
    dropin.patch(vo, adam=False)
    assert vo.optimize_vp is ref_optimize_vp
    dropin.unpatch(vo)


def test_exports():
    import pyvbmc_amd

    assert pyvbmc_amd.optimize_vp is ov.optimize_vp and "optimize_vp" in pyvbmc_amd.__all__
    lib = _lib.load()
    for n in ("vbmc_elcbo_full", "vbmc_elcbo_prune_trial", "vbmc_elcbo_prune_accept", "vbmc_elcbo_put", "vbmc_elcbo_record_info"):
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    host = _lib.Context(-1)
    try:  # the entries need a device: a host-only context is refused, not served elsewhere
        out = np.empty(7)
        with pytest.raises(_lib.NoDeviceError):
            host.check(lib.vbmc_elcbo_prune_trial(host._h, 0, 2, _lib.EPS_PHILOX, 0, _lib.ptr(out)))
    finally:
        host.close()
