"""CPU tests of the ``train_gp`` mirror (pyvbmc_amd/gaussian_process_train.py): what the reference decides against
tests/golden/train_gp.npz -- recorded from the reference's own functions on the plain dicts of tests/train_gp_cases.py
by tools/train_gp_golden.py -- the MATLAB known answer of ``_estimate_noise``, the package's own box rule,
``train_gp(device=False)`` with its bookkeeping and its use of NumPy's global stream, the refusals and the patch."""
import copy
import math
import sys
import types
from pathlib import Path

import numpy as np
import pytest
from scipy.stats import norm

import train_gp_cases as tc

GOLDEN = Path(__file__).parent / "golden" / "train_gp.npz"
# the same FP64 formulas as the reference's: the margin covers a different but fixed summation order over at most a few
# hundred terms
RTOL = 1e-12


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def close(a, b):
    return np.shape(a) == np.shape(b) and np.allclose(a, b, rtol=RTOL, atol=0, equal_nan=True)


def make_gp(mean, noisy=False):
    from pyvbmc_amd import gp as gpm
    from pyvbmc_amd.gaussian_process_train import _meanfun_name_to_mean_function

    return gpm.GP(tc.D, gpm.SquaredExponential(), _meanfun_name_to_mean_function(mean),
                  gpm.GaussianNoise(constant_add=True, user_provided_add=noisy))


# ------------------------------------------------------------------------------------------------ _estimate_noise
def test_estimate_noise_matlab_known_answer():
    """The setup of the reference's own test (testing/vbmc/test_gaussian_process_train.py:19-50), restated with the
    package's squared-exponential kernel in D = 1: the estimate depends on hyp[cov_N] and s2 alone."""
    from pyvbmc_amd import gp as gpm
    from pyvbmc_amd.gaussian_process_train import _estimate_noise

    state = np.random.get_state()
    np.random.seed(1234)
    N = 31
    X = -5 + np.random.rand(N, 1) * 10
    s2 = 0.05 * np.exp(0.5 * X)
    y = np.sin(X) + np.sqrt(s2) * norm.ppf(np.random.random_sample(X.shape))
    y[y < 0] = -np.abs(3 * y[y < 0]) ** 2
    np.random.set_state(state)
    gp = gpm.GP(1, gpm.SquaredExponential(), gpm.NegativeQuadratic(), gpm.GaussianNoise(constant_add=True, user_provided_add=True))
    gp.update(X_new=X, y_new=y, s2_new=s2, hyp=np.array([[-2.5, 1.7, -7.5, 0.3, 2.6, 1.2]]))
    assert np.isclose(_estimate_noise(gp), 0.106582207806606)


# --------------------------------------------------------------------- what the reference decides, against the golden
@pytest.mark.parametrize("name", list(tc.training_option_cases()))
def test_training_options_and_hyp_cov_against_the_reference(golden, name):
    from pyvbmc_amd.gaussian_process_train import _get_gp_training_options, _get_hyp_cov

    st, hist, opts, hd, s_N = tc.training_option_cases()[name]
    before = copy.deepcopy((st, opts, hd))
    cov = _get_hyp_cov(st, hist, opts, hd)
    ref = golden[f"cov/{name}"]
    assert (cov is None and ref.size == 0) or close(cov, ref), name
    got = _get_gp_training_options(st, hist, opts, hd, s_N)
    keys = {k.split("/")[2] for k in golden if k.startswith(f"opt/{name}/")}
    assert set(got) == keys, (name, set(got) ^ keys)
    for k, v in got.items():
        ref = golden[f"opt/{name}/{k}"]
        if isinstance(v, str):
            assert str(ref) == v, (name, k, v, ref)
        elif v is None:
            assert ref.size == 0, (name, k)
        else:
            assert close(np.asarray(v, dtype=np.float64), ref), (name, k, v, ref)
    assert repr(before) == repr((st, opts, hd))  # (nothing given is modified)


def test_training_option_cases_cover_the_branches(golden):
    s = lambda name, k: golden[f"opt/{name}/{k}"]
    assert {str(s(f"first_{n}", "sampler")) for n in tc.SAMPLERS} == set(tc.SAMPLERS)
    assert str(s("laplace_small", "sampler")) == "slicesample" and str(s("cov_over_thresh", "sampler")) == "slicesample"
    assert s("later_covsample", "widths").ndim == 2 and s("later_mala", "widths").ndim == 1 and s("mala_step", "step_size") == 0.3
    assert (s("recompute_no_samples", "opts_N"), s("first_slicesample", "opts_N")) == (2, 1)
    assert (s("retrain_samples", "opts_N"), s("retrain_samples", "init_N")) == (0, 0) and s("retrain_no_samples", "opts_N") == 1
    assert s("no_retrain_unreliable", "init_N") >= 9 and s("no_retrain_unreliable_no_samples", "opts_N") == 2
    assert s("later_slicelite", "thin") == 1 and s("no_widths", "widths").size == 0
    assert s("first_slicesample", "init_N") > s("late_n_eff", "init_N") >= 9
    # (the weighted form is square in the number of samples, 4, as the reference's array handling makes it; the running
    # one in the number of hyper-parameters, 9)
    assert golden["cov/first_slicesample"].size == 0 and golden["cov/running_cov"].shape == (9, 9)
    assert golden["cov/weighted_break"].shape == golden["cov/later_slicesample"].shape == (4, 4)
    with pytest.raises(ValueError, match="Unknown MCMC sampler"):
        from pyvbmc_amd.gaussian_process_train import _get_gp_training_options

        _get_gp_training_options(tc.optim_state(), tc.history(0), tc.options(gp_hyp_sampler="hmc"), dict(run_cov=None), 4)


@pytest.mark.parametrize("name", list(tc.gp_hyp_cases()))
def test_gp_hyp_against_the_reference(golden, name):
    from pyvbmc_amd.gaussian_process_train import _gp_hyp

    st, opts, noisy = tc.gp_hyp_cases()[name]
    X, y, _ = tc.data(noisy)
    gp = make_gp(st["gp_mean_fun"], noisy)
    gp, hyp0, s_N = _gp_hyp(st, opts, tc.PLB, tc.PUB, gp, X, y)
    assert close(hyp0, golden[f"hyp/{name}/hyp0"]) and s_N == golden[f"hyp/{name}/gp_s_N"] and isinstance(s_N, int)
    ref_b, pri = gp.temporary_data["reference_bounds"], gp.get_priors()
    for nm, _, n in gp._blocks():
        lo, hi = (np.array(np.broadcast_to(np.ravel(v), (n,)), dtype=np.float64) for v in ref_b[nm])
        assert close(lo, golden[f"hyp/{name}/lb/{nm}"]) and close(hi, golden[f"hyp/{name}/ub/{nm}"]), (name, nm)
        kind, ref = str(golden[f"hyp/{name}/prior_kind/{nm}"]), golden[f"hyp/{name}/prior/{nm}"]
        if kind == "none":
            assert pri[nm] is None
        else:
            assert pri[nm][0] == kind and close(np.stack([np.broadcast_to(v, (n,)) for v in pri[nm][1]]), ref), (name, nm)
    # the package's own rule: the box is finite and ordered, what the reference decided stands, the design box lies inside
    b = gp.get_bounds(as_array=True)
    lb, ub = b["lb"], b["ub"]
    assert np.all(np.isfinite(lb)) and np.all(np.isfinite(ub)) and np.all(lb <= ub)
    for nm, f, n in gp._blocks():
        lo, hi = golden[f"hyp/{name}/lb/{nm}"], golden[f"hyp/{name}/ub/{nm}"]
        assert close(lb[f : f + n][np.isfinite(lo)], lo[np.isfinite(lo)]), (name, nm)
        keep = np.isfinite(hi) & (hi >= lb[f : f + n])
        assert close(ub[f : f + n][keep], hi[keep]), (name, nm)
    dlb, dub = gp.temporary_data["design_box"]
    assert np.all(dlb >= lb) and np.all(dub <= ub) and np.all(dlb <= dub)
    assert np.all(hyp0[: tc.D + 1] >= lb[: tc.D + 1])


def test_gp_hyp_cases_cover_the_branches(golden):
    g = lambda name, k: golden[f"hyp/{name}/{k}"]
    lo = math.log(tc.options()["tol_gp_noise"])
    assert g("mean_negquad", "hyp0")[tc.D + 1] == lo and g("noise_size_small", "hyp0")[tc.D + 1] == lo
    assert g("noise_size", "hyp0")[tc.D + 1] == math.log(0.02) and g("level2", "hyp0")[tc.D + 1] == lo
    assert np.isfinite(g("mean_const", "ub/mean_const")) and np.isfinite(g("mean_negquad", "ub/mean_const"))
    assert np.isinf(g("no_quadratic_bound", "ub/mean_const")) and "hyp/mean_zero/ub/mean_const" not in golden
    assert np.all(np.isnan(g("mean_negquad", "ub/covariance_log_lengthscale")))  # (left to gpyreg by the reference)
    assert np.all(np.isfinite(g("mean_negquad", "lb/covariance_log_lengthscale")))
    assert str(g("mean_negquad", "prior_kind/noise_log_scale")) == "student_t"
    assert [int(g(n, "gp_s_N")) for n in ("mean_negquad", "main_phase", "stable_by_N", "stable_by_K", "stopped")] == [8, 10, 3, 2, 1]


def test_unsupported_noise_levels_and_covariances():
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gaussian_process_train import _cov_identifier_to_covariance_function, _gp_hyp, _meanfun_name_to_mean_function

    X, y, _ = tc.data()
    with pytest.raises(_lib.UnsupportedShape):
        _gp_hyp(tc.optim_state(uncertainty_handling_level=1), tc.options(), tc.PLB, tc.PUB, make_gp("const"), X, y)
    for ident in (3, [3, 1]):
        with pytest.raises(_lib.UnsupportedShape):
            _cov_identifier_to_covariance_function(ident)
    with pytest.raises(ValueError, match="Unknown covariance"):
        _cov_identifier_to_covariance_function(7)
    with pytest.raises(ValueError, match="Unknown mean"):
        _meanfun_name_to_mean_function("linear")


def test_box_passes_fit_for_the_three_means():
    """The final box passes ``GP.fit``'s finiteness check: a fit without optimiser and chains runs for every mean."""
    from pyvbmc_amd.gaussian_process_train import _gp_hyp

    X, y, _ = tc.data()
    for mean in tc.MEANS:
        gp = make_gp(mean)
        gp, hyp0, _ = _gp_hyp(tc.optim_state(gp_mean_fun=mean), tc.options(), tc.PLB, tc.PUB, gp, X, y)
        dlb, dub = gp.temporary_data["design_box"]
        hyp, opt, smp = gp.fit(X, y, None, hyp0=hyp0, options=dict(init_N=3, opts_N=0, n_samples=0, design_lb=dlb, design_ub=dub),
                               device=False, seed=5, optimizer="fused")
        assert hyp.shape == (1, tc.P_OF[mean]) and smp is None and np.isfinite(opt["log_post"])
        assert np.all(opt["candidates"][1:] >= dlb) and np.all(opt["candidates"][1:] <= dub)


# ------------------------------------------------------------------------------------------- train_gp on the host
SMALL = dict(gp_train_n_init=12, gp_train_n_init_final=9, ns_gp_max=24, ns_gp_max_warmup=3, gp_sample_thin=2, gp_tol_opt=1e-3)


def run_twice(device, ctx=None, noisy=False):
    """``train_gp`` twice in a row on the stand-ins, the second call with the first call's GP in the history: the calls'
    results, and the state of NumPy's global stream a replay of the reference's sub-sampling leaves."""
    from pyvbmc_amd.gaussian_process_train import train_gp

    opts = tc.options(**SMALL)
    st = tc.optim_state(gp_noise_fun=[1, int(noisy), 0], uncertainty_handling_level=2 if noisy else 0)
    log = tc.logger(noisy)
    hd = {}
    hist0 = dict(r_index=np.array([]), sKL=np.array([]), gp_hyp_full=[], gp=np.array([], dtype=object))
    np.random.seed(77)
    first = train_gp(hd, st, log, hist0, opts, tc.PLB, tc.PUB, device=device, seed=41, ctx=ctx)
    untouched = np.random.get_state()[1].copy()
    np.random.seed(77)
    assert np.array_equal(untouched, np.random.get_state()[1])  # iteration 0 draws nothing from the global stream
    gp1, hd1 = first[0], copy.deepcopy(first[3])
    gps = np.empty(1, dtype=object)
    gps[0] = gp1
    hist1 = dict(r_index=np.array([2.0]), sKL=np.array([np.inf, 0.2]), gp_hyp_full=[gp1.get_hyperparameters()], gp=gps)
    st2 = dict(st, iter=1, recompute_var_post=False)
    np.random.seed(78)
    second = train_gp(hd, st2, log, hist1, opts, tc.PLB, tc.PUB, device=device, seed=42, ctx=ctx)
    after = np.random.get_state()[1].copy()
    return opts, (first, hd1), (second, hd), gp1, after


def check_results(opts, first, second, gp1):
    from pyvbmc_amd.gaussian_process_train import _get_gp_training_options

    P = tc.P_OF["negquad"]
    for (gp, s_N, sn2, out), hd in (first, second):
        assert set(out) == set(hd)
        assert set(hd) == {"hyp", "warp", "logp", "full", "run_cov"} and hd["warp"] is None
        assert s_N == 3 and hd["hyp"].shape == (3, P) and hd["full"].shape == (3, P) and hd["logp"].shape == (3,)
        assert np.array_equal(gp.get_hyperparameters(), hd["hyp"]) and len(gp.posteriors) == s_N
        b = gp.get_bounds(as_array=True)
        assert np.all(hd["hyp"] >= b["lb"]) and np.all(hd["hyp"] <= b["ub"])
        assert np.isfinite(sn2) and sn2 >= opts["tol_gp_noise"] ** 2
        assert hd["run_cov"].shape == (P, P)
    # the running covariance: the first call's is the samples' covariance, the second mixes it in (:180-189)
    (_, hd1), (_, hd2) = first, second
    assert np.allclose(hd1["run_cov"], np.cov(hd1["full"].T), rtol=1e-12, atol=0)
    w = opts["hyp_run_weight"] ** opts["fun_evals_per_iter"]
    assert np.allclose(hd2["run_cov"], (1 - w) * np.cov(hd2["full"].T) + w * hd1["run_cov"], rtol=1e-12, atol=1e-300)
    assert not np.array_equal(hd1["hyp"], hd2["hyp"])


def test_train_gp_on_the_host_twice():
    from pyvbmc_amd.gaussian_process_train import _get_gp_training_options

    opts, first, second, gp1, after = run_twice(False)
    check_results(opts, first, second, gp1)
    # the second call's hyp0 came from the history: 3 samples > init_N / 2 ... only where init_N < 6; here init_N >= 9, so
    # all three rows are kept and nothing is drawn -- unless the sub-sample applies.  Replay the reference's rule.
    st2 = tc.optim_state(iter=1, recompute_var_post=False)
    hist1 = dict(r_index=np.array([2.0]), sKL=np.array([np.inf, 0.2]), gp_hyp_full=[gp1.get_hyperparameters()])
    init_N = _get_gp_training_options(st2, hist1, opts, dict(run_cov=first[1]["run_cov"]), 3)["init_N"]
    np.random.seed(78)
    if 3 > init_N / 2:
        np.random.choice(3, math.ceil(init_N / 2), replace=False)
    assert np.array_equal(after, np.random.get_state()[1])
    cand = second[0][0]  # (the GP of the second call; its fit saw the history's rows among its candidates)
    assert cand is not gp1


def test_train_gp_subsamples_the_history_on_the_global_stream():
    """More history rows than ``init_N / 2``: ``np.random.choice`` on the global stream picks ``ceil(init_N / 2)`` of them,
    and the stream is consumed by exactly that draw."""
    from pyvbmc_amd.gaussian_process_train import train_gp

    opts = tc.options(**SMALL)
    log = tc.logger()
    st = tc.optim_state()
    np.random.seed(5)
    gp0, _, _, hd = train_gp({}, st, log, dict(r_index=np.array([]), sKL=np.array([]), gp_hyp_full=[], gp=[]), opts, tc.PLB,
                             tc.PUB, device=False, seed=1)
    gps = np.empty(4, dtype=object)
    for i in range(4):
        gps[i] = gp0  # four past iterations of 3 samples: the second half (indices 1 .. 3) gives 9 rows > init_N / 2
    hist = dict(r_index=np.array([np.inf, 3.0, 2.0, 1.5]), sKL=np.array([np.inf, 0.3, 0.2, 0.1, 0.05]),
                gp_hyp_full=[gp0.get_hyperparameters()] * 4, gp=gps)
    seen = {}
    real_fit = type(gp0).fit

    def spy(self, *a, **kw):
        seen["hyp0"], seen["options"] = kw["hyp0"], kw["options"]
        return real_fit(self, *a, **kw)

    type(gp0).fit = spy
    try:
        np.random.seed(9)
        train_gp(dict(hd), dict(st, iter=4), log, hist, opts, tc.PLB, tc.PUB, device=False, seed=2)
        after = np.random.get_state()[1].copy()
    finally:
        type(gp0).fit = real_fit
    init_N = seen["options"]["init_N"]
    assert 9 <= init_N < 18 and seen["options"]["opts_N"] == 1 and seen["options"]["n_samples"] == 3
    np.random.seed(9)
    rows = np.concatenate([gp0.get_hyperparameters()] * 3)
    pick = rows[np.random.choice(9, math.ceil(init_N / 2), replace=False)]
    assert np.array_equal(after, np.random.get_state()[1])
    assert np.array_equal(seen["hyp0"], np.unique(np.concatenate([pick, np.atleast_2d(hd["hyp"])]), axis=0))


def test_refusal_before_side_effects():
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gaussian_process_train import train_gp

    log = tc.logger()
    hist = dict(r_index=np.array([]), sKL=np.array([]), gp_hyp_full=[], gp=[])
    for st, opts in ((tc.optim_state(), tc.options(gp_hyp_sampler="mala")), (tc.optim_state(), tc.options(gp_hyp_sampler="laplace")),
                     (tc.optim_state(gp_noise_fun=[1, 2, 0]), tc.options()), (tc.optim_state(gp_noise_fun=[1, 0, 1]), tc.options()),
                     (tc.optim_state(gp_noise_fun=[0, 1, 0]), tc.options()),
                     (tc.optim_state(uncertainty_handling_level=1), tc.options()), (tc.optim_state(gp_cov_fun=3), tc.options())):
        hd = {"hyp": None, "marker": 1}
        np.random.seed(3)
        before = np.random.get_state()[1].copy()
        with pytest.raises(_lib.UnsupportedShape):
            train_gp(hd, st, log, hist, opts, tc.PLB, tc.PUB, device=False)
        assert hd == {"hyp": None, "marker": 1} and np.array_equal(before, np.random.get_state()[1])
    # laplace with few effective points is slice sampling, as in the reference
    out = train_gp({}, tc.optim_state(n_eff=20), log, hist, tc.options(gp_hyp_sampler="laplace", **SMALL), tc.PLB, tc.PUB,
                   device=False, seed=3)
    assert out[1] == 3 and len(out[0].posteriors) == 3


# -------------------------------------------------------------------------------------------------------- the patch
def test_patch_train_gp_on_stand_in_modules(monkeypatch):
    import pyvbmc_amd
    from pyvbmc_amd import _lib

    calls = []

    def reference(*a):
        calls.append(("reference", a))
        return "reference"

    def mirror(*a, **kw):
        calls.append(("mirror", a, kw))
        if a[0].get("refuse"):
            raise _lib.UnsupportedShape("refused")
        return "mirror"

    monkeypatch.setattr(sys.modules["pyvbmc_amd.gaussian_process_train"], "train_gp", mirror)
    mods = [types.ModuleType(n) for n in ("gpt_stand_in", "vbmc_stand_in", "loop_stand_in", "bystander")]
    for mod in mods[:3]:
        mod.train_gp = reference
    done = pyvbmc_amd.patch_train_gp(mods, device=False, seed=4)
    assert done == mods[:3] and not hasattr(mods[3], "train_gp")
    args = ({}, 1, 2, 3, 4, 5, 6)
    for mod in mods[:3]:
        assert mod.train_gp is not reference and mod.train_gp(*args) == "mirror"
    assert calls[-1] == ("mirror", args, dict(device=False, seed=4))
    refused = ({"refuse": True}, 1, 2, 3, 4, 5, 6)
    assert mods[1].train_gp(*refused) == "reference" and calls[-1] == ("reference", refused)
    again = pyvbmc_amd.patch_train_gp(mods)  # idempotent: the reference stays the saved binding
    assert again == mods[:3] and mods[0].train_gp(*refused) == "reference"
    pyvbmc_amd.unpatch_train_gp(mods)
    assert all(mod.train_gp is reference for mod in mods[:3])
    with pytest.raises(TypeError):
        pyvbmc_amd.patch_train_gp(mods, rng="philox")
