"""CPU tests of active_importance_sampling: the NumPy restatement (tests/ais_host.py) against the reference's recorded
outputs, and the parts of the device mirror (pyvbmc_amd/active_importance_sampling.py, pyvbmc_amd/dropin.py) that need
no device.

Bounds.  ais_host and the reference run the same float64 operations on the same inputs (the reference's GP arithmetic
behind the recorded values IS oracle/gp_ref.py, through oracle/_stubs/gpyreg), so agreement is expected to a few ulp;
the bounds below are the ones the fixtures' issue lists: the proposal points at rtol 1e-13, f_s2 and ln_weights at 1e-12,
the quantities implied by K_Xa_X / C_tmp at 1e-12 sf^2.
"""
import types

import numpy as np
import pytest

import ais_host
from oracle import gp_ref, mixture_ref

GPCOV = ["homo", "hetero", "tiny"]
KINDS = {"AcqFcnVIQR": ais_host.VIQR, "AcqFcnIMIQR": ais_host.IMIQR}
GPCOV_OPTS = {
    "AcqFcnVIQR": ais_host.Opts(active_importance_sampling_mcmc_samples=48),
    "AcqFcnIMIQR": ais_host.Opts(active_importance_sampling_vp_samples=30, active_importance_sampling_box_samples=18,
                                active_importance_sampling_mcmc_samples=0),
}


def gpcov_gp(c, name):
    s2 = c["s2"] if name == "hetero" else None
    return gp_ref.make_gp(c["X"], c["y"], c[f"{name}_hyp"], gp_ref.MEAN_NEGQUAD, s2=s2, noise_user=s2 is not None)


def gpcov_mix(c):
    return mixture_ref.Mixture.make(c["vp_mu"], c["vp_sigma"], c["vp_lambd"], c["vp_w"])


def known_gp(c):
    return gp_ref.make_gp(c["X"], c["y"], c["hyp"], gp_ref.MEAN_NEGQUAD)


def sf2_max(gp):
    return max(float(np.exp(2 * p.hyp[gp.D])) for p in gp.posteriors)


@pytest.mark.parametrize("name", ["viqr", "imiqr"])
def test_proposal_pdf_known_answers(golden, name):
    c = golden("is_known")
    gp = known_gp(c)
    mix = mixture_ref.Mixture.make(c["aspp_mu"], np.ones(2), np.ones(3), [0.7, 0.3])
    rect_delta = 2 * np.std(gp.X, ddof=1, axis=0)
    lw, fs2 = ais_host.proposal_pdf(c["Xa"], gp, mix, 0.5, rect_delta, name)
    assert lw.shape == c[f"aspp_{name}_ln_weights"].shape == (3, 2)
    assert np.max(np.abs(fs2 - c[f"aspp_{name}_f_s2"])) <= 1e-12 * sf2_max(gp)
    ref = c[f"aspp_{name}_ln_weights"]
    assert np.max(np.abs(lw - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-12


def test_fess_known_answers(golden):
    c = golden("is_known")
    gp = known_gp(c)
    mix = mixture_ref.Mixture.make(c["fess_mu"], c["fess_sigma"], np.ones(3), c["fess_w"])
    gp_means = np.arange(-5, 5).reshape((5, 2), order="F") * np.pi  # the input of oracle/make_golden.py is_known
    assert ais_host.fess(mix, gp_means, c["X"]) == pytest.approx(float(c["fess_means"]), rel=1e-12)
    assert ais_host.fess(mix, gp, c["Xa"]) == pytest.approx(float(c["fess_gp"]), rel=1e-12)


@pytest.mark.parametrize("cls", list(KINDS))
@pytest.mark.parametrize("name", GPCOV)
def test_full_function_vs_reference(golden, name, cls):
    c = golden("gpcov")
    gp, tag = gpcov_gp(c, name), f"{name}_{cls}"
    np.random.seed(11)
    with np.errstate(all="ignore"):
        out = ais_host.ais(gpcov_mix(c), gp, KINDS[cls], GPCOV_OPTS[cls])
    sf2 = sf2_max(gp)
    np.testing.assert_allclose(out["X"], c[f"{tag}_Xa"], rtol=1e-13, atol=0)
    assert np.max(np.abs(out["f_s2"] - c[f"{tag}_ais_f_s2"])) <= 1e-12
    assert np.max(np.abs(out["ln_weights"] - c[f"{tag}_ais_ln_weights"])) <= 1e-12
    assert out["K_Xa_X"].shape == (2, 48, 60) and out["C_tmp"].shape == (2, 60, 48)
    fs2_imp, cross = ais_host.implied(gp, out)
    assert np.max(np.abs(fs2_imp - c[f"{tag}_fs2_implied"])) <= 1e-12 * sf2
    assert np.max(np.abs(cross - c[f"{tag}_cross_implied"])) <= 1e-12 * sf2
    # the same state from the points alone (the entry the philox tests use)
    again = ais_host.from_points(gp, gpcov_mix(c), out["X"], KINDS[cls], 30, 18)
    for k in ("f_s2", "ln_weights", "K_Xa_X", "C_tmp"):
        # (one predict over all 48 rows instead of 30 + 18: BLAS blocks the products differently, so a few ulp)
        assert np.max(np.abs(again[k] - out[k])) <= 1e-13 * max(1.0, sf2), k


def test_mcmc_run_vs_reference(golden):
    c = golden("ais_mcmc")
    gp = gp_ref.make_gp(c["X"], c["y"], c["hyp"], gp_ref.MEAN_NEGQUAD)
    mix = mixture_ref.Mixture.make(c["vp_mu"], c["vp_sigma"], c["vp_lambd"], c["vp_w"])
    opts = ais_host.Opts({k: int(c[k]) for k in c if k.startswith("active_importance_sampling_")})
    np.random.seed(int(c["seed"]))
    with np.errstate(all="ignore"):
        out = ais_host.ais(mix, gp, ais_host.IMIQR, opts, sampler=ais_host.StandInSampler)
    assert out["X"].shape == (2, 12, 3) and out["f_s2"].shape == (12, 2) and out["ln_weights"].shape == (2, 12)
    np.testing.assert_allclose(out["X"], c["out_X"], rtol=1e-13, atol=0)
    assert np.max(np.abs(out["f_s2"] - c["out_f_s2"])) <= 1e-12
    assert np.max(np.abs(out["ln_weights"] - c["out_ln_weights"])) <= 1e-12
    sf2 = sf2_max(gp)
    ref = dict(K_Xa_X=c["out_K_Xa_X"], C_tmp=c["out_C_tmp"])
    for a, b in zip(ais_host.implied(gp, out), ais_host.implied(gp, ref)):
        assert np.max(np.abs(a - b)) <= 1e-12 * sf2
    assert float(np.min(c["choice_margin"])) >= 1e-6


# ------------------------------------------------------------------------------------------ the mirror, without a device
def _plain(c):
    from helpers import PlainGP, PlainVP

    return PlainVP(gpcov_mix(c)), PlainGP(gpcov_gp(c, "homo"))


def test_exports_and_small_functions():
    import pyvbmc_amd
    from pyvbmc_amd.active_importance_sampling import get_mcmc_opts, renormalize_weights

    for n in ("active_importance_sampling", "active_sample_proposal_pdf", "fess", "get_mcmc_opts", "renormalize_weights",
              "patch_active_sampling", "unpatch_active_sampling"):
        assert callable(getattr(pyvbmc_amd, n)) and n in pyvbmc_amd.__all__
    ln_w = np.log(np.array([[0.2, 1.5, 3.0], [0.7, 0.1, 2.5]]))
    r = renormalize_weights(ln_w)
    assert r.shape == ln_w.shape and abs(np.sum(np.exp(r)) - 1.0) < 1e-15
    np.testing.assert_allclose(r - ln_w, (r - ln_w)[0, 0], rtol=0, atol=1e-15)
    assert np.array_equal(r, ais_host.renormalize_weights(ln_w))
    assert get_mcmc_opts(12) == ({"display": "off", "diagnostics": False}, 1, 6)
    assert get_mcmc_opts(7, thin=3) == ({"display": "off", "diagnostics": False}, 3, 11)
    assert get_mcmc_opts(7, 2, 4)[1:] == (2, 4)


@pytest.mark.parametrize("bad", [0, -3, np.inf, np.nan])
def test_viqr_sample_count_must_be_positive(golden, bad):
    from pyvbmc_amd.acquisition import AcqFcnVIQR
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    vp, gp = _plain(golden("gpcov"))
    state = np.random.get_state()
    for opts in (ais_host.Opts(active_importance_sampling_mcmc_samples=bad), {"active_importance_sampling_mcmc_samples": bad}):
        with pytest.raises((ValueError, OverflowError), match="positive integer|cannot convert"):
            active_importance_sampling(vp, gp, AcqFcnVIQR(), opts)
    assert np.array_equal(np.random.get_state()[1], state[1])


def test_dict_option_strings_are_evaluated():
    from pyvbmc_amd.active_importance_sampling import _eval_option

    env = {"K": 3, "n_vars": 4, "D": 4}
    assert _eval_option({"k": "100 * (D + K)"}, "k", env) == 700
    assert _eval_option({"k": 48}, "k", env) == 48
    assert _eval_option(ais_host.Opts(k=5), "k", env) == 5


def test_smoothed_posterior_construction(golden):
    from pyvbmc_amd.active_importance_sampling import smoothed_posterior

    vp, _ = _plain(golden("gpcov"))
    state = np.random.get_state()
    sm = smoothed_posterior(vp)
    assert np.array_equal(np.random.get_state()[1], state[1])  # (built without the constructor's draw)
    ref = ais_host.smoothed(gpcov_mix(golden("gpcov")))
    assert sm.K == 4 * vp.K == ref.K and sm.D == vp.D
    assert sm.mu.shape == (vp.D, sm.K) and sm.sigma.shape == (1, sm.K) and sm.w.shape == (1, sm.K)
    assert np.array_equal(sm.mu, ref.mu) and np.array_equal(sm.sigma.ravel(), ref.sigma)
    assert np.array_equal(sm.w.ravel(), ref.w) and np.array_equal(sm.lambd.ravel(), ref.lambd)
    assert abs(sm.w.sum() - 1.0) < 1e-15
    for j, s in enumerate((0.0, 0.05, 0.2, 1.0)):
        np.testing.assert_allclose(sm.sigma[0, j * vp.K:(j + 1) * vp.K], np.sqrt(vp.sigma.ravel() ** 2 + s**2), rtol=1e-15)


def test_patch_active_sampling_on_a_fake_module(golden):
    import pyvbmc_amd
    from pyvbmc_amd import _lib
    from pyvbmc_amd.acquisition import AcqFcnIMIQR
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    calls = []

    def reference_fn(vp, gp, acq_fcn, options, **kw):
        calls.append(kw)
        return "reference result"

    mod = types.ModuleType("fake_active_sample")
    mod.active_importance_sampling = reference_fn
    assert pyvbmc_amd.patch_active_sampling(mod) is mod
    patched = mod.active_importance_sampling
    assert patched is not reference_fn and patched.__wrapped__ is active_importance_sampling
    pyvbmc_amd.patch_active_sampling(mod)  # idempotent: the saved callable is still the reference's
    # a shape the kernels refuse goes to the saved callable, the mirror-only keywords stripped, nothing drawn
    vp, gp = _plain(golden("gpcov"))
    gp.X = np.zeros((5, 33))
    opts = dict(active_importance_sampling_vp_samples=4, active_importance_sampling_box_samples=4,
                active_importance_sampling_mcmc_samples=0)
    state = np.random.get_state()
    with pytest.raises(_lib.UnsupportedShape):
        active_importance_sampling(vp, gp, AcqFcnIMIQR(), opts)
    out = mod.active_importance_sampling(vp, gp, AcqFcnIMIQR(), opts, rng="philox", seed=3, sampler=object, products=False)
    assert out == "reference result" and calls == [{}]
    assert np.array_equal(np.random.get_state()[1], state[1])
    pyvbmc_amd.unpatch_active_sampling(mod)
    assert mod.active_importance_sampling is reference_fn
    pyvbmc_amd.unpatch_active_sampling(mod)  # a second call changes nothing
    assert mod.active_importance_sampling is reference_fn
    # patch() itself leaves the name alone
    vo = types.ModuleType("fake_vo")
    vo.active_importance_sampling = reference_fn
    pyvbmc_amd.patch(vo)
    assert vo.active_importance_sampling is reference_fn
    pyvbmc_amd.unpatch(vo)
