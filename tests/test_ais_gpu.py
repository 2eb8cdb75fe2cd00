"""GPU tests of pyvbmc_amd.active_importance_sampling (csrc/acq_is_prep.hip, vbmc_acq_is_build in csrc/api_acq_is.hip)
against the reference's recorded outputs (tests/golden/is_known.npz, gpcov.npz, ais_mcmc.npz) and against
tests/ais_host.py, the NumPy / SciPy restatement those fixtures pin on the CPU (tests/test_ais_host.py).

Bounds: f_s2 and the quantities implied by K_Xa_X / C_tmp at 1e-10 sf^2 (what the project holds predict and the same
product to, tests/test_acquisition.py), ln_weights at 1e-9, acquisition values at 1e-9, proposal points of the default
stream at rtol 1e-13.  C_tmp entry by entry has no bound of the project's: CTMP_REL_MEASURED below is the measured
max|C_tmp - C_tmp(SciPy solves)| / max|C_tmp| and the tests assert 10 x that figure (the explicit L^-1 route's error
grows with the conditioning of K + Sigma; the margin covers that).
"""
from types import SimpleNamespace

import numpy as np
import pytest

import ais_host
from helpers import PlainGP, PlainVP
from oracle import gp_ref, mixture_ref
from test_ais_host import GPCOV, GPCOV_OPTS, KINDS, gpcov_gp, gpcov_mix, known_gp, sf2_max

pytestmark = pytest.mark.gpu

# max |C_tmp(device) - C_tmp(ais_host)| / max |C_tmp| over the tile-edge and philox cases below, as measured on an
# MI355X by this file's own printed figures (recorded in profiles/ais_rows.json, rows "ctmp_rel_err_*"): 1.05e-13 at
# Na = 70, 1.27e-13 at Na = 129, 5.3e-14 with per-sample points; philox cases 6.6e-14 .. 1.05e-13
CTMP_REL_MEASURED = 1.27e-13


class CountingLib:
    """The library handle with the calls that install an importance state counted."""

    def __init__(self, lib):
        self._lib_real, self.n_set, self.n_build = lib, 0, 0

    def __getattr__(self, name):
        fn = getattr(self._lib_real, name)
        if name == "vbmc_acq_is_set":
            self.n_set += 1
        if name == "vbmc_acq_is_build":
            self.n_build += 1
        return fn


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


def mirror_acq(kind):
    from pyvbmc_amd.acquisition import AcqFcnIMIQR, AcqFcnVIQR

    return AcqFcnVIQR() if kind == ais_host.VIQR else AcqFcnIMIQR()


def plain_gp(ogp, rng_sn2=None):
    gp = PlainGP(ogp)
    length = np.exp(ogp.posteriors[0].hyp[: ogp.D])
    gp.temporary_data["X_rescaled"] = ogp.X / length
    gp.temporary_data["sn2_new"] = rng_sn2
    return gp, length


def optim_state(X, length, ais):
    return dict(integer_vars=None, lb_eps_orig=X.min(0) - 50.0, ub_eps_orig=X.max(0) + 50.0, gp_length_scale=length,
                variance_regularized_acq_fcn=False, active_importance_sampling=ais)


def nearest_sn2(Xs, X, length, sn2_new):
    d = ((Xs[:, None, :] / length - (X / length)[None, :, :]) ** 2).sum(-1)
    return sn2_new[np.argmin(d, axis=1)]


def ctmp_rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def check_state(out, host, ogp, what, lnw_tol=1e-9):
    """The mirror's dict against ais_host's for the same points: f_s2, ln_weights, implied quantities, C_tmp."""
    sf2 = sf2_max(ogp)
    assert out["f_s2"].shape == host["f_s2"].shape and out["ln_weights"].shape == host["ln_weights"].shape
    e_f = float(np.max(np.abs(out["f_s2"] - host["f_s2"])))
    fin = np.isfinite(host["ln_weights"])
    assert np.array_equal(fin, np.isfinite(out["ln_weights"]))
    e_w = float(np.max(np.abs(out["ln_weights"][fin] - host["ln_weights"][fin])))
    assert out["K_Xa_X"].shape == host["K_Xa_X"].shape and out["C_tmp"].shape == host["C_tmp"].shape
    e_k = float(np.max(np.abs(out["K_Xa_X"] - host["K_Xa_X"])))
    imp_d, imp_h = ais_host.implied(ogp, out), ais_host.implied(ogp, host)
    e_i = max(float(np.max(np.abs(a - b))) for a, b in zip(imp_d, imp_h))
    e_c = ctmp_rel(out["C_tmp"], host["C_tmp"])
    print(f"{what}: f_s2 {e_f / sf2:.2e} sf2, ln_w {e_w:.2e}, K {e_k / sf2:.2e} sf2, implied {e_i / sf2:.2e} sf2, "
          f"C_tmp rel {e_c:.2e}")
    assert e_f <= 1e-10 * sf2 and e_w <= lnw_tol and e_k <= 1e-10 * sf2 and e_i <= 1e-10 * sf2
    assert e_c <= 10 * CTMP_REL_MEASURED
    return e_c


# ------------------------------------------------------------------------------------------------ 1. known answers
@pytest.mark.parametrize("name", ["viqr", "imiqr"])
def test_proposal_pdf_known_answers(ctx, golden, name):
    from pyvbmc_amd.active_importance_sampling import active_sample_proposal_pdf

    c = golden("is_known")
    ogp = known_gp(c)
    gp = PlainGP(ogp)
    vp = PlainVP(mixture_ref.Mixture.make(c["aspp_mu"], np.ones(2), np.ones(3), [0.7, 0.3]))
    rect_delta = 2 * np.std(gp.X, ddof=1, axis=0)
    lw, fs2 = active_sample_proposal_pdf(c["Xa"], gp, vp, 0.5, rect_delta, mirror_acq(name))
    sf2 = sf2_max(ogp)
    ref = c[f"aspp_{name}_ln_weights"]
    assert lw.shape == ref.shape == (3, 2) and fs2.shape == (3, 2)
    e_f = float(np.max(np.abs(fs2 - c[f"aspp_{name}_f_s2"])))
    e_w = float(np.max(np.abs(lw - ref) / np.maximum(np.maximum(1.0, sf2), np.abs(ref))))
    print(f"aspp {name}: f_s2 {e_f / sf2:.2e} sf2, ln_w {e_w:.2e}")
    assert e_f <= 1e-10 * sf2 and e_w <= 1e-10


def test_fess_known_answers(ctx, golden):
    from pyvbmc_amd.active_importance_sampling import fess

    c = golden("is_known")
    gp = PlainGP(known_gp(c))
    vp = PlainVP(mixture_ref.Mixture.make(c["fess_mu"], c["fess_sigma"], np.ones(3), c["fess_w"]))
    gp_means = np.arange(-5, 5).reshape((5, 2), order="F") * np.pi
    assert fess(vp, gp_means, c["X"]) == pytest.approx(float(c["fess_means"]), rel=1e-9)
    assert fess(vp, gp, c["Xa"]) == pytest.approx(float(c["fess_gp"]), rel=1e-9)
    np.random.seed(3)
    assert 0.0 < fess(vp, gp, 40) <= 1.0  # a sample count: the points are drawn from vp


# ------------------------------------------------------------------------------------------------ 2. the full function
@pytest.mark.parametrize("cls", list(KINDS))
@pytest.mark.parametrize("name", GPCOV)
def test_full_function_vs_reference(ctx, golden, name, cls):
    from pyvbmc_amd.acquisition import _is_state_key
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    c = golden("gpcov")
    ogp, tag, kind = gpcov_gp(c, name), f"{name}_{cls}", KINDS[cls]
    gp, length = plain_gp(ogp, c[f"{name}_sn2_new"])
    vp = PlainVP(gpcov_mix(c))
    acq = mirror_acq(kind)
    flog = SimpleNamespace(y_max=float(np.max(c["y"])))
    sf2 = sf2_max(ogp)
    for products in ((True, False) if (name, kind) == ("homo", ais_host.IMIQR) else (True,)):
        np.random.seed(11)
        out = active_importance_sampling(vp, gp, acq, GPCOV_OPTS[cls], products=products)
        np.testing.assert_allclose(out["X"], c[f"{tag}_Xa"], rtol=1e-13, atol=0)
        e_f = float(np.max(np.abs(out["f_s2"] - c[f"{tag}_ais_f_s2"])))
        e_w = float(np.max(np.abs(out["ln_weights"] - c[f"{tag}_ais_ln_weights"])))
        assert e_f <= 1e-10 * sf2 and e_w <= 1e-9
        if products:
            assert out["K_Xa_X"].shape == (2, 48, 60) and out["C_tmp"].shape == (2, 60, 48)
            fs2_imp, cross = ais_host.implied(ogp, out)
            e_i = max(float(np.max(np.abs(fs2_imp - c[f"{tag}_fs2_implied"]))),
                      float(np.max(np.abs(cross - c[f"{tag}_cross_implied"]))))
            print(f"{tag}: f_s2 {e_f / sf2:.2e} sf2, ln_w {e_w:.2e}, implied {e_i / sf2:.2e} sf2")
            assert e_i <= 1e-10 * sf2
        else:
            assert "K_Xa_X" not in out and "C_tmp" not in out
        # the call left the state installed: the acquisition finds its key and uploads nothing
        assert ctx.__dict__["_acq_is_key"] == _is_state_key(out, ctx)[0]
        counting = CountingLib(ctx._lib)
        ctx._lib = counting
        try:
            v = acq(c["Xs"].copy(), gp, vp, flog, optim_state(c["X"], length, out))
        finally:
            ctx._lib = counting._lib_real
        assert counting.n_set == 0 and counting.n_build == 0
        err = float(np.max(np.abs(v - c[f"{tag}_acq"])))
        print(f"{tag} products={products}: max |acq - reference| = {err:.2e}")
        assert err < 1e-9


def test_products_false_dict_survives_a_displaced_state(ctx, golden):
    """A dict without products whose state another dict displaced is formed again on the device, not refused."""
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    c = golden("gpcov")
    ogp = gpcov_gp(c, "hetero")
    gp, length = plain_gp(ogp, c["hetero_sn2_new"])
    vp, acq = PlainVP(gpcov_mix(c)), mirror_acq(ais_host.IMIQR)
    flog = SimpleNamespace(y_max=0.0)
    np.random.seed(11)
    first = active_importance_sampling(vp, gp, acq, GPCOV_OPTS["AcqFcnIMIQR"], products=False)
    np.random.seed(12)
    active_importance_sampling(vp, gp, acq, GPCOV_OPTS["AcqFcnIMIQR"], products=False)  # displaces it
    v = acq(c["Xs"].copy(), gp, vp, flog, optim_state(c["X"], length, first))
    assert float(np.max(np.abs(v - c["hetero_AcqFcnIMIQR_acq"]))) < 1e-9


# ------------------------------------------------------------------------------------------------ 3. tile edges
def check_quantile_acq(acq, gp, vp, ogp, length, sn2_new, Xs, out, host, kind=ais_host.IMIQR):
    """The quantile acquisition over the installed state ``out`` at the points Xs against the host's over ``host``."""
    sn2 = nearest_sn2(Xs, ogp.X, length, sn2_new)
    with np.errstate(all="ignore"):
        ref = ais_host.quantile_acq(ogp, Xs, sn2, host, kind)
    v = acq(Xs.copy(), gp, vp, SimpleNamespace(y_max=0.0), optim_state(ogp.X, length, out))
    err = float(np.max(np.abs(v - ref)))
    print(f"acq at {Xs.shape[0]} points: max |device - host| = {err:.2e} (max |acq| {np.max(np.abs(ref)):.2f})")
    assert err <= 1e-9
    return err


@pytest.fixture(scope="module")
def larger():
    return ais_host.larger_case()


@pytest.mark.parametrize("n_vp,n_box,n_mcmc", [(40, 30, 0), (70, 59, 0), (40, 30, 70)])
def test_tile_edges_vs_host(ctx, larger, n_vp, n_box, n_mcmc):
    """Na = 70 and Na = 129 (N = 150: three column tiles of 64, the last of 22; Na: two tiles with 6 columns in the
    second, three tiles with one), and a run whose points are per sample, (S, 70, D), after the MCMC step.

    Measured max|C_tmp - C_tmp(SciPy)| / max|C_tmp| on an MI355X: 1.05e-13 (Na = 70), 1.27e-13 (Na = 129),
    5.3e-14 (per-sample points); asserted at 10 x the largest, 1.27e-12 (CTMP_REL_MEASURED)."""
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    ogp, mix, Xs, sn2_new = larger
    gp, length = plain_gp(ogp, sn2_new)
    vp, acq = PlainVP(mix), mirror_acq(ais_host.IMIQR)
    opts = ais_host.Opts(active_importance_sampling_vp_samples=n_vp, active_importance_sampling_box_samples=n_box,
                         active_importance_sampling_mcmc_samples=n_mcmc, active_importance_sampling_mcmc_thin=1)
    np.random.seed(7)
    out = active_importance_sampling(vp, gp, acq, opts, sampler=ais_host.StandInSampler)
    if n_mcmc:
        assert out["X"].shape == (3, n_mcmc, 4)
        np.random.seed(7)
        with np.errstate(all="ignore"):
            host = ais_host.ais(mix, ogp, ais_host.IMIQR, opts, sampler=ais_host.StandInSampler)
        np.testing.assert_allclose(out["X"], host["X"], rtol=1e-12, atol=0)
        host["K_Xa_X"], host["C_tmp"] = ais_host.products(ogp, out["X"])
    else:
        assert out["X"].shape == (n_vp + n_box, 4)
        with np.errstate(all="ignore"):
            host = ais_host.from_points(ogp, mix, out["X"], ais_host.IMIQR, n_vp, n_box)
    check_state(out, host, ogp, f"tile edges {n_vp}+{n_box} mcmc {n_mcmc}")
    check_quantile_acq(acq, gp, vp, ogp, length, sn2_new, Xs, out, host)


# ------------------------------------------------------------------------------------------------ 4. MCMC plumbing
def test_mcmc_run_vs_reference(ctx, golden):
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    c = golden("ais_mcmc")
    ogp = gp_ref.make_gp(c["X"], c["y"], c["hyp"], gp_ref.MEAN_NEGQUAD)
    gp, _ = plain_gp(ogp)
    vp = PlainVP(mixture_ref.Mixture.make(c["vp_mu"], c["vp_sigma"], c["vp_lambd"], c["vp_w"]))
    opts = {k: int(c[k]) for k in c if k.startswith("active_importance_sampling_")}  # a plain dict
    np.random.seed(int(c["seed"]))
    out = active_importance_sampling(vp, gp, mirror_acq(ais_host.IMIQR), opts, sampler=ais_host.StandInSampler)
    assert out["X"].shape == (2, 12, 3) and out["f_s2"].shape == (12, 2) and out["ln_weights"].shape == (2, 12)
    assert out["K_Xa_X"].shape == (2, 12, 60) and out["C_tmp"].shape == (2, 60, 12)
    sf2 = sf2_max(ogp)
    np.testing.assert_allclose(out["X"], c["out_X"], rtol=1e-12, atol=0)
    e_w = float(np.max(np.abs(out["ln_weights"] - c["out_ln_weights"])))
    e_f = float(np.max(np.abs(out["f_s2"] - c["out_f_s2"])))
    ref = dict(K_Xa_X=c["out_K_Xa_X"], C_tmp=c["out_C_tmp"])
    e_i = max(float(np.max(np.abs(a - b))) for a, b in zip(ais_host.implied(ogp, out), ais_host.implied(ogp, ref)))
    print(f"mcmc: ln_w {e_w:.2e}, f_s2 {e_f / sf2:.2e} sf2, implied {e_i / sf2:.2e} sf2")
    assert e_w <= 1e-9 and e_f <= 1e-10 * sf2 and e_i <= 1e-10 * sf2


def test_mcmc_without_gpyreg_names_the_missing_sampler(ctx, golden, monkeypatch):
    import sys

    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    monkeypatch.setitem(sys.modules, "gpyreg", None)  # (importing it raises ImportError, installed or not)
    monkeypatch.setitem(sys.modules, "gpyreg.slice_sample", None)
    c = golden("ais_mcmc")
    gp, _ = plain_gp(gp_ref.make_gp(c["X"], c["y"], c["hyp"], gp_ref.MEAN_NEGQUAD))
    vp = PlainVP(mixture_ref.Mixture.make(c["vp_mu"], c["vp_sigma"], c["vp_lambd"], c["vp_w"]))
    opts = {k: int(c[k]) for k in c if k.startswith("active_importance_sampling_")}
    with pytest.raises(ImportError, match="SliceSampler"):
        active_importance_sampling(vp, gp, mirror_acq(ais_host.IMIQR), opts)


def test_viqr_fess_mcmc_branch_vs_host(ctx, larger):
    """Step 0 with the acquisition's ``mcmc_importance_sampling`` flag (:80-108): a fESS threshold above 1 always takes
    the MCMC pass (all samples handed to the sampler, the last Na kept), one of 0 never does."""
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    ogp, mix, _, sn2_new = larger
    gp, _ = plain_gp(ogp, sn2_new)
    vp, acq = PlainVP(mix), mirror_acq(ais_host.VIQR)
    acq.acq_info["mcmc_importance_sampling"] = True
    outs = {}
    for thresh in (1.5, 0.0):
        opts = ais_host.Opts(active_importance_sampling_mcmc_samples=40, active_importance_sampling_mcmc_thin=2,
                             active_importance_sampling_fess_thresh=thresh)
        np.random.seed(13)
        out = active_importance_sampling(vp, gp, acq, opts, sampler=ais_host.StandInSampler)
        np.random.seed(13)
        host = ais_host.ais(mix, ogp, ais_host.VIQR, opts, sampler=ais_host.StandInSampler, mcmc_importance_sampling=True)
        assert out["X"].shape == (40, 4)
        np.testing.assert_allclose(out["X"], host["X"], rtol=1e-12, atol=0)
        check_state(out, host, ogp, f"viqr fess thresh {thresh}")
        outs[thresh] = out["X"]
    assert not np.array_equal(outs[1.5], outs[0.0])  # the MCMC pass moved the points


# ------------------------------------------------------------------------------------------------ 5. philox
def check_philox_imiqr(ogp, mix, sn2_new, n_vp, n_box, what="philox"):
    """The Philox route of the IMIQR importance state on a GP and mixture: reproducible, NumPy's stream untouched, the box
    draws near training points, and the state against the host's at the device's points."""
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    gp, _ = plain_gp(ogp, sn2_new)
    vp, acq = PlainVP(mix), mirror_acq(ais_host.IMIQR)
    opts = dict(active_importance_sampling_vp_samples=n_vp, active_importance_sampling_box_samples=n_box,
                active_importance_sampling_mcmc_samples=0)
    state = np.random.get_state()
    a = active_importance_sampling(vp, gp, acq, opts, rng="philox", seed=5)
    b = active_importance_sampling(vp, gp, acq, opts, rng="philox", seed=5)
    assert np.array_equal(np.random.get_state()[1], state[1])  # a given seed: np.random is not consumed
    for k in ("X", "f_s2", "ln_weights", "K_Xa_X", "C_tmp"):
        assert np.array_equal(a[k], b[k]), k
    other = active_importance_sampling(vp, gp, acq, opts, rng="philox", seed=6, products=False)
    assert not np.array_equal(other["X"], a["X"])
    assert a["X"].shape == (n_vp + n_box, ogp.D) and np.all(np.isfinite(a["X"]))
    if n_box:
        rect_delta = 2 * np.std(ogp.X, ddof=1, axis=0)
        box = a["X"][n_vp:]
        near = np.all(np.abs(box[:, None, :] - ogp.X[None, :, :]) <= rect_delta, axis=2).any(axis=1)
        assert near.all()
        for d in range(ogp.D):
            assert len(np.unique(box[:, d])) == n_box  # distinct draws, in every dimension
        assert not np.any(np.all(box[:, None, :] == ogp.X[None, :, :], axis=2))  # ... off the training points
    with np.errstate(all="ignore"):
        host = ais_host.from_points(ogp, mix, a["X"], ais_host.IMIQR, n_vp, n_box)
    return check_state(a, host, ogp, f"{what} {n_vp}+{n_box}")


@pytest.mark.parametrize("n_vp,n_box", [(30, 18), (0, 20), (20, 0)])
def test_philox_imiqr(ctx, larger, n_vp, n_box):
    ogp, mix, _, sn2_new = larger
    check_philox_imiqr(ogp, mix, sn2_new, n_vp, n_box)


def test_philox_viqr_and_env_default(ctx, larger, monkeypatch):
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling

    ogp, mix, _, sn2_new = larger
    gp, _ = plain_gp(ogp, sn2_new)
    vp, acq = PlainVP(mix), mirror_acq(ais_host.VIQR)
    opts = ais_host.Opts(active_importance_sampling_mcmc_samples=65)
    a = active_importance_sampling(vp, gp, acq, opts, rng="philox", seed=9)
    monkeypatch.setenv("VBMC_HIP_RNG", "philox")
    b = active_importance_sampling(vp, gp, acq, opts, seed=9)
    assert a["X"].shape == (65, 4) and np.array_equal(a["X"], b["X"]) and np.array_equal(a["C_tmp"], b["C_tmp"])
    host = ais_host.from_points(ogp, mix, a["X"], ais_host.VIQR)
    check_state(a, host, ogp, "philox viqr")
    with pytest.raises(ValueError, match="unknown rng"):
        active_importance_sampling(vp, gp, acq, opts, rng="mt")


# ------------------------------------------------------------------------------------------------ 6. contracts
def test_point_outside_every_box_is_invalid(ctx, golden):
    from pyvbmc_amd.active_importance_sampling import active_sample_proposal_pdf

    c = golden("gpcov")
    gp = PlainGP(gpcov_gp(c, "homo"))
    rect_delta = 2 * np.std(gp.X, ddof=1, axis=0)
    Xa = np.vstack([gp.X[:2] + 0.1, gp.X.max(0) + 3 * rect_delta])
    with pytest.raises(ValueError, match="Invalid value."):
        active_sample_proposal_pdf(Xa, gp, None, 0, rect_delta, mirror_acq(ais_host.IMIQR))
    lw, _ = active_sample_proposal_pdf(Xa[:2], gp, None, 0, rect_delta, mirror_acq(ais_host.IMIQR))
    assert np.all(np.isfinite(lw))


def test_unsupported_dimension_is_refused_before_any_draw(ctx, golden):
    from pyvbmc_amd import _lib
    from pyvbmc_amd.active_importance_sampling import active_importance_sampling, active_sample_proposal_pdf

    rng = np.random.default_rng(2)
    D, N = 33, 40
    X = rng.standard_normal((N, D))
    y = -0.5 * np.sum(X**2, axis=1, keepdims=True)
    hyp = np.concatenate([np.zeros(D), [0.5], [np.log(0.1)], [0.0], np.zeros(D), np.zeros(D)])
    gp = PlainGP(gp_ref.make_gp(X, y, hyp, gp_ref.MEAN_NEGQUAD))
    vp = PlainVP(mixture_ref.Mixture.make(rng.standard_normal((D, 2)), [0.5, 0.7], np.ones(D), [0.5, 0.5]))
    before_key = ctx.__dict__.get("_acq_is_key")
    for kind, opts in ((ais_host.VIQR, GPCOV_OPTS["AcqFcnVIQR"]), (ais_host.IMIQR, GPCOV_OPTS["AcqFcnIMIQR"])):
        for rng_mode in ("numpy", "philox"):
            np.random.seed(4)
            state = np.random.get_state()
            with pytest.raises(_lib.UnsupportedShape):
                active_importance_sampling(vp, gp, mirror_acq(kind), opts, rng=rng_mode)
            after = np.random.get_state()
            assert np.array_equal(after[1], state[1]) and after[2:] == state[2:]
    with pytest.raises(_lib.UnsupportedShape):
        active_sample_proposal_pdf(X[:3], gp, vp, 0.5, np.ones(D), mirror_acq(ais_host.IMIQR))
    assert ctx.__dict__.get("_acq_is_key") == before_key
