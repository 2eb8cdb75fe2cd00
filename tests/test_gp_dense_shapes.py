"""The dense GP entry points at the ragged shapes where the shared 64 x 64 tile (csrc/mfma_tile.h), predict's finish and
sample moments (csrc/gp_dev.h) and the batch plan can go wrong, against the oracle: N = 65 (a second column tile of one
column), one and two row tiles and the <= 32-point kernel, D padded to 4, a non-Cholesky sample, the three mean kinds,
both finishes of predict; sq_dist ties inside and across tiles; acq_eval's polled and copy path with more than 64
mixture components; acq_is_eval's rectangular panel product.  Tolerances are those of tests/test_acquisition.py."""
from types import SimpleNamespace

import numpy as np
import pytest
from helpers import PlainGP, PlainVP
from test_acquisition import KINDS, close

from oracle import acq_ref, gp_ref, mixture_ref

pytestmark = pytest.mark.gpu
N = 65
NOISE = {1: [0.05], 2: [0.05, 3e-4], 3: [0.05, 3e-4, 0.1]}  # sn per GP sample; 3e-4 makes a non-Cholesky sample
MEANS = {"ZeroMean": gp_ref.MEAN_ZERO, "ConstantMean": gp_ref.MEAN_CONST, "NegativeQuadratic": gp_ref.MEAN_NEGQUAD}


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


def ell_scale(D):
    """Length scales that leave K + sn2 I of the 65 standard-normal points well conditioned (<= 1e5 for D >= 2) while
    K* keeps sizeable entries: on a non-Cholesky sample the reference's own variance K*' (K + sn2 I)^-1 K* carries
    cond x 1e-16, which has to stay far inside the 1e-10 bound."""
    return np.sqrt(D) * (0.3 if D < 8 else 1.0)


def make_gp(rng, D, S, mean="NegativeQuadratic"):
    X = rng.standard_normal((N, D))
    y = -0.5 * np.sum(X**2, axis=1) / D + 0.05 * rng.standard_normal(N)
    hm = {"ZeroMean": [], "ConstantMean": [0.1], "NegativeQuadratic": [0.1] + [0.0] * D + [np.log(np.sqrt(D))] * D}[mean]
    hyp = np.array([np.concatenate([np.log((0.8 + 0.3 * rng.random(D)) * ell_scale(D)), [np.log(2.0)], [np.log(sn)], hm])
                    for sn in NOISE[S]])
    ogp = gp_ref.make_gp(X, y, hyp, MEANS[mean])
    assert [p.L_chol for p in ogp.posteriors] == [sn > 1e-3 for sn in NOISE[S]]
    return ogp, PlainGP(ogp, mean)


def make_mix(rng, D, K):
    eta = rng.standard_normal(K)
    return mixture_ref.Mixture.make(rng.standard_normal((D, K)), 0.4 + 0.5 * rng.random(K), 0.7 + 0.6 * rng.random(D),
                                    np.exp(eta) / np.sum(np.exp(eta)), eta)


def device_predict(ctx, gp, xs, add_noise, separate):
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gp import upload_gp

    upload_gp(gp, ctx)
    xs = _lib.f64(xs)
    shape = (xs.shape[0], len(gp.posteriors) if separate else 1)
    fmu, fs2 = np.empty(shape), np.empty(shape)
    ctx.check(ctx._lib.vbmc_gp_predict(ctx._h, xs.shape[0], _lib.ptr(xs), int(add_noise), int(separate), _lib.ptr(fmu),
                                       _lib.ptr(fs2)))
    return fmu, fs2


@pytest.mark.parametrize("D,S,mean", [(1, 1, "NegativeQuadratic"), (3, 2, "ZeroMean"), (3, 2, "ConstantMean"),
                                      (5, 2, "NegativeQuadratic"), (32, 1, "NegativeQuadratic")])
def test_predict_ragged(ctx, D, S, mean):
    rng = np.random.default_rng(100 + D)
    ogp, gp = make_gp(rng, D, S, mean)
    sf2 = float(np.exp(2 * ogp.posteriors[0].hyp[D]))
    for M in (1, 33, 70):
        xs = rng.standard_normal((M, D))
        for noise in (False, True):
            for sep in (False, True):
                omu, os2 = gp_ref.predict(ogp, xs, add_noise=noise, separate_samples=sep)
                for fused in (0, 2):
                    ctx.set_option("predict_fused", fused)
                    fmu, fs2 = device_predict(ctx, gp, xs, noise, sep)
                    assert fmu.shape == omu.shape and fs2.shape == os2.shape
                    assert np.max(np.abs(fmu - omu)) <= 1e-10 * max(1.0, np.max(np.abs(omu)))
                    assert np.max(np.abs(fs2 - os2)) <= 1e-10 * max(1.0, sf2)
    ctx.set_option("predict_fused", 1)


def test_sq_dist_ragged_and_ties(ctx):
    from pyvbmc_amd.acquisition import nearest_neighbour, sq_dist

    rng = np.random.default_rng(7)
    for n in (1, 65):
        for m in (1, 130):
            for D in (1, 5, 32):
                a, b = rng.standard_normal((n, D)), rng.standard_normal((m, D))
                if m > 100:  # identical rows of b at columns 63 | 64 (two tiles) and 10, 100: np.argmin keeps the first
                    b[64], b[100] = b[63], b[10]
                    a[0] = b[63]
                    a[-1] = b[10]
                ref = acq_ref.sq_dist(a, b)
                c, idx = sq_dist(a, b, ctx=ctx, return_argmin=True)
                assert np.max(np.abs(c - ref)) < 1e-12 * max(1.0, ref.max())
                assert np.all(c >= 0.0)
                assert np.array_equal(idx, np.argmin(c, axis=1))
                if m > 100:
                    assert idx[-1] == 10 and (n == 1 or idx[0] == 63)
                assert np.array_equal(sq_dist(a, b, ctx=ctx), c)
                assert np.array_equal(nearest_neighbour(a, b, ctx=ctx), idx)


@pytest.mark.parametrize("D,K,S", [(2, 1, 1), (2, 70, 3), (5, 70, 1), (5, 1, 3)])
def test_acq_eval_small_and_copy_path(ctx, D, K, S):
    from pyvbmc_amd import acquisition

    rng = np.random.default_rng(10 * D + K + S)
    ogp, gp = make_gp(rng, D, S)
    mix = make_mix(rng, D, K)
    vp = PlainVP(mix)
    length = np.exp(ogp.posteriors[0].hyp[:D])
    gp.temporary_data["X_rescaled"] = ogp.X / length
    gp.temporary_data["sn2_new"] = 0.01 + rng.random(N)
    flog = SimpleNamespace(y_max=float(np.max(ogp.y)))
    for M in (1, 5, 300):  # polled completion up to 256 points, copies beyond
        Xs = 1.2 * rng.standard_normal((M, D))
        _, v = gp_ref.predict(ogp, Xs)
        state = dict(integer_vars=None, lb_eps_orig=np.full(D, -50.0), ub_eps_orig=np.full(D, 50.0), gp_length_scale=length,
                     variance_regularized_acq_fcn=True, tol_gp_var=float(np.median(v)))  # some variances below it
        for cls, kind in KINDS.items():
            with np.errstate(all="ignore"):
                ref = acq_ref.acq_call(kind, Xs.copy(), ogp, mix, flog.y_max, state, X_rescaled=ogp.X / length,
                                       sn2_new=gp.temporary_data["sn2_new"])
            close(getattr(acquisition, cls)()(Xs.copy(), gp, vp, flog, state), ref, 1e-8)


def test_acq_is_eval_ragged(ctx):
    from pyvbmc_amd.acquisition import AcqFcnIMIQR, AcqFcnVIQR
    from scipy.stats import norm

    rng = np.random.default_rng(31)
    D, S = 3, 2
    ogp, gp = make_gp(rng, D, S)
    vp = PlainVP(make_mix(rng, D, 2))
    length = np.exp(ogp.posteriors[0].hyp[:D])
    gp.temporary_data["X_rescaled"] = ogp.X / length
    gp.temporary_data["sn2_new"] = 0.01 + rng.random(N)
    flog = SimpleNamespace(y_max=0.0)
    base = dict(integer_vars=None, lb_eps_orig=np.full(D, -50.0), ub_eps_orig=np.full(D, 50.0), gp_length_scale=length,
                variance_regularized_acq_fcn=False)
    for Na in (1, 65):
        Xa = rng.standard_normal((Na, D))
        _, fs2a = gp_ref.predict(ogp, Xa, separate_samples=True)
        K_Xa_X = np.stack([gp_ref.se_ard(p.hyp[: D + 1], Xa, ogp.X) for p in ogp.posteriors])
        for M in (3, 70):
            Xs = 1.3 * rng.standard_normal((M, D))
            d = ((Xs[:, None, :] / length - (ogp.X / length)[None, :, :]) ** 2).sum(-1)
            sn2 = gp.temporary_data["sn2_new"][np.argmin(d, axis=1)]
            for cls, usew in ((AcqFcnVIQR, False), (AcqFcnIMIQR, True)):
                ais = dict(X=Xa, f_s2=fs2a, ln_weights=rng.standard_normal((S, Na)), K_Xa_X=K_Xa_X)
                ref = acq_ref.quantile_acq(ogp, Xs, sn2, ais, norm.ppf(0.75), usew)
                v = cls()(Xs.copy(), gp, vp, flog, dict(base, active_importance_sampling=ais))
                assert np.max(np.abs(v - ref)) < 1e-9 * max(1.0, np.max(np.abs(ref)))
