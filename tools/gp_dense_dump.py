#!/usr/bin/env python
"""Outputs of the dense GP entry points -- vbmc_gp_predict, the variance of vbmc_gp_log_joint, vbmc_sq_dist, vbmc_acq_eval,
vbmc_acq_is_set / _eval -- for a fixed list of small ragged cases, written to an .npz: run once per library
(VBMC_HIP_LIB names the one to load, as in tools/ab_libs.sh) and compare.
    VBMC_HIP_LIB=$PWD/variants/libvbmc_parent.so python tools/gp_dense_dump.py parent.npz
    python tools/gp_dense_dump.py new.npz
    python tools/gp_dense_dump.py --compare parent.npz new.npz      # np.array_equal per array; exit status 1 on a mismatch
The cases are the smallest shapes at which the shared pieces (csrc/mfma_tile.h, csrc/gp_dev.h, PredictPlan) can go wrong:
N = 65 (a second column tile of one column), one and two row tiles and the <= 32-point kernel, D padded to 4, Cholesky
and non-Cholesky samples, the three mean kinds, both finishes of predict, ties of sq_dist inside and across tiles, the
polled and the copy path of acq_eval with more than 64 components, the rectangular panel product of acq_is_eval."""
import ctypes as C
import itertools
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.adam_traj_dump import compare  # noqa: E402

NOISE = {1: [0.05], 2: [0.05, 3e-4], 3: [0.05, 3e-4, 0.1]}  # sn per GP sample; 3e-4 makes a non-Cholesky sample


def ell_scale(D):
    """Length scales that leave K + sn2 I of the 65 standard-normal points well conditioned (<= 1e5 for D >= 2) while
    K* keeps sizeable entries: on a non-Cholesky sample the reference's own variance K*' (K + sn2 I)^-1 K* carries
    cond x 1e-16, which has to stay far inside the 1e-10 bound."""
    return np.sqrt(D) * (0.3 if D < 8 else 1.0)


def make_gp(ctx, rng, N, D, S, mean="NegativeQuadratic"):
    from pyvbmc_amd import gp as gpm

    X = rng.standard_normal((N, D))
    y = -0.5 * np.sum(X**2, axis=1) / D + 0.05 * rng.standard_normal(N)
    hm = {"ZeroMean": [], "ConstantMean": [0.1], "NegativeQuadratic": [0.1] + [0.0] * D + [np.log(np.sqrt(D))] * D}[mean]
    hyp = np.array([np.concatenate([np.log((0.8 + 0.3 * rng.random(D)) * ell_scale(D)), [np.log(2.0)], [np.log(sn)], hm])
                    for sn in NOISE[S]])
    gp = gpm.GP(D, gpm.SquaredExponential(), getattr(gpm, mean)(), gpm.GaussianNoise(constant_add=True))
    gp.ctx = ctx
    gp.update(X_new=X, y_new=y, hyp=hyp)
    return gp


def make_vp(ctx, rng, D, K):
    from pyvbmc_amd import VariationalPosterior

    vp = VariationalPosterior(D, K)
    vp.mu = rng.standard_normal((D, K))
    vp.sigma = (0.4 + 0.5 * rng.random(K)).reshape(1, -1)
    vp.lambd = (0.7 + 0.6 * rng.random(D)).reshape(-1, 1)
    vp.eta = rng.standard_normal(K).reshape(1, -1)
    vp.w = np.exp(vp.eta) / np.sum(np.exp(vp.eta))
    vp.ctx = ctx
    return vp


def main(out):
    from pyvbmc_amd import _lib, acquisition
    from pyvbmc_amd.variational_optimization import _gp_log_joint

    ctx = _lib.Context(0)
    rng = np.random.default_rng(2025)
    res = {}
    N = 65
    # ---- vbmc_gp_predict
    for D, S in itertools.product((1, 3, 5, 32), (1, 2)):
        for mean in (("ZeroMean", "ConstantMean", "NegativeQuadratic") if D == 3 else ("NegativeQuadratic",)):
            gp = make_gp(ctx, rng, N, D, S, mean)
            for M in (1, 33, 70):
                xs = rng.standard_normal((M, D))
                for noise, sep, fused in itertools.product((0, 1), (0, 1), (0, 2)):
                    ctx.set_option("predict_fused", fused)
                    fmu, fs2 = gp.predict(xs, add_noise=bool(noise), separate_samples=bool(sep))
                    tag = f"predict/D{D}_S{S}_{mean}_M{M}_n{noise}_s{sep}_f{fused}"
                    res[tag + "/fmu"], res[tag + "/fs2"] = fmu, fs2
    ctx.set_option("predict_fused", 1)
    # ---- the variance of the expected log joint (the panel product's Cout path): K = 3, both sample kinds
    gp, vp = make_gp(ctx, rng, N, 3, 2), make_vp(ctx, rng, 3, 3)
    r = _gp_log_joint(vp, gp, False, avg_flag=False, compute_var=True, separate_K=True)
    for name, v in zip(("G", "varG", "I_sk", "J_sjk"), (r[0], r[2], r[5], r[6])):
        res[f"logjoint/{name}"] = np.asarray(v)
    # ---- vbmc_sq_dist: ties inside a tile (63, 64 straddle two tiles; 10, 100 are two tiles apart)
    for n, m, D in itertools.product((1, 65), (1, 130), (1, 5, 32)):
        a, b = rng.standard_normal((n, D)), rng.standard_normal((m, D))
        if m > 100:
            b[64], b[100] = b[63], b[10]
            a[0] = b[63]
            a[-1] = b[10]
        tag = f"sqdist/n{n}_m{m}_D{D}"
        res[tag + "/c"], res[tag + "/idx"] = acquisition.sq_dist(a, b, ctx=ctx, return_argmin=True)
        res[tag + "/c_only"] = acquisition.sq_dist(a, b, ctx=ctx)
        res[tag + "/idx_only"] = acquisition.nearest_neighbour(a, b, ctx=ctx)
    # ---- vbmc_acq_eval: the four kinds, polled path (M = 1, 5) and copy path (M = 300), two components per lane at K = 70
    for D, K, S in itertools.product((2, 5), (1, 70), (1, 3)):
        gp, vp = make_gp(ctx, rng, N, D, S), make_vp(ctx, rng, D, K)
        acquisition.upload_vp(vp, ctx)
        acquisition.upload_gp(gp, ctx)
        for M in (1, 5, 300):
            xs = _lib.f64(1.2 * rng.standard_normal((M, D)))
            sn2 = _lib.f64(0.01 + rng.random(M))
            _, fs2 = gp.predict(xs)
            tol = float(np.median(fs2)) if M > 1 else 0.0  # some variances below it
            for kind in range(4):
                acq, f_bar, var_tot = np.empty(M), np.empty(M), np.empty(M)
                ctx.check(ctx._lib.vbmc_acq_eval(ctx._h, M, _lib.ptr(xs), kind, 0.3, tol, _lib.ptr(sn2), _lib.ptr(acq),
                                                 _lib.ptr(f_bar), _lib.ptr(var_tot)))
                tag = f"acq/D{D}_K{K}_S{S}_M{M}_k{kind}"
                res[tag + "/acq"], res[tag + "/f_bar"], res[tag + "/var_tot"] = acq, f_bar, var_tot
    # ---- vbmc_acq_is_set / _eval: VIQR (no weights) and IMIQR, S = 2 with one non-Cholesky sample
    D, S = 3, 2
    gp = make_gp(ctx, rng, N, D, S)
    acquisition.upload_gp(gp, ctx)
    for Na, M, lnw in itertools.product((1, 65), (3, 70), (False, True)):
        ctmp = _lib.f64(0.1 * rng.standard_normal((S, N, Na)))
        Xa, fs2a = _lib.f64(rng.standard_normal((Na, D))), _lib.f64(0.5 + rng.random((Na, S)))
        w = _lib.f64(rng.standard_normal((S, Na))) if lnw else None
        ctx.check(ctx._lib.vbmc_acq_is_set(ctx._h, Na, _lib.ptr(Xa), 0, _lib.ptr(ctmp), _lib.ptr(fs2a), _lib.ptr(w)))
        xs, sn2 = _lib.f64(rng.standard_normal((M, D))), _lib.f64(0.01 + rng.random(M))
        acq, var_tot = np.empty(M), np.empty(M)
        ctx.check(ctx._lib.vbmc_acq_is_eval(ctx._h, M, _lib.ptr(xs), _lib.ptr(sn2), C.c_double(0.6744897501960817),
                                            _lib.ptr(acq), _lib.ptr(var_tot)))
        res[f"acqis/Na{Na}_M{M}_w{int(lnw)}/acq"], res[f"acqis/Na{Na}_M{M}_w{int(lnw)}/var_tot"] = acq, var_tot
    ctx.close()
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    np.savez(out, **res)
    print(f"{out}: {len(res)} arrays from {_lib.LIB_PATH}")


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main(sys.argv[1])
