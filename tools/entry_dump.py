#!/usr/bin/env python
"""Outputs of the entry points that list their device scratch through csrc/scratch.h and are not in tools/gp_dense_dump.py
-- the sampler and its consumers (kl_div, moments, mtv, mode), the transformer, pdf_orig, kde_1d, the importance-sampling
preparation and its MCMC step, neg_elcbo_batch, the device-built GP posterior and its append, GP hyper-parameter sampling and
optimisation, the batched log marginal likelihood, the acquisition search's evaluation of a resident set and its CMA-ES refinement -- for a fixed list of small
cases, written to an .npz: run once per library (VBMC_HIP_LIB names the one to load, as in tools/ab_libs.sh) and compare.
    VBMC_HIP_LIB=$PWD/variants/libvbmc_parent.so python tools/entry_dump.py parent.npz
    python tools/entry_dump.py new.npz
    python tools/entry_dump.py --compare parent.npz new.npz      # np.array_equal per array; exit status 1 on a mismatch
Fixed seeds, device draws from Philox.  The shapes are the smallest at which a piece of a layout can move: an odd count of
int32 labels in front of the selector, a second mixture with more components than the first (the selector is sized by the
larger), P = D and P > D in the moments' partial sums, optional pieces present and absent."""
import ctypes as C
import itertools
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.adam_traj_dump import compare  # noqa: E402
from tools.gp_dense_dump import make_gp  # noqa: E402


def mixture(rng, D, K):
    """(mu K x D, sigma, lambd, w, eta) of a random mixture"""
    eta = rng.standard_normal(K)
    w = np.exp(eta) / np.sum(np.exp(eta))
    return [np.ascontiguousarray(a, dtype=np.float64)
            for a in (rng.standard_normal((K, D)), 0.4 + 0.5 * rng.random(K), 0.7 + 0.6 * rng.random(D), w, eta)]


def main(out):
    from pyvbmc_amd import _lib
    from pyvbmc_amd.gp import upload_gp

    ctx = _lib.Context(0)
    L, h, p, f64 = ctx._lib, ctx._h, _lib.ptr, _lib.f64
    rng = np.random.default_rng(2026)
    res = {}

    def set_mixture(m, D, K):
        ctx.check(L.vbmc_set_mixture(h, D, K, *[p(a) for a in m]))

    def set_transformer(slot, D, shift):
        # unbounded, logit and (D = 3) probit dimensions, centred
        types = f64([0.0, 3.0, 12.0][:D])
        lb, ub = f64([-np.inf, -3.0, -4.0][:D]), f64([np.inf, 4.0, 5.0][:D])
        mu, delta = f64(np.full(D, 0.1 + shift)), f64(np.full(D, 1.2 - shift))
        ctx.check(L.vbmc_set_transformer(h, slot, D, p(types), p(lb), p(ub), p(mu), p(delta), None, None))
        return lb, ub

    D, K, K2 = 3, 2, 3
    m1, m2 = mixture(rng, D, K), mixture(rng, D, K2)
    set_mixture(m1, D, K)
    set_transformer(0, D, 0.0)
    set_transformer(1, D, 0.3)
    # ---- vbmc_mixture_sample / _t / _orig
    for N, lab, bal in itertools.product((5, 257), (0, 1), (0, 1)):
        for name, df in (("sample", None), ("sample_t", 4.0), ("sample_orig", np.inf)):
            x, c = np.empty((N, D)), np.empty(N, dtype=np.int32)
            cp = c.ctypes.data_as(C.POINTER(C.c_int32)) if lab else None
            if df is None:
                ctx.check(L.vbmc_mixture_sample(h, N, 11, bal, p(x), cp))
            else:
                ctx.check(getattr(L, "vbmc_mixture_" + name)(h, N, 11, bal, df, p(x), cp))
            tag = f"{name}/N{N}_l{lab}_b{bal}"
            res[tag + "/x"] = x
            if lab:
                res[tag + "/comp"] = c
        if lab:  # labels alone
            c = np.empty(N, dtype=np.int32)
            ctx.check(L.vbmc_mixture_sample(h, N, 11, bal, None, c.ctypes.data_as(C.POINTER(C.c_int32))))
            res[f"sample/N{N}_b{bal}/comp_only"] = c
    # ---- vbmc_kl_div_mc / _orig: K = 2 against K2 = 3
    for name in ("vbmc_kl_div_mc", "vbmc_kl_div_mc_orig"):
        kl = np.empty(2)
        ctx.check(getattr(L, name)(h, 300, 5, K2, *[p(a) for a in m2[:4]], p(kl)))
        res[name] = kl
    # ---- vbmc_mixture_moments_orig: D = 3 (P = 6 > D) here, D = 1 (P = D) below
    for cov in (0, 1):
        mean, cv = np.empty(D), np.zeros((D, D))
        ctx.check(L.vbmc_mixture_moments_orig(h, 300, 9, cov, p(mean), p(cv) if cov else None))
        res[f"moments/D{D}_c{cov}/mean"], res[f"moments/D{D}_c{cov}/cov"] = mean, cv
    # ---- vbmc_transform
    xin = f64(rng.random((5, D)) * [2.0, 6.0, 8.0] + [-1.0, -2.9, -3.9])
    for d in (0, 1, 2):
        o = np.empty(5 if d == 2 else (5, D))
        ctx.check(L.vbmc_transform(h, 5, d, p(xin), p(o)))
        res[f"transform/d{d}"] = o
    # ---- vbmc_mixture_pdf_orig (a gradient with the log is refused: three flag pairs)
    for lg, gr in ((0, 0), (1, 0), (0, 1)):
        y, dy = np.empty(5), np.zeros((5, D))
        ctx.check(L.vbmc_mixture_pdf_orig(h, 5, p(xin), lg, gr, np.inf, p(y), p(dy) if gr else None))
        res[f"pdf_orig/l{lg}_g{gr}/y"], res[f"pdf_orig/l{lg}_g{gr}/dy"] = y, dy
    # ---- vbmc_mixture_mode: uploaded candidates and Philox, both spaces
    R, n = 2, 300
    cand = f64(rng.standard_normal((R, n, D)))
    for orig, up in itertools.product((0, 1), (0, 1)):
        x, fo, rec, pts, ys = np.empty(D), C.c_double(), np.empty((R, 5)), np.empty((R, D)), np.empty((R, D))
        ctx.check(L.vbmc_mixture_mode(h, R, orig, n, p(cand) if up else None, 21, 50, 1e-9, p(x), C.byref(fo), p(rec), p(pts),
                                      p(ys)))
        for k, v in zip(("x", "f", "rec", "pts", "ys"), (x, np.array(fo.value), rec, pts, ys)):
            res[f"mode/o{orig}_u{up}/{k}"] = v
    # ---- the entry points on a GP of N = 65, D = 3, S = 2, one sample non-Cholesky
    N, S = 65, 2
    gp = make_gp(ctx, rng, N, D, S)
    upload_gp(gp, ctx)
    rect = f64(0.3 + 0.2 * rng.random(D))
    Na = 70
    Xa = f64(rng.standard_normal((Na, D)))
    for fmu_flag in (0, 1):
        lnw, fs2, inv = np.empty((Na, S)), np.empty((Na, S)), C.c_int(0)
        ctx.check(L.vbmc_is_proposal(h, Na, p(Xa), K2, *[p(a) for a in m2[:4]], 0.5, p(rect), fmu_flag, p(lnw), p(fs2),
                                     C.byref(inv)))
        res[f"is_proposal/f{fmu_flag}/lnw"], res[f"is_proposal/f{fmu_flag}/fs2"] = lnw, fs2
        res[f"is_proposal/f{fmu_flag}/invalid"] = np.array(inv.value)
    xb = np.empty((70, D))
    ctx.check(L.vbmc_is_box_sample(h, 70, 31, p(rect), p(xb)))
    res["is_box_sample"] = xb
    fs2a, lnwa = f64(0.5 + rng.random((Na, S))), f64(rng.standard_normal((S, Na)))
    Ko, Co = np.empty((S, Na, N)), np.empty((S, N, Na))
    ctx.check(L.vbmc_acq_is_build(h, Na, p(Xa), 0, p(fs2a), p(lnwa), p(Ko), p(Co)))
    res["acq_is_build/K"], res["acq_is_build/C"] = Ko, Co
    xs, sn2 = f64(rng.standard_normal((7, D))), f64(0.01 + rng.random(7))
    acq, vt = np.empty(7), np.empty(7)
    ctx.check(L.vbmc_acq_is_eval(h, 7, p(xs), p(sn2), C.c_double(0.6744897501960817), p(acq), p(vt)))
    res["acq_is_build/eval_acq"], res["acq_is_build/eval_var_tot"] = acq, vt
    nk = 3
    x0, wd = f64(0.3 * rng.standard_normal((S, D))), f64(np.full(D, 1.5))
    lb, ub = f64(np.full(D, -4.0)), f64(np.full(D, 4.0))
    for fmu_flag in (0, 1):
        X, lp, fm, fv = np.empty((S, nk, D)), np.empty((S, nk)), np.empty((nk, S)), np.empty((nk, S))
        st, inv = np.zeros((S, 4), dtype=np.int64), C.c_int(0)
        ctx.check(L.vbmc_is_mcmc(h, fmu_flag, 0.6744897501960817, p(x0), p(wd), p(lb), p(ub), nk, 1, 2, 77, p(X), p(lp), p(fm),
                                 p(fv), st.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(inv)))
        for k, v in zip(("X", "logp", "fmu", "fs2", "stats", "invalid"), (X, lp, fm, fv, st, np.array(inv.value))):
            res[f"is_mcmc/f{fmu_flag}/{k}"] = v
    # ---- vbmc_neg_elcbo_batch: B = 3, every block optimised, with and without bounds
    B, n_theta = 3, D * K + K + D + K
    th = f64(np.concatenate([m1[0].ravel(), np.log(m1[1]), np.log(m1[2]), m1[4]])[None, :] + 0.1 * rng.standard_normal((B, n_theta)))
    n_bnd = D * K + D * K + K
    blb, bub = f64(np.full(n_bnd, -0.5)), f64(np.full(n_bnd, 0.5))
    for bnd in (0, 1):
        opts = _lib.ElboOpts()
        opts.ns_per_comp, opts.compute_grad, opts.optimize_mask = 0, 0, 15
        if bnd:
            opts.bnd_lb, opts.bnd_ub, opts.n_bnd, opts.tol_con = p(blb), p(bub), n_bnd, 1e-3
            opts.weight_threshold, opts.weight_penalty = 0.3, 0.1
        F, G, H = np.empty(B), np.empty(B), np.empty(B)
        ctx.check(L.vbmc_neg_elcbo_batch(h, p(th), B, n_theta, C.byref(opts), p(F), p(G), p(H)))
        res[f"elcbo_batch/b{bnd}/F"], res[f"elcbo_batch/b{bnd}/G"], res[f"elcbo_batch/b{bnd}/H"] = F, G, H
    # ---- vbmc_gp_posterior -> vbmc_gp_append -> vbmc_gp_fetch: N = 65 -> 66, S = 2, constant noise (all Cholesky)
    X = f64(rng.standard_normal((N, D)))
    y = f64(-0.5 * np.sum(X**2, axis=1) / D + 0.05 * rng.standard_normal(N))
    sn2_div = f64([0.0025, 0.01])
    sn2 = f64(np.repeat(sn2_div[:, None], N, axis=1))
    hyp = f64([np.concatenate([np.log((0.8 + 0.3 * rng.random(D)) * 0.5), [np.log(2.0)], [np.log(0.05)], [0.1]]) for _ in range(S)])
    al, Lm = np.empty((S, N)), np.empty((S, N, N))
    ctx.check(L.vbmc_gp_posterior(h, N, D, S, D + 3, _lib.MEAN_CONST, p(X), p(y), p(sn2), p(sn2_div), p(hyp), p(al), p(Lm)))
    res["gp_post/alpha"], res["gp_post/L"] = al, Lm
    al1, L1 = np.empty((S, N + 1)), np.empty((S, N + 1, N + 1))
    ctx.check(L.vbmc_gp_append(h, p(f64(rng.standard_normal(D))), 0.2, p(al1), p(L1)))
    res["gp_post/append_alpha"], res["gp_post/append_L"] = al1, L1
    al2, L2 = np.empty((S, N + 1)), np.empty((S, N + 1, N + 1))
    ctx.check(L.vbmc_gp_fetch(h, p(al2), p(L2)))
    res["gp_post/fetch_alpha"], res["gp_post/fetch_L"] = al2, L2
    # ---- vbmc_kde_1d: 2 columns, one-sided bounds (the lower ones alone, then the upper ones alone)
    xk = f64(np.abs(rng.standard_normal((2, 100))))
    for side, klb, kub in (("lb", f64([-0.5, -0.2]), None), ("ub", None, f64([6.0, 7.0]))):
        dens, xm, bw, info = np.empty((2, 16)), np.empty((2, 16)), np.empty(2), np.zeros((2, 2), dtype=np.int64)
        ctx.check(L.vbmc_kde_1d(h, 2, 100, p(xk), 16, p(klb), p(kub), p(dens), p(xm), p(bw),
                                info.ctypes.data_as(C.POINTER(C.c_int64))))
        for k, v in zip(("density", "xmesh", "bandwidth", "info"), (dens, xm, bw, info)):
            res[f"kde_1d/{side}/{k}"] = v
    # ---- D = 1: moments with P = D
    set_mixture(mixture(rng, 1, K), 1, K)
    set_transformer(0, 1, 0.0)
    for cov in (0, 1):
        mean, cv = np.empty(1), np.zeros((1, 1))
        ctx.check(L.vbmc_mixture_moments_orig(h, 300, 9, cov, p(mean), p(cv) if cov else None))
        res[f"moments/D1_c{cov}/mean"], res[f"moments/D1_c{cov}/cov"] = mean, cv
    # ---- vbmc_mtv, D = 2: host samples on both sides; both sides drawn on the device, K2 = 3 > K = 2
    D = 2
    m1, m2 = mixture(rng, D, K), mixture(rng, D, K2)
    set_mixture(m1, D, K)
    tlb, tub = set_transformer(0, D, 0.0)
    set_transformer(1, D, 0.3)
    hs = [f64(rng.random((200, D)) * [2.0, 6.0] + [-1.0, -2.9]) for _ in range(2)]
    for dev in (0, 1):
        sides = []
        for s in range(2):
            sd = _lib.MtvSide()
            sd.source, sd.n, sd.seed = (_lib.MTV_MIX1 + s, 300, 41 + s) if dev else (_lib.MTV_HOST, 200, 0)
            sd.x_NxD, sd.lb_D, sd.ub_D = (None if dev else p(hs[s])), p(tlb), p(tub)
            sides.append(sd)
        mtv, info = np.empty(D), np.zeros((2 * D, 2), dtype=np.int64)
        ctx.check(L.vbmc_mtv(h, D, C.byref(sides[0]), C.byref(sides[1]), K2, *[p(a) for a in m2[:4]], p(mtv),
                             info.ctypes.data_as(C.POINTER(C.c_int64))))
        res[f"mtv/dev{dev}/mtv"], res[f"mtv/dev{dev}/info"] = mtv, info
    # ---- vbmc_gp_hyp_sample: N = 65, D = 3, constant mean, 3 chains of 2 kept samples (a generator of its own: the rows
    # above keep their inputs)
    r2 = np.random.default_rng(2024)
    N, D, Cn, nk = 65, 3, 3, 2
    X = f64(r2.standard_normal((N, D)) * 2.0)
    y = f64(-0.5 * np.sum(X**2, axis=1) / D + 0.3 * r2.standard_normal(N))
    h0 = np.concatenate([np.log(1.4 * np.ones(D)), [np.log(1.2)], [np.log(0.3)], [0.1]])
    P = h0.size
    x0 = f64(h0 + 0.1 * r2.standard_normal((Cn, P)))
    lb, ub, wd = f64(h0 - 1.5), f64(h0 + 1.5), f64(np.full(P, 0.6))
    pmu, psg, pdf = f64(np.full(P, np.log(1.5))), f64(np.full(P, np.nan)), f64(np.full(P, 3.0))
    psg[:D], psg[D + 1], pdf[D + 1] = 1.0, 0.5, np.inf
    smp, lpo, lpr = np.empty((Cn, nk, P)), np.empty((Cn, nk)), np.empty((Cn, nk))
    st, inv = np.zeros((Cn, 4), dtype=np.int64), np.zeros(Cn, dtype=np.int32)
    ctx.check(L.vbmc_gp_hyp_sample(h, N, D, P, _lib.MEAN_CONST, p(X), p(y), None, Cn, p(x0), p(wd), p(lb), p(ub), p(pmu),
                                   p(psg), p(pdf), nk, 2, 1, C.c_uint64(77), p(smp), p(lpo), p(lpr),
                                   st.ctypes.data_as(C.POINTER(C.c_int64)), inv.ctypes.data_as(C.POINTER(C.c_int32))))
    for k, v in zip(("samples", "log_post", "log_priors", "stats", "invalid"), (smp, lpo, lpr, st, inv)):
        res[f"gp_hyp_sample/{k}"] = v
    # ---- vbmc_gp_hyp_optimize on the same data: 3 starts, 6 iterations of 3 pairs, traced; once more in chunks of 2
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    mi, mh, cap = 6, 3, 7
    for chunk in (0, 2):
        ctx.set_option("gp_lml_chunk", chunk)
        ho, lpo, go = np.zeros((Cn, P)), np.zeros(Cn), np.zeros((Cn, P))
        st, inv = np.zeros((Cn, 4), dtype=np.int64), np.zeros(Cn, dtype=np.int32)
        tit, tev = np.zeros((Cn, cap, 3 * P + 3)), np.zeros((Cn, 1 + 31 * cap, 4))
        ctx.check(L.vbmc_gp_hyp_optimize(h, N, D, P, _lib.MEAN_CONST, p(X), p(y), None, Cn, p(x0), p(lb), p(ub), p(pmu), p(psg),
                                         p(pdf), mi, mh, 1e-5, 1e-9, cap, p(ho), p(lpo), p(go), st.ctypes.data_as(i64p),
                                         inv.ctypes.data_as(i32p), p(tit), p(tev)))
        for k, v in zip(("hyp", "log_post", "grad", "stats", "invalid", "trace_iter", "trace_eval"),
                        (ho, lpo, go, st, inv, tit, tev)):
            res[f"gp_hyp_optimize/c{chunk}/{k}"] = v
    # ---- vbmc_gp_lml on the same data: B = 3 (the starts; the third row's sf^2 overflows, a candidate that does not
    # factorise), value alone and with the gradient, then in chunks of 2
    hb = f64(x0)
    hb[2, D] = 400.0
    e = np.exp(2.0 * hb[:, D + 1])
    sn2b, divb, dsb = f64(np.repeat(e[:, None], N, axis=1)), f64(e), f64(2.0 * e)
    for tag, chunk, gr in (("v", 0, 0), ("g", 0, 1), ("g_c2", 2, 1)):
        ctx.set_option("gp_lml_chunk", chunk)
        lm, dl, stt = np.empty(Cn), np.zeros((Cn, P)), np.zeros(Cn, dtype=np.int32)
        ctx.check(L.vbmc_gp_lml(h, N, D, Cn, P, _lib.MEAN_CONST, p(X), p(y), p(sn2b), p(divb), p(dsb), p(hb), gr, p(lm),
                                p(dl) if gr else None, stt.ctypes.data_as(i32p)))
        lm[np.isneginf(lm)] = -12345.0  # (a fixed stand-in, as for the search's NaN: np.array_equal could not compare NaN)
        dl[np.isnan(dl)] = -12345.0
        res[f"gp_lml/{tag}/lml"], res[f"gp_lml/{tag}/dlml"], res[f"gp_lml/{tag}/status"] = lm, dl, stt
    ctx.set_option("gp_lml_chunk", 0)
    # ---- vbmc_search_put / vbmc_search_eval on 300 resident points, every kind; then vbmc_search_cmaes, whose scoring
    # is the same code (a library from before that entry point: the search arrays alone)
    r3 = np.random.default_rng(2025)
    D, K, N, S, M = 3, 2, 65, 2, 300
    set_mixture(mixture(r3, D, K), D, K)
    set_transformer(0, D, 0.0)
    upload_gp(make_gp(ctx, r3, N, D, S), ctx)
    Xs = f64(0.8 * r3.standard_normal((M, D)))
    ell, Xr, sn2n = f64(0.8 + 0.3 * r3.random(D)), f64(r3.standard_normal((N, D))), f64(0.01 + r3.random(N))
    lbe, ube = f64([-np.inf, -2.5, -3.5]), f64([np.inf, 3.5, 4.5])
    Na = 40
    Xa, fs2a = f64(r3.standard_normal((Na, D))), f64(0.5 + r3.random((Na, S)))
    ctx.check(L.vbmc_acq_is_build(h, Na, p(Xa), 0, p(fs2a), None, None, None))
    ctx.check(L.vbmc_search_put(h, M, D, p(Xs), 1 << 1, 1))
    for kind in range(5):
        for tol in (0.0, 0.05):
            noisy = kind >= 3
            acq, order, Xo = np.empty(M), np.empty(M, dtype=np.int64), np.empty((M, D))
            ctx.check(L.vbmc_search_eval(h, kind, 0.3, tol, 0.6744897501960817, N if noisy else 0, p(Xr) if noisy else None,
                                         p(sn2n) if noisy else None, p(ell) if noisy else None, 1, p(lbe), p(ube), p(acq),
                                         order.ctypes.data_as(C.POINTER(C.c_int64)), p(Xo)))
            acq[np.isnan(acq)] = -12345.0  # (np.array_equal could not compare NaN)
            for k, v in zip(("acq", "order", "X_sorted"), (acq, order, Xo)):
                res[f"search/k{kind}_t{tol}/{k}"] = v
    if hasattr(L, "vbmc_search_cmaes"):
        R = 3
        x0 = f64(0.3 * r3.standard_normal((R, D)))
        for kind in (1, 3, 4):
            noisy = kind >= 3
            opts = _lib.CmaesOpts(0, 1 + 7 * 12, 1e-2, 0.0, 99)
            o = [np.empty((R, D)), np.empty(R), np.empty(R), np.empty((R, D)), np.empty(R), np.empty((R, D, D))]
            st = np.zeros((R, 4), dtype=np.int64)
            ctx.check(L.vbmc_search_cmaes(h, kind, 0.3, 0.0, 0.6744897501960817, N if noisy else 0, p(Xr) if noisy else None,
                                          p(sn2n) if noisy else None, p(ell) if noisy else None, 1, p(lbe), p(ube), R, p(x0),
                                          p(f64(np.full(R, 0.5))), p(f64(np.full(D, -2.0))), p(f64(np.full(D, 2.0))), 1 << 1,
                                          C.byref(opts), *[p(a) for a in o], st.ctypes.data_as(C.POINTER(C.c_int64))))
            for k, v in zip(("x_best", "f_best", "f0", "mean", "sigma", "C", "stats"), o + [st]):
                res[f"search_cmaes/k{kind}/{k}"] = v
    ctx.close()
    nans = sorted(k for k, v in res.items() if np.asarray(v).dtype.kind == "f" and np.isnan(v).any())
    assert not nans, f"NaN in {nans}: np.array_equal could not compare them"
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    np.savez(out, **res)
    print(f"{out}: {len(res)} arrays from {_lib.LIB_PATH}")


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main(sys.argv[1])
