#!/usr/bin/env python
"""Wall-clock milliseconds of the GP hyper-parameter fit as one device call (``GP.fit(optimizer="fused")``, vbmc_gp_fit)
next to the composition it joins, on the same device in the same process, the variants alternating.

    python tools/gp_fit_rows.py [--reps 3] [--warm 1] [--out profiles/gp_fit_rows.json]

Shapes N = 100 and N = 400 at D = 10, negative-quadratic mean (P = 33); the reference's default shape of a fit:
``init_N`` 1024, ``opts_N`` 1, 8 samples, thin 5, burn 15, ``tol_opt`` 1e-5; bounds around one point -+ 1.5 (noise from log
0.05), Student-t(3) priors on the length scales and the noise (tools/gp_opt_rows.py's case).  Per shape, medians over
--reps calls after --warm, with [min, max]:
  fused_ms      ``GP.fit(optimizer="fused", device=True)`` end to end, the posterior left installed;
  composed_ms   THE SAME WORK as separate calls with the host between them: the fused fit's own candidates scored by
                ``log_marginal_likelihood(device=True)`` plus the prior, ranked in NumPy, ``optimize_hyperparameters`` from
                the best, ``sample_hyperparameters`` from the optimum under the same seed, ``update(device=True)`` -- the
                same kernels on the same inputs (the samples are checked to be the fused call's, bit for bit);
  lockstep_ms   ``GP.fit(optimizer="lockstep", device=True)`` with the same options: the parent commit's route, whose Python
                and library code are unchanged.  Its design is NumPy's in the hard box, so its candidates, its optimiser's
                path and its chains differ from the fused call's: the same shape of work, not the same work;
  opt_ms, hyp_ms  ``vbmc_last_kernel_ms`` of the optimiser's and the chains' rounds inside one timed fused call (HIP events);
  new_share     1 - (opt_ms + hyp_ms) / that call's wall time: everything else -- the upload, the design, scoring 1027
                candidates, the rank, select and hand-over kernels, the build, the download."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pyvbmc_amd import _lib  # noqa: E402
from pyvbmc_amd import gp as gpm  # noqa: E402

SHAPES = ((100, 10), (400, 10))
OPTS = {"init_N": 1024, "opts_N": 1, "n_samples": 8, "thin": 5, "burn": 15, "tol_opt": 1e-5}
SEED = 2024


def make_case(N, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)) * 2.0
    y = (-0.5 * np.sum(X**2, axis=1) / D + 0.3 * rng.standard_normal(N)).reshape(-1, 1)
    h = np.concatenate([np.log(0.8 * np.sqrt(D) * (1 + 0.2 * rng.random(D))), [np.log(1.2)], [np.log(0.3)], [0.1],
                        0.1 * rng.standard_normal(D), np.log(2.0 + rng.random(D))])
    P = h.size
    lb, ub = h - 1.5, h + 1.5
    lb[D + 1] = np.log(0.05)
    pri = {k: np.full(P, np.nan) for k in ("mu", "sigma", "df")}
    pri["mu"][:D], pri["sigma"][:D], pri["df"][:D] = np.log(1.5), 1.0, 3.0
    pri["mu"][D + 1], pri["sigma"][D + 1], pri["df"][D + 1] = np.log(0.3), 0.5, 3.0
    return X, y, h + 0.1 * rng.standard_normal((3, P)), lb, ub, pri


def spread(t):
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def new_gp(ctx, X, y, lb, ub, pri):
    gp = gpm.GP(X.shape[1], gpm.SquaredExponential(), gpm.NegativeQuadratic(), gpm.GaussianNoise(constant_add=True))
    gp.ctx = ctx
    gp.X, gp.y = X, y
    gp.set_bounds({"lb": lb, "ub": ub})
    gp.set_priors(pri)
    return gp


def composed(gp, cand, lb, ub, pri, widths, ctx):
    score = gpm.log_marginal_likelihood(gp, cand, device=True, ctx=ctx) + gpm.hyper_log_prior(cand, pri)
    score, order = gpm.fit_rank(score)
    res = gpm.optimize_hyperparameters(gp, cand[order[:1]], lb=lb, ub=ub, priors=pri, tol_g=OPTS["tol_opt"], ctx=ctx)
    k, _ = gpm.fit_select(float(score[order[0]]), res["log_post"], np.zeros(1))
    best = res["hyp"][k] if k >= 0 else cand[order[0]]
    smp = gpm.sample_hyperparameters(gp, np.tile(best, (OPTS["n_samples"], 1)), lb=lb, ub=ub, widths=widths, priors=pri, n=1,
                                     thin=OPTS["thin"], burn_in=OPTS["burn"], seed=SEED, ctx=ctx)
    hyp = smp["samples"][:, 0, :]
    gp.update(hyp=hyp, device=True)
    return hyp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gp_fit_rows.json"))
    a = ap.parse_args()
    ctx = _lib.Context(0)
    _lib.set_default_context(ctx)
    rows = []
    for N, D in SHAPES:
        X, y, hyp0, lb, ub, pri = make_case(N, D, 100 + N)
        widths = (ub - lb) / 8
        t = {"fused": [], "composed": [], "lockstep": []}
        same = True
        for rep in range(a.warm + a.reps):
            for name in ("fused", "composed", "lockstep") if rep % 2 == 0 else ("lockstep", "composed", "fused"):
                gp = new_gp(ctx, X, y, lb, ub, pri)
                ctx.synchronize()
                t0 = time.perf_counter()
                if name == "composed":  # (the first pass runs the fused call first: its candidates exist by now)
                    hyp = composed(gp, cand, lb, ub, pri, widths, ctx)
                else:
                    hyp, opt, _ = gp.fit(hyp0=hyp0, options=OPTS, seed=SEED, optimizer=name)
                ctx.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                if name == "fused":
                    cand, fused_hyp, iters = opt["candidates"], hyp, opt["n_iterations"]
                if name == "composed":
                    same = same and np.array_equal(hyp, fused_hyp)
                if name == "lockstep":
                    lock_iters = opt["n_iterations"]
                if rep >= a.warm:
                    t[name].append(ms)
        ctx.set_timing(1)
        gp = new_gp(ctx, X, y, lb, ub, pri)
        t0 = time.perf_counter()
        gp.fit(hyp0=hyp0, options=OPTS, seed=SEED, optimizer="fused")
        wall = (time.perf_counter() - t0) * 1e3
        opt_ms, hyp_ms = ctx.last_kernel_ms(_lib.T_GP_OPT), ctx.last_kernel_ms(_lib.T_GP_HYP)
        ctx.set_timing(0)
        row = dict(N=N, D=D, P=int(lb.size), options=OPTS, fused_ms=spread(t["fused"]), composed_ms=spread(t["composed"]),
                   lockstep_ms=spread(t["lockstep"]), composed_equals_fused=bool(same), fused_iterations=int(iters),
                   lockstep_iterations=int(lock_iters), timed_call_ms=wall, opt_ms=opt_ms, hyp_ms=hyp_ms,
                   new_share=1.0 - (opt_ms + hyp_ms) / wall)
        rows.append(row)
        print(json.dumps(row), flush=True)
    Path(a.out).write_text(json.dumps(dict(device=str(ctx.device_info()), reps=a.reps, warm=a.warm, rows=rows), indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
