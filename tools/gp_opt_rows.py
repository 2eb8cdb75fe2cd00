#!/usr/bin/env python
"""Wall-clock milliseconds of GP hyper-parameter optimisation on the device (lockstep quasi-Newton runs,
vbmc_gp_hyp_optimize), next to what ``GP.fit`` did before it: SciPy L-BFGS-B from the same starts one after the other,
every objective call one ``log_marginal_likelihood(device=True)`` batch of one candidate.

    python tools/gp_opt_rows.py [--reps 3] [--warm 1] [--out profiles/gp_opt_rows.json]

Shapes (N, D) = (400, 10), (800, 20), negative-quadratic mean, R = 1, 2, 8 and 32 starts around one point; bounds start
-+ 1.5 (noise from log 0.05), Student-t(3) priors on the length scales and the noise (tools/gp_hyp_rows.py's case);
``max_iter`` 200, 8 pairs, ``tol_g`` 1e-5, ``tol_f`` 1e-9 -- the defaults.  Per row (shape, R), medians over --reps
calls after --warm, with [min, max]:
  call_ms        ``optimize_hyperparameters(device=True)`` end to end;
  rounds         the largest evaluation count of a run plus the advance that consumes the last one (the host reads the
                 count of unfinished runs every 4 rounds, so up to 3 more are queued);
  rounds_ms      ``vbmc_last_kernel_ms(T_GP_OPT)``, the call's rounds between HIP events (a timed call of its own);
  ms_per_round   call_ms / rounds;
  evaluations, iterations, stop reasons, best_log_post: of the runs.
``scipy_*``: ``GP.fit(hyp0=starts, options={"opts_N": R, "tol_opt": 1e-5}, optimizer="scipy", device=True)`` on the same
starts, one call: its wall time (candidate scoring and the final posterior included), its number of value+gradient
objective calls, ``n_iterations`` and the log posterior it ends at.  That route's Python and the library code under it
are what the parent commit has, unchanged.  Every shape runs in a fresh child process under ``timeout -k 10 <--limit>``;
after a child that does not exit with 0 nothing further is started and the tool exits with that status."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pyvbmc_amd import _lib  # noqa: E402
from pyvbmc_amd import gp as gpm  # noqa: E402

SHAPES = ((400, 10), (800, 20))
RUNS = (1, 2, 8, 32)


def make_case(N, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)) * 2.0
    y = (-0.5 * np.sum(X**2, axis=1) / D + 0.3 * rng.standard_normal(N)).reshape(-1, 1)
    h = np.concatenate([np.log(0.8 * np.sqrt(D) * (1 + 0.2 * rng.random(D))), [np.log(1.2)], [np.log(0.3)], [0.1],
                        0.1 * rng.standard_normal(D), np.log(2.0 + rng.random(D))])
    P = h.size
    x0 = h + 0.1 * rng.standard_normal((max(RUNS), P))
    lb, ub = h - 1.5, h + 1.5
    lb[D + 1] = np.log(0.05)
    pri = {k: np.full(P, np.nan) for k in ("mu", "sigma", "df")}
    pri["mu"][:D], pri["sigma"][:D], pri["df"][:D] = np.log(1.5), 1.0, 3.0
    pri["mu"][D + 1], pri["sigma"][D + 1], pri["df"][D + 1] = np.log(0.3), 0.5, 3.0
    return X, y, x0, lb, ub, pri


def spread(t):
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def make_gp(ctx, X, y, D, lb, ub, pri):
    gp = gpm.GP(D, gpm.SquaredExponential(), gpm.NegativeQuadratic(), gpm.GaussianNoise(constant_add=True))
    gp.ctx = ctx
    gp.X, gp.y = X, y
    gp.set_bounds({"lb": lb, "ub": ub})
    gp.set_priors(pri)
    return gp


def child(N, D, reps, warm):
    ctx = _lib.Context(0)
    _lib.set_default_context(ctx)
    X, y, x0, lb, ub, pri = make_case(N, D, 7)
    rows = []
    for R in RUNS:
        gp = make_gp(ctx, X, y, D, lb, ub, pri)
        t, ev, out = [], [], None
        for i in range(warm + reps):
            t0 = time.perf_counter()
            out = gpm.optimize_hyperparameters(gp, x0[:R], lb=lb, ub=ub, priors=pri, ctx=ctx)
            if i >= warm:
                t.append(1e3 * (time.perf_counter() - t0))
        ctx.set_timing(1)
        for _ in range(reps):
            gpm.optimize_hyperparameters(gp, x0[:R], lb=lb, ub=ub, priors=pri, ctx=ctx)
            ev.append(ctx.last_kernel_ms(_lib.T_GP_OPT))
        ctx.set_timing(0)
        rounds = int(np.max(out["stats"][:, 1])) + 1
        row = dict(N=N, D=D, R=R, call_ms=spread(t), rounds=rounds, rounds_ms=spread(ev),
                   ms_per_round=statistics.median(t) / rounds, evaluations=out["stats"][:, 1].tolist(),
                   iterations=out["stats"][:, 0].tolist(), stop_reasons=out["stats"][:, 3].tolist(),
                   best_log_post=float(np.max(out["log_post"])))
        # the scipy route of GP.fit on the same starts, its objective calls counted
        calls = [0]
        real = gpm.log_marginal_likelihood

        def counting(*a, **kw):
            calls[0] += 1 if kw.get("grad") else 0
            return real(*a, **kw)

        gp = make_gp(ctx, X, y, D, lb, ub, pri)
        gpm.log_marginal_likelihood = counting
        try:
            t0 = time.perf_counter()
            _, opt, _ = gp.fit(X, y, None, hyp0=x0[:R], options={"opts_N": R, "tol_opt": 1e-5}, device=True, optimizer="scipy")
            row["scipy_fit_ms"] = 1e3 * (time.perf_counter() - t0)
        finally:
            gpm.log_marginal_likelihood = real
        row.update(scipy_objective_calls=calls[0], scipy_iterations=int(opt["n_iterations"]), scipy_log_post=float(opt["log_post"]))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    ctx.close()
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--limit", type=int, default=280)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gp_opt_rows.json"))
    ap.add_argument("--child", nargs=2, type=int)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.reps, a.warm)
    rows = []
    for N, D in SHAPES:
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, __file__, "--child", str(N), str(D),
                            "--reps", str(a.reps), "--warm", str(a.warm)], stdout=subprocess.PIPE)
        if p.returncode != 0:
            print(f"shape ({N}, {D}) exited with {p.returncode}: nothing further is started", file=sys.stderr)
            return p.returncode
        rows += json.loads(p.stdout.decode().strip().splitlines()[-1])
    doc = {"tool": "tools/gp_opt_rows.py", "reps": a.reps, "warm": a.warm, "device": "MI355X (gfx950)",
           "scipy_route": "GP.fit(optimizer='scipy', device=True): Python and library code unchanged from the parent commit",
           "rows": rows}
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    for r in rows:
        print(f"N={r['N']} D={r['D']} R={r['R']}: call {r['call_ms']['median']:.1f} ms, {r['rounds']} rounds, "
              f"{r['ms_per_round']:.3f} ms/round; scipy fit {r['scipy_fit_ms']:.1f} ms, {r['scipy_objective_calls']} calls")
    return 0


if __name__ == "__main__":
    sys.exit(main())
