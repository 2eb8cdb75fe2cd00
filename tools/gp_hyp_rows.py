#!/usr/bin/env python
"""Wall-clock milliseconds of GP hyper-parameter sampling on the device (lockstep slice chains, vbmc_gp_hyp_sample), next
to what a user had before it: the same chain run by the host sampler with one ``log_marginal_likelihood(device=True)``
call of B = 1 per evaluation.

    python tools/gp_hyp_rows.py [--reps 3] [--warm 1] [--out profiles/gp_hyp_rows.json]

Shapes (N, D) = (100, 5), (400, 10), (800, 20), negative-quadratic mean, C = 1, 8 and 32 chains of n = 1, thin = 5,
burn_in = 5 from starts around one point; bounds start -+ 1.5 (noise from log 0.05), widths 0.6, Student-t(3) priors on
the length scales and the noise.  Per row (shape, C), medians over --reps calls after --warm, with [min, max]:
  call_ms         ``sample_hyperparameters(device=True)`` end to end;
  rounds          the largest evaluation count of a chain plus the advance that consumes the last value (the host reads
                  the count of unfinished chains every 4 rounds, so up to 3 more are queued);
  rounds_ms       ``vbmc_last_kernel_ms(T_GP_HYP)``, the call's rounds between HIP events (a timed call of its own);
  ms_per_round    call_ms / rounds;  ms_per_eval_per_chain  call_ms / (rounds C).
Per shape, ``baseline_*``: chain 0 alone run by the host sampler (``pyvbmc_amd.gp._slice_chain``) over
``log_marginal_likelihood(device=True)`` with B = 1 plus the prior -- every evaluation uploads X, y again and
synchronises; the library code under it is unchanged from the parent commit.  It runs one chain because its chains run
one after the other: C chains cost C times as much.  ``baseline_ms_per_eval`` is the figure to hold against
``ms_per_round`` (one round evaluates all C chains).  At the smallest shape also ``numpy_*``: the same chain with
``device=False``.  Every shape runs in a fresh child process under ``timeout -k 10 <--limit>``; after a child that does
not exit with 0 nothing further is started and the tool exits with that status."""
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

SHAPES = ((100, 5), (400, 10), (800, 20))
CHAINS = (1, 8, 32)
N_KEEP, THIN, BURN = 1, 5, 5


def make_case(N, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)) * 2.0
    y = (-0.5 * np.sum(X**2, axis=1) / D + 0.3 * rng.standard_normal(N)).reshape(-1, 1)
    h = np.concatenate([np.log(0.8 * np.sqrt(D) * (1 + 0.2 * rng.random(D))), [np.log(1.2)], [np.log(0.3)], [0.1],
                        0.1 * rng.standard_normal(D), np.log(2.0 + rng.random(D))])
    P = h.size
    x0 = h + 0.1 * rng.standard_normal((max(CHAINS), P))
    lb, ub = h - 1.5, h + 1.5
    lb[D + 1] = np.log(0.05)
    pri = {k: np.full(P, np.nan) for k in ("mu", "sigma", "df")}
    pri["mu"][:D], pri["sigma"][:D], pri["df"][:D] = np.log(1.5), 1.0, 3.0
    pri["mu"][D + 1], pri["sigma"][D + 1], pri["df"][D + 1] = np.log(0.3), 0.5, 3.0
    return X, y, x0, lb, ub, np.full(P, 0.6), pri


def spread(t):
    return round(statistics.median(t), 3), [round(min(t), 3), round(max(t), 3)]


def run_shape(N, D, reps, warm):
    ctx = _lib.Context(0)
    _lib.set_default_context(ctx)
    X, y, x0, lb, ub, widths, pri = make_case(N, D, 100 + N)
    gp = gpm.GP(D, gpm.SquaredExponential(), gpm.NegativeQuadratic(), gpm.GaussianNoise(constant_add=True))
    gp.ctx = ctx
    gp.X, gp.y = X, y
    kw = dict(lb=lb, ub=ub, widths=widths, priors=pri, n=N_KEEP, thin=THIN, burn_in=BURN, seed=5)
    for Cn in CHAINS:
        t, ev, out = [], [], None
        for i in range(warm + reps):
            t0 = time.perf_counter()
            out = gpm.sample_hyperparameters(gp, x0[:Cn], ctx=ctx, **kw)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= warm:
                t.append(dt)
        ctx.set_timing(1)
        gpm.sample_hyperparameters(gp, x0[:Cn], ctx=ctx, **kw)
        ev.append(ctx.last_kernel_ms(_lib.T_GP_HYP))
        ctx.set_timing(0)
        rounds = int(out["stats"][:, 0].max()) + 1
        row = {"row": f"N{N}_D{D}_C{Cn}", "reps": reps, "warm": warm, "rounds": rounds,
               "evaluations_per_chain": [int(out["stats"][:, 0].min()), int(out["stats"][:, 0].max())]}
        row["call_ms"], row["call_min_max_ms"] = spread(t)
        row["rounds_ms"] = round(ev[0], 3)
        row["ms_per_round"] = round(row["call_ms"] / rounds, 4)
        row["ms_per_eval_per_chain"] = round(row["call_ms"] / rounds / Cn, 4)
        print(json.dumps(row), flush=True)

    # the baseline: chain 0 on the host, one B = 1 device call per evaluation
    def log_p(h):
        return float(gpm.log_marginal_likelihood(gp, h[None, :], ctx=ctx)[0]) + gpm.hyper_log_prior(h, pri)

    t, stats = [], None
    for i in range(1 + max(1, reps - 1)):
        t0 = time.perf_counter()
        _, _, stats = gpm._slice_chain(log_p, x0[0], widths, lb, ub, N_KEEP, THIN, BURN, 5, 0)
        dt = (time.perf_counter() - t0) * 1e3
        if i >= 1:
            t.append(dt)
    row = {"row": f"N{N}_D{D}_baseline", "chains": 1, "evaluations": int(stats[0])}
    row["baseline_ms"], row["baseline_min_max_ms"] = spread(t)
    row["baseline_ms_per_eval"] = round(row["baseline_ms"] / int(stats[0]), 4)
    if (N, D) == SHAPES[0]:
        t0 = time.perf_counter()
        out = gpm.sample_hyperparameters(gp, x0[:1], device=False, **kw)
        row["numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        row["numpy_ms_per_eval"] = round(row["numpy_ms"] / int(out["stats"][0, 0]), 4)
    print(json.dumps(row), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--limit", type=int, default=420, help="seconds a shape's child process may take")
    ap.add_argument("--shape", type=int, default=None, help="(child) run shape number SHAPE in this process")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gp_hyp_rows.json"))
    a = ap.parse_args()
    if a.shape is not None:
        run_shape(*SHAPES[a.shape], a.reps, a.warm)
        return 0
    lines = []
    for i in range(len(SHAPES)):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, str(Path(__file__).resolve()), "--shape", str(i),
               "--reps", str(a.reps), "--warm", str(a.warm)]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
        for ln in p.stdout:  # (as they come: a row is printed when it is measured)
            if ln.startswith("{"):
                print(ln.rstrip("\n"), flush=True)
                lines.append(ln.rstrip("\n"))
        p.wait()
        if p.returncode != 0:
            print(f"shape {SHAPES[i]}: child ended with status {p.returncode}; nothing further is started", file=sys.stderr)
            return p.returncode
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
