#!/usr/bin/env python
"""Wall-clock milliseconds per acquired point of every stage of ``pyvbmc_amd.active_sample``, one shape per BASELINE
config, and the one-point append under per-point noise against the rebuild it replaces.

    python tools/active_sample_rows.py [--points 4] [--reps 10] [--warm 2] [--out profiles/active_sample_rows.json]
    python tools/active_sample_rows.py --not-run      # write the file with every row marked as not run (no GPU touched)

Stage rows (``kind: "stages"``): the BASELINE shapes (D, K, N) of pyvbmc_amd/synthetic.py with S = 8 hyper-parameter
samples, ``ns_search = 2^13``, ``search_optimizer = "cmaes"`` with ``search_max_fun_evals = 500 (D + 2)``, ``rng="philox"``;
configs 1-4 an exact quadratic target with ``AcqFcnLog``, config 5 a target with user-provided noise and ``AcqFcnVIQR``
(100 importance points).  The stages are cut by wrapping the driver's own hooks: ``_search`` / ``_refine`` around the real
functions, ``timer`` for the target (``fun_time``) and the GP update (``gp_train``); the pre-computation is what lies
between the end of one point's update and the start of the next search.  Per stage the median over the points after the
first (which pays the one-time allocations) -- the last point has no GP update.

Append rows (``kind: "noisy_append"``): D = 20, S = 8, N = 400 and 800, user-provided noise; ``append_point`` (the noisy
entry, fetch=False) against ``GP.update(device=True, fetch=False)`` on the N + 1 rows, the N-point posterior rebuilt
before every call outside the timing; median of --reps after --warm.

Every row runs in a fresh child process under ``timeout -k 10 <--limit>``; after a child that does not exit with 0 nothing
further is started, and the rows not reached are written with ``"measured": false``.  No time is promised anywhere: the
file records what was measured, and says so for every row that was not."""
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
sys.path.insert(0, str(ROOT / "tests"))

STAGES = ("precompute", "search", "refine", "target", "gp_update")
ROWS = [("noisy_append", N) for N in (400, 800)] + [("stages", cfg) for cfg in (1, 2, 3, 4, 5)]


def row_name(kind, arg):
    return f"config{arg}" if kind == "stages" else f"D20_N{arg}_S8"


class StageTimer:
    """``timer`` of the driver: the intervals by name, in order."""

    def __init__(self):
        self.t0, self.spans = {}, []

    def start_timer(self, name):
        self.t0[name] = time.perf_counter()

    def stop_timer(self, name):
        t1 = time.perf_counter()
        self.spans.append((name, self.t0.pop(name), t1))


def run_stages(cfg, points):
    import active_sample_host as ash
    from pyvbmc_amd import VariationalPosterior, _lib, active_sample, active_search, synthetic
    from pyvbmc_amd import gp as gpm
    from pyvbmc_amd.variational_posterior import IdentityTransformer

    S = 8
    wl = synthetic.make_workload(cfg, S=S)
    D, K, N = wl.D, wl.K, wl.N
    noisy = cfg == 5
    ctx = _lib.Context(0)
    _lib.set_default_context(ctx)
    pt = IdentityTransformer(D)

    def target(x):
        f = float(-0.5 * np.sum(np.square(x)))
        return (f, 0.1 + 0.05 * abs(float(np.ravel(x)[0]))) if noisy else f

    log = ash.PlainLogger(target, D, noisy, 2 if noisy else 0, cache_size=N + points + 8, parameter_transformer=pt)
    for x in wl.X:
        log(x)
    vp = VariationalPosterior(D, K, parameter_transformer=pt)
    vp.ctx = ctx
    vp.mu, vp.sigma, vp.lambd = wl.mu.copy(), wl.sigma.reshape(1, -1).copy(), wl.lambd.reshape(-1, 1).copy()
    vp.w, vp.eta = wl.w.reshape(1, -1).copy(), wl.eta.reshape(1, -1).copy()
    gp = gpm.GP(D, gpm.SquaredExponential(), gpm.NegativeQuadratic(), gpm.GaussianNoise(constant_add=True, user_provided_add=noisy))
    gp.ctx = ctx
    hyp = wl.hyp.copy()
    hyp[:, D + 1] = np.log(0.05)
    gp.update(log.X[log.X_flag].copy(), log.y[log.X_flag].copy(), ash.training_s2(log), hyp, device=True, fetch=False)
    one = np.ones((1, D))
    st = {"cache": {"x_orig": np.zeros((0, D)), "y_orig": np.zeros(0)}, "search_cache": np.zeros((0, D)), "lb_search": -4.0 * one,
          "ub_search": 4.0 * one, "lb_tran": -np.inf * one, "ub_tran": np.inf * one, "plb_tran": -one, "pub_tran": one,
          "lb_eps_orig": -np.inf * one, "ub_eps_orig": np.inf * one, "integer_vars": None, "variance_regularized_acq_fcn": True,
          "tol_gp_var": 1e-4, "iter": 5, "last_warmup": 0, "hyp_dict": None, "recompute_var_post": True, "entropy_alpha": 0.0}
    options = dict(ash.DEFAULT_OPTIONS, ns_search=2**13, search_optimizer="cmaes", search_max_fun_evals=500 * (D + 2),
                   search_acq_fcn=["AcqFcnVIQR()" if noisy else "AcqFcnLog()"], active_importance_sampling_mcmc_samples=100)
    timer, marks = StageTimer(), []

    def search(*a, **kw):
        t0 = time.perf_counter()
        out = active_search.search(*a, **kw)
        marks.append(("search", t0, time.perf_counter()))
        return out

    def refine(*a, **kw):
        t0 = time.perf_counter()
        out = active_search.refine(*a, **kw)
        marks.append(("refine", t0, time.perf_counter()))
        return out

    np.random.seed(1)
    t_begin = time.perf_counter()
    active_sample(gp, points, st, log, {"r_index": [1.0]}, vp, options, rng="philox", seed=7, ctx=ctx, timer=timer, fetch=False,
                  _search=search, _refine=refine)
    t_end = time.perf_counter()
    per = {k: [] for k in STAGES}
    searches = [m for m in marks if m[0] == "search"]
    refines = [m for m in marks if m[0] == "refine"]
    targets = [s for s in timer.spans if s[0] == "fun_time"]
    updates = [s for s in timer.spans if s[0] == "gp_train"]
    prev_end = t_begin
    for i in range(points):
        per["precompute"].append(searches[i][1] - prev_end)
        per["search"].append(searches[i][2] - searches[i][1])
        per["refine"].append(refines[i][2] - refines[i][1])
        per["target"].append(targets[i][2] - targets[i][1])
        if i < len(updates):
            per["gp_update"].append(updates[i][2] - updates[i][1])
            prev_end = updates[i][2]
    row = {"kind": "stages", "row": row_name("stages", cfg), "measured": True, "D": D, "K": K, "N": N, "S": S, "points": points,
           "acq": options["search_acq_fcn"][0], "total_ms": round((t_end - t_begin) * 1e3, 3)}
    for k in STAGES:
        v = per[k][1:] if len(per[k]) > 1 else per[k]
        row[f"{k}_ms"] = round(statistics.median(v) * 1e3, 3)
        row[f"{k}_first_ms"] = round(per[k][0] * 1e3, 3)
    print(json.dumps(row), flush=True)
    ctx.close()


def run_append(N, reps, warm):
    from pyvbmc_amd import _lib
    from pyvbmc_amd import gp as gpm

    D, S = 20, 8
    ctx = _lib.Context(0)
    _lib.set_default_context(ctx)
    rng = np.random.default_rng(N)
    X = rng.standard_normal((N + 1, D))
    y = (-0.5 * np.sum(X**2, axis=1) + 0.05 * rng.standard_normal(N + 1)).reshape(-1, 1)
    s2 = rng.uniform(0.01, 1.0, size=(N + 1, 1))
    s2[N, 0] = max(s2[N, 0], 1.5 * float(np.min(s2[:N])))
    hyp = np.array([np.concatenate([np.log(1.5 + rng.random(D)), [np.log(2.0 + 0.1 * s)], [np.log(0.05 + 0.01 * s)], [0.1],
                                    np.zeros(D), np.log(3.0) * np.ones(D)]) for s in range(S)])
    gp = gpm.GP(D, gpm.SquaredExponential(), gpm.NegativeQuadratic(), gpm.GaussianNoise(constant_add=True, user_provided_add=True))
    gp.ctx = ctx

    def build(n):
        gp.update(X[:n], y[:n], s2[:n], hyp, device=True, fetch=False)

    def timed(fn):
        t = []
        for i in range(warm + reps):
            build(N)
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(t[warm:]), 3)

    real, names = ctx._lib, []
    ctx._lib = type("CallLog", (), {"__getattr__": lambda self, k: (names.append(k), getattr(real, k))[1]})()

    def append():
        del names[:]
        gpm.append_point(gp, X[N], y[N, 0], s2[N, 0], ctx=ctx, fetch=False)
        if "vbmc_gp_posterior" in names:
            raise RuntimeError("the noisy append was refused and the posterior rebuilt: the row would time the rebuild")

    row = {"kind": "noisy_append", "row": row_name("noisy_append", N), "measured": True, "D": D, "N": N, "S": S, "reps": reps,
           "warm": warm, "append_noisy_ms": timed(append), "rebuild_ms": timed(lambda: build(N + 1))}
    row["append_lt_rebuild"] = row["append_noisy_ms"] < row["rebuild_ms"]
    print(json.dumps(row), flush=True)
    ctx.close()


def not_run(kind, arg, why):
    return json.dumps({"kind": kind, "row": row_name(kind, arg), "measured": False, "note": why})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a row's child process may take")
    ap.add_argument("--row", type=int, default=None, help="(child) run row number ROW in this process")
    ap.add_argument("--not-run", action="store_true", help="write every row as not run")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "active_sample_rows.json"))
    a = ap.parse_args()
    if a.row is not None:
        kind, arg = ROWS[a.row]
        if kind == "stages":
            run_stages(arg, a.points)
        else:
            run_append(arg, a.reps, a.warm)
        return 0
    lines, status = [], 0
    for i, (kind, arg) in enumerate(ROWS):
        if a.not_run or status:
            lines.append(not_run(kind, arg, "not run: nothing is measured for this row yet" if a.not_run else
                                 f"not run: an earlier row's process ended with status {status}"))
            continue
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, str(Path(__file__).resolve()), "--row", str(i), "--points",
               str(a.points), "--reps", str(a.reps), "--warm", str(a.warm)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        found = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not found:
            status = p.returncode or 1
            print(f"row {row_name(kind, arg)}: child ended with status {p.returncode}; nothing further is started", file=sys.stderr)
            lines.append(not_run(kind, arg, f"not measured: the row's process ended with status {p.returncode}"))
            continue
        print(found[-1], flush=True)
        lines.append(found[-1])
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
