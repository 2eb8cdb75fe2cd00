#!/usr/bin/env python
"""Wall-clock milliseconds of the CMA-ES refinement of the acquisition search (vbmc/active_sample.py:355-423) on the device
(``pyvbmc_amd.active_search.refine(device=True)``: lockstep runs, vbmc_search_cmaes), next to the composed route a user
had before it: the same algorithm and draws in NumPy around this package's batched acquisition call
(``refine(device=False)``: every generation uploads its points and waits for its values).

    python tools/search_cmaes_rows.py [--reps 5] [--warm 1] [--out profiles/search_cmaes_rows.json]

Shapes: config 3 (D = 10, K = 50, N = 400) and config 5 (D = 20, K = 100, N = 800) of pyvbmc_amd/synthetic.py as
tools/search_times.py sets them up (``AcqFcnLog``, one GP sample, identity transformer), a ranked search of 2**13 points
first, then the refinement from its best point with the reference's defaults (``search_max_fun_evals = 500 (D + 2)``,
``search_cmaes_vp_init``), R = 1 and 8 starts.  Per row (shape, R), medians over --reps alternating repetitions after
--warm, with [min, max]:
  device_ms       ``refine(device=True)`` end to end;   host_ms  ``refine(device=False)`` from the same start (R = 1 only);
  generations, evaluations   of run 0 (and the largest over the runs: the call's rounds);
  rounds_ms       ``vbmc_last_kernel_ms(T_SEARCH_CMAES)``, all rounds of a call between HIP events (a timed call of its own);
  ms_per_round    rounds_ms / (largest generation count + 2).
Every shape runs in a fresh child process under ``timeout -k 10 <--limit>``; after a child that does not exit with 0
nothing further is started and the tool exits with that status."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

CONFIGS = (3, 5)
STARTS = (1, 8)


def spread(t):
    return round(statistics.median(t), 3), [round(min(t), 3), round(max(t), 3)]


def run_shape(cfg, reps, warm):
    import search_times as st

    from pyvbmc_amd import _lib, acquisition, active_search

    ctx = _lib.Context(0)
    _lib.set_default_context(ctx)
    s = st.setup(cfg, ctx)
    acq = acquisition.AcqFcnLog()
    options = dict(st.OPTIONS, search_optimizer="cmaes", search_cmaes_vp_init=True, search_max_fun_evals=500 * (s.D + 2))
    res = active_search.search(acq, s.gp, s.vp, s.flog, s.state, options, rng="philox", seed=1000, ctx=ctx)
    for R in STARTS:
        dev, host, out, outh = [], [], None, None
        for i in range(warm + reps):  # the two routes alternate
            t0 = time.perf_counter()
            out = active_search.refine(res, acq, s.gp, s.vp, s.flog, s.state, options, n_starts=R, seed=7, ctx=ctx)
            t1 = time.perf_counter()
            if R == 1:
                outh = active_search.refine(res, acq, s.gp, s.vp, s.flog, s.state, options, seed=7, device=False, ctx=ctx)
            t2 = time.perf_counter()
            if i >= warm:
                dev.append((t1 - t0) * 1e3)
                host.append((t2 - t1) * 1e3)
        ctx.set_timing(1)
        active_search.refine(res, acq, s.gp, s.vp, s.flog, s.state, options, n_starts=R, seed=7, ctx=ctx)
        rounds_ms = ctx.last_kernel_ms(_lib.T_SEARCH_CMAES)
        ctx.set_timing(0)
        gens = int(out.stats[:, 0].max())
        row = {"row": f"config{cfg}_D{s.D}_K{s.K}_N{s.N}_R{R}", "acq": "AcqFcnLog", "reps": reps, "warm": warm,
               "runs": int(out.stats.shape[0]), "generations_run0": int(out.stats[0, 0]), "evaluations_run0": int(out.stats[0, 1]),
               "stop_reasons": out.stats[:, 2].tolist(), "generations_max": gens, "accepted": bool(out.accepted),
               "f_val_old": float(out.f_val_old), "f_val": float(out.f_val)}
        row["device_ms"], row["device_min_max_ms"] = spread(dev)
        row["rounds_ms"] = round(rounds_ms, 3)
        row["ms_per_round"] = round(rounds_ms / (gens + 2), 4)
        if R == 1:
            row["host_ms"], row["host_min_max_ms"] = spread(host)
            row["host_stats_equal"] = bool((outh.stats == out.stats).all())
            row["device_lt_host"] = row["device_ms"] < row["host_ms"]
        print(json.dumps(row), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--limit", type=int, default=300, help="seconds a shape's child process may take")
    ap.add_argument("--shape", type=int, default=None, help="(child) run shape number SHAPE in this process")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "search_cmaes_rows.json"))
    a = ap.parse_args()
    if a.shape is not None:
        run_shape(CONFIGS[a.shape], a.reps, a.warm)
        return 0
    lines = []
    for i in range(len(CONFIGS)):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, str(Path(__file__).resolve()), "--shape", str(i),
               "--reps", str(a.reps), "--warm", str(a.warm)]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
        for ln in p.stdout:  # (as they come: a row is printed when it is measured)
            if ln.startswith("{"):
                print(ln.rstrip("\n"), flush=True)
                lines.append(ln.rstrip("\n"))
        p.wait()
        if p.returncode != 0:
            print(f"config {CONFIGS[i]}: child ended with status {p.returncode}; nothing further is started", file=sys.stderr)
            return p.returncode
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
