#!/usr/bin/env python
"""Whole inferences through ``pyvbmc_amd.VBMC`` on the device, one run per target, written to profiles/vbmc_driver_rows.json.

    python tools/vbmc_driver_rows.py [--targets mvn6,half_normal,cigar,cigar_bounded,uniform] [--seed 1]
                                     [--out profiles/vbmc_driver_rows.json]

Targets: the five problems of the reference's end-to-end tests with an error bound (tests/vbmc_driver_cases.py), at the
reference's default budget ``max_fun_evals = 50 (2 + D)``.  Per run: the errors the reference bounds by 0.5 (RMS error of
the posterior mean, ``|elbo - lnZ|``), iterations, the final K, the termination message, and wall seconds per stage --
active sampling, GP training, variational fit, finalize, and the best-posterior choice with the final boost -- in total
and per iteration (median and maximum over the iterations).  Needs a gfx950 device and the built library.
"""
import argparse
import json
import statistics
import sys
import time
import traceback
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import vbmc_driver_cases as cases  # noqa: E402

TARGETS = {"mvn6": lambda: cases.mvn(6), "half_normal": lambda: cases.half_normal(2), "cigar": lambda: cases.cigar(False),
           "cigar_bounded": lambda: cases.cigar(True), "uniform": cases.uniform}
PER_ITER = ("active_sampling", "gp_train", "variational_fit", "finalize")


def run(name, seed):
    case = TARGETS[name]()
    t0 = time.perf_counter()
    vb = cases.make(case, seed)
    vp, res = vb.optimize(on_iteration=lambda d: d.iteration % 10 or print(
        "  %s: iteration %d, %d evaluations, %.0f s" % (name, d.iteration, d.function_logger.func_count,
                                                         time.perf_counter() - t0), file=sys.stderr, flush=True))
    seconds = time.perf_counter() - t0
    err_mean, err_lnZ = cases.errors(case, vp, res)
    timers = vb.iteration_history["timer"]
    per_iter = {k: {"median": statistics.median(t.get(k, 0.0) for t in timers), "max": max(t.get(k, 0.0) for t in timers)}
                for k in PER_ITER}
    return {"target": name, "D": vb.D, "seed": seed, "budget": int(vb.options["max_fun_evals"]), "err_mean": err_mean,
            "err_lnZ": err_lnZ, "bound": 0.5, "within_bound": bool(err_mean < 0.5 and err_lnZ < 0.5), "elbo": float(res["elbo"]),
            "elbo_sd": float(res["elbo_sd"]), "lnZ": float(case.lnZ), "iterations": int(res["iterations"]) + 1,
            "func_count": int(res["func_count"]), "K": int(vp.K), "best_iter": int(res["best_iter"]),
            "convergence_status": res["convergence_status"], "message": res["message"], "seconds": seconds,
            "stage_seconds": res["timings"], "per_iteration_seconds": per_iter,
            "warmup_ended_at": vb.optim_state["last_warmup"] if vb.optim_state["last_warmup"] != float("inf") else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", default=",".join(TARGETS))
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vbmc_driver_rows.json"))
    a = ap.parse_args()
    rows = []
    for name in a.targets.split(","):
        try:
            rows.append(run(name, a.seed))
        except Exception:  # (recorded, and the other targets still run)
            rows.append({"target": name, "seed": a.seed, "error": traceback.format_exc()})
        print(json.dumps(rows[-1]), flush=True)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")  # (after every run: a long job leaves what it finished)


if __name__ == "__main__":
    main()
