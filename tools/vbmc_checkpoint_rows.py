#!/usr/bin/env python
"""What a checkpoint of ``VBMC.optimize`` costs: per iteration the seconds of the write and the bytes of the file, beside the
same iteration's stage times (``iteration_history["timer"]``).  One run per target with ``checkpoint_every=1``, written to
profiles/vbmc_checkpoint_rows.json; profiles/vbmc_checkpoint.md reads from it.

    python tools/vbmc_checkpoint_rows.py [--targets mvn2,mvn6] [--seed 1] [--out profiles/vbmc_checkpoint_rows.json]

Targets: ``mvn2`` -- tests/vbmc_driver_cases.py ``mvn(2, max_fun_evals=60)``, the run of the GPU tests; ``mvn6`` -- the D = 6
row of profiles/vbmc_driver.md at its default budget.  Deterministic by the seed.  Needs a gfx950 device and the built library.
"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import vbmc_driver_cases as cases  # noqa: E402

TARGETS = {"mvn2": lambda: cases.mvn(2, max_fun_evals=60), "mvn6": lambda: cases.mvn(6)}
STAGES = ("active_sampling", "gp_train", "variational_fit", "finalize")


def run(name, seed, directory):
    vb = cases.make(TARGETS[name](), seed)
    t0 = time.perf_counter()
    vp, res = vb.optimize(checkpoint=Path(directory) / (name + ".pkl"))
    seconds = time.perf_counter() - t0
    timers, h = vb.iteration_history["timer"], vb.iteration_history
    rows = []
    for it, write_s, size in vb.checkpoint_log[:-1]:  # (the last entry is the save after the loop)
        t = timers[it]
        rows.append({"iteration": it, "N": int(h["gp"][it].X.shape[0]), "S": int(len(h["gp"][it].posteriors)), "write_s": write_s,
                     "bytes": size, **{k: t.get(k, 0.0) for k in STAGES},
                     "write_over_gp_train": write_s / t["gp_train"] if t.get("gp_train") else None})
    final = vb.checkpoint_log[-1]
    return {"target": name, "D": vb.D, "seed": seed, "iterations": vb.iteration + 1, "func_count": int(res["func_count"]),
            "seconds": seconds, "write_seconds_total": sum(c[1] for c in vb.checkpoint_log), "final_write_s": final[1],
            "final_bytes": final[2], "writes_slower_than_gp_train": [r["iteration"] for r in rows if r["write_s"] > r["gp_train"]],
            "per_iteration": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", default=",".join(TARGETS))
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vbmc_checkpoint_rows.json"))
    a = ap.parse_args()
    out = []
    with tempfile.TemporaryDirectory() as d:
        for name in a.targets.split(","):
            row = run(name, a.seed, d)
            out.append(row)
            last = row["per_iteration"][-1]
            print("%s: %d iterations in %.1f s, writes %.2f s in all; last iteration: write %.4f s, %d bytes, gp_train %.3f s; "
                  "slower than gp_train in %s" % (name, row["iterations"], row["seconds"], row["write_seconds_total"],
                                                  last["write_s"], last["bytes"], last["gp_train"],
                                                  row["writes_slower_than_gp_train"] or "no iteration"), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
