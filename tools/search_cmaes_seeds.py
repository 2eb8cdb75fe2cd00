#!/usr/bin/env python
"""Seeds for the CMA-ES replay cases of tests/cmaes_host.py: for every case, the smallest gap between neighbouring ranked
values over a whole run of the host statement, per seed, in units of the acquisition parity bound (1e-9 max(1, |value|)).
A seed is usable when the gap is at least 1000 of those units and every exact tie was between identical rows; the twin
of tests/cmaes_host.py must also keep every rank.  CPU only.
    python tools/search_cmaes_seeds.py [case ...] [--seeds N]
"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import cmaes_host as ch  # noqa: E402


def golden(name):
    return np.load(ROOT / "tests" / "golden" / f"{name}.npz", allow_pickle=False)


def main(argv):
    n = int(argv[argv.index("--seeds") + 1]) if "--seeds" in argv else 6
    names = [a for a in argv if a in ch.SPECS] or list(ch.SPECS)
    for name in names:
        for seed in range(1, n + 1):
            k = ch.build_case(name, golden, seed=seed)
            t = time.perf_counter()
            es = ch.replay(k)
            ok = es.gap >= 1000 * ch.PARITY and es.tied_rows_only
            line = (f"{name} seed {seed}: stats {es.stats.tolist()} f0 {es.f0:.6g} f_best {es.f_best:.6g} "
                    f"gap {es.gap / ch.PARITY:.3g} units ties_ok {es.tied_rows_only} {time.perf_counter() - t:.1f}s")
            if ok:
                bounds, dev, same = ch.drift_bounds(k, es)
                line += f" twin_same_ranks {same} dev " + " ".join(f"{q}={v:.2e}" for q, v in dev.items())
            print(line, "USABLE" if ok and same else "", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
