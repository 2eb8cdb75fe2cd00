#!/usr/bin/env python
"""Device time of VariationalPosterior.mode at the benchmark's config 3 (D = 10, K = 50) and config 5 (D = 20,
K = 100) shapes, both spaces, both rng settings -> profiles/mode_rows.json.

    python tools/mode_rows.py [OUTPUT.json]

Wall time of the whole call (median of 5 after a warm-up), the mixture and transformer already on the device.
With rng="numpy" the call includes drawing n_opts x 1e5 samples from NumPy's stream on the host and uploading
them; with rng="philox" nothing but the result crosses PCIe.  The reference's wall times for the same shapes
are in tests/golden/mode.npz (``*_time``)."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import mode_host as mh  # noqa: E402


def main():
    g = np.load(ROOT / "tests" / "golden" / "mode.npz")
    rows = []
    for name in ("d10", "d20"):
        D, K = mh.CASES[name][:2]
        vp = mh.golden_vp(g, name)
        for orig in (False, True):
            for rng in ("philox", "numpy"):
                ts = []
                for rep in range(6):
                    vp._mode = None
                    np.random.seed(100)
                    t0 = time.perf_counter()
                    vp.mode(orig_flag=orig, rng=rng, seed=11)
                    ts.append(time.perf_counter() - t0)
                rows.append({"case": name, "D": D, "K": K, "orig_flag": orig, "rng": rng,
                             "median_ms": 1e3 * float(np.median(ts[1:])), "min_ms": 1e3 * float(np.min(ts[1:])),
                             "iterations": [int(v) for v in vp.mode_info["records"][:, 3]],
                             "reference_s": float(np.median(g[f"{name}_o{int(orig)}_time"]))})
                print(rows[-1], flush=True)
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "mode_rows.json"
    out.write_text(json.dumps({"rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
