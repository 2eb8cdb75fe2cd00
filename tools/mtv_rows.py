#!/usr/bin/env python
"""End-to-end milliseconds of VariationalPosterior.mtv and pyvbmc_amd.stats.kde_1d on the device
(csrc/kde.hip), next to tests/kde_host.py's NumPy / SciPy restatement of the same work on the same box.

    python tools/mtv_rows.py [--reps 5] [--out profiles/mtv_rows.json]

Rows: mtv(vp2, N=1e5) at D = 10, K = 50 with rng="philox" (draws on the device) and rng="numpy" (the
reference's NumPy stream, drawn on the host and uploaded once); kde_1d on 1e5 and 1e6 samples at n = 2^14.
The host column runs the restatement on the same samples (for mtv: the samples of sample(N, True, True)).
Median of --reps calls after one warm-up call (host: median of max(1, reps // 2)); one JSON line per row,
also written to --out."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import kde_host  # noqa: E402
from pyvbmc_amd import VariationalPosterior, _lib  # noqa: E402
from pyvbmc_amd.stats import kde_1d  # noqa: E402


def make_vp(D, K, seed, ctx):
    vp = VariationalPosterior(D, K)
    vp.ctx = ctx
    vp.mu, vp.sigma, vp.lambd, vp.w = kde_host.mixture_params(D, K, seed)
    return vp


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mtv_rows.json"))
    ap.add_argument("--no-host", action="store_true", help="device rows only (e.g. under a profiler)")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    _lib.set_default_context(ctx)
    D, K, N = 10, 50, 10**5
    vp1, vp2 = make_vp(D, K, 4, ctx), make_vp(D, K, 5, ctx)
    inf = np.full(D, np.inf)
    xx1 = vp1.sample(N, True, True, rng="philox", seed=1)[0]
    xx2 = vp2.sample(N, True, True, rng="philox", seed=2)[0]
    r = np.random.RandomState(0)
    s5, s6 = r.randn(10**5), r.randn(10**6)
    rows = [
        ("mtv_D10_K50_N1e5_philox", lambda: vp1.mtv(vp2, N=N, rng="philox", seed=1),
         lambda: kde_host.mtv_host(xx1, xx2, -inf, inf, -inf, inf)),
        ("mtv_D10_K50_N1e5_numpy", lambda: vp1.mtv(vp2, N=N, rng="numpy"),
         lambda: kde_host.mtv_host(xx1, xx2, -inf, inf, -inf, inf)),
        ("kde_1d_1e5_n2^14", lambda: kde_1d(s5, 2**14), lambda: kde_host.kde_1d_host(s5, 2**14)),
        ("kde_1d_1e6_n2^14", lambda: kde_1d(s6, 2**14), lambda: kde_host.kde_1d_host(s6, 2**14)),
    ]
    lines = []
    for name, dev_fn, host_fn in rows:
        dev = timed(dev_fn, a.reps)
        host = None if a.no_host else timed(host_fn, max(1, a.reps // 2))
        line = json.dumps({"row": name, "device_ms": round(dev, 3),
                           "host_restatement_ms": None if host is None else round(host, 3)})
        print(line, flush=True)
        lines.append(line)
    if not a.no_host:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
