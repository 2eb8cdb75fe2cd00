#!/usr/bin/env python
"""Milliseconds of VariationalPosterior.marginals on the device (csrc/marginals.hip), next to its NumPy route
(device=False) on the same samples on the same box.

    python tools/marginals_rows.py [--reps 5] [--out profiles/marginals_rows.json]

Rows: D in {2, 10, 20}, n in {1e5, 1e6, the cap 2^22}, bins = 40, K = 4, rng="philox" (draws on the device), and one
D = 32 row at n = 1e6.  Per row: the wall time of the device call (median of --reps after one warm-up call); the wall
time of what a user without the device route pays -- vp.sample(n, rng="philox") with its download, then device=False
on those samples (one call; two and the median below 1e6 samples); the six stage times between HIP events (samples,
sort + columns, kde, bin indices, pair histograms, levels; median over the same calls); for the pair kernel the bytes
of the index array (D x n) and the bytes its workgroups load (a group of g pairs loads g + (rows i it spans) rows) over
its time, and that load count as passes over the index array.  One JSON line per row, also written to --out."""
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
from pyvbmc_amd import marginals as mg  # noqa: E402

PAIR_LDS, MAX_GROUP = 128 * 1024, 32  # csrc/marginals.hip: kPairLds, kPairMaxGroup


def make_vp(D, K, seed, ctx):
    vp = VariationalPosterior(D, K)
    vp.ctx = ctx
    vp.mu, vp.sigma, vp.lambd, vp.w = kde_host.mixture_params(D, K, seed)
    return vp


def pair_passes(D, bins):
    """(pairs a group, groups, rows of idx loaded per sample tile / D)."""
    pairs = mg.pair_table(D)
    G = max(1, min(MAX_GROUP, PAIR_LDS // (bins * bins * 4), len(pairs)))
    rows = 0
    for p0 in range(0, len(pairs), G):
        grp = pairs[p0:p0 + G]
        rows += len(grp) + len(set(grp[:, 0]))
    return G, -(-len(pairs) // G), rows / D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "marginals_rows.json"))
    ap.add_argument("--no-host", action="store_true", help="device rows only")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    _lib.set_default_context(ctx)
    bins, K = 40, 4
    shapes = [(D, n) for D in (2, 10, 20) for n in (10**5, 10**6, mg.MAX_SAMPLES)] + [(32, 10**6)]
    lines = []
    for D, n in shapes:
        vp = make_vp(D, K, 3, ctx)
        stage = np.zeros(6, dtype=np.float32)
        wall, stages = [], []
        for it in range(a.reps + 1):
            t0 = time.perf_counter()
            mg.marginals(vp, n, bins, rng="philox", seed=1, stage_ms=stage)
            if it:
                wall.append((time.perf_counter() - t0) * 1e3)
                stages.append(stage.copy())
        st = np.median(np.array(stages), axis=0)
        host = None
        if not a.no_host:
            t = []
            for _ in range(1 if n >= 10**6 else 2):
                t0 = time.perf_counter()
                x, _ = vp.sample(n, rng="philox", seed=1)
                vp.marginals(samples=x, bins=bins, device=False)
                t.append((time.perf_counter() - t0) * 1e3)
            host = statistics.median(t)
        G, groups, passes = pair_passes(D, bins)
        pair_s = float(st[4]) * 1e-3
        line = json.dumps({
            "row": f"marginals_D{D}_n{n}_bins{bins}", "device_ms": round(statistics.median(wall), 3),
            "host_route_ms": None if host is None else round(host, 1),
            "stage_ms": dict(zip(("samples", "sort", "kde", "bins", "pairs", "levels"), (round(float(v), 3) for v in st))),
            "pairs_per_group": G, "pair_groups": groups, "idx_passes": round(passes, 2),
            "pair_idx_GBps": round(D * n / pair_s / 1e9, 2) if pair_s > 0 else None,
            "pair_loaded_GBps": round(passes * D * n / pair_s / 1e9, 2) if pair_s > 0 else None})
        print(line, flush=True)
        lines.append(line)
    G, groups, passes = pair_passes(32, 128)
    line = json.dumps({"row": "plan_D32_bins128", "pairs_per_group": G, "pair_groups": groups, "idx_passes": round(passes, 2)})
    print(line, flush=True)
    lines.append(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
