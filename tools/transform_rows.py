#!/usr/bin/env python
"""End-to-end milliseconds of VariationalPosterior's original-space calls with a reference-shaped
transformer (D = 10, probit, plausible bounds, rotoscaled): the device transformer (pyvbmc_amd/
transformer.py) against the host one (VBMC_HIP_TRANSFORM=0), and the transformed-space calls.

    python tools/transform_rows.py [--reps 5]

Rows: sample(1e6) and pdf(1e6) with orig_flag True / False, moments(1e6, orig_flag=True), and
kl_div(N=1e5) between two posteriors with different transformers (rng="philox" throughout).
Median of --reps calls after one warm-up call; one JSON line per row."""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from pyvbmc_amd import VariationalPosterior, _lib  # noqa: E402
from transform_host import RefShapedTransformer  # noqa: E402


def make_pt(D, rng, shift=0.0):
    lb, ub = -5.0 * np.ones(D), 5.0 * np.ones(D)
    mu, delta = shift + 0.1 * rng.standard_normal(D), np.exp(0.1 * rng.standard_normal(D))
    q, r = np.linalg.qr(rng.standard_normal((D, D)))
    return RefShapedTransformer(np.full(D, 12.0), lb, ub, mu, delta, q * np.sign(np.diag(r)),
                                np.exp(0.2 * rng.standard_normal(D)))


def make_vp(D, K, pt, rng, ctx):
    vp = VariationalPosterior(D, K, parameter_transformer=pt)
    vp.ctx = ctx
    vp.mu = 0.5 * rng.standard_normal((D, K))
    vp.sigma = 0.5 * np.ones((1, K))
    vp.lambd = np.ones((D, 1))
    vp.w = np.ones((1, K)) / K
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
    ap.add_argument("--D", type=int, default=10)
    ap.add_argument("--K", type=int, default=10)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = _lib.Context(0)
    vp = make_vp(a.D, a.K, make_pt(a.D, rng), rng, ctx)
    vp2 = make_vp(a.D, a.K, make_pt(a.D, rng, 0.05), rng, ctx)
    n = 10**6
    x, _ = vp.sample(n, orig_flag=True, rng="philox", seed=1)
    u = vp.parameter_transformer(x)
    rows = {
        "sample_1e6_orig": lambda: vp.sample(n, orig_flag=True, rng="philox", seed=2),
        "sample_1e6_transformed": lambda: vp.sample(n, orig_flag=False, rng="philox", seed=2),
        "pdf_1e6_orig": lambda: vp.pdf(x, orig_flag=True),
        "pdf_1e6_transformed": lambda: vp.pdf(u, orig_flag=False),
        "moments_1e6_orig": lambda: vp.moments(n, orig_flag=True, cov_flag=True, rng="philox", seed=3),
        "kl_div_1e5_two_transformers": lambda: vp.kl_div(vp2, N=10**5, rng="philox", seed=4),
    }
    for name, fn in rows.items():
        os.environ["VBMC_HIP_TRANSFORM"] = "1"
        dev = timed(fn, a.reps)
        os.environ["VBMC_HIP_TRANSFORM"] = "0"
        host = timed(fn, max(1, a.reps // 2)) if "orig" in name or "kl" in name else None
        os.environ["VBMC_HIP_TRANSFORM"] = "1"
        print(json.dumps({"row": name, "device_ms": round(dev, 3),
                          "host_transform_ms": None if host is None else round(host, 3)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
