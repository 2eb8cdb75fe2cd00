#!/usr/bin/env python
"""Wall-clock milliseconds of pyvbmc_amd.active_importance_sampling on the device, next to the host route on the same
box: tests/ais_host.py (the reference's arithmetic in NumPy / SciPy, step 3 by ``solve_triangular``) followed by
``vbmc_acq_is_set``.

    python tools/ais_rows.py [--reps 7] [--out profiles/ais_rows.json]

Shapes: D = 20, N = 800, S in {1, 8}; VIQR with 100 importance points, IMIQR with 100 + 100 and no MCMC.  Every device
row is timed under both draw sources and with ``products`` on and off; the host column runs the same function on
``np.random`` and then uploads its state.  Median, minimum and maximum of --reps calls after two warm-up calls (host:
of max(3, reps // 2) calls after one); ``host_over_device`` is the ratio of the medians.  One JSON line per row, also
written to --out.  The last line holds the largest
max|C_tmp(device) - C_tmp(host solves)| / max|C_tmp| over the rows' shapes (``ctmp_rel_err``)."""
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

import ais_host  # noqa: E402
from helpers import PlainGP, PlainVP  # noqa: E402
from oracle import gp_ref, mixture_ref  # noqa: E402
from pyvbmc_amd import _lib  # noqa: E402
from pyvbmc_amd.acquisition import AcqFcnIMIQR, AcqFcnVIQR  # noqa: E402
from pyvbmc_amd.active_importance_sampling import active_importance_sampling  # noqa: E402


def make_case(D, N, S, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    y = (-0.5 * np.sum(X**2, axis=1) + 0.05 * rng.standard_normal(N)).reshape(-1, 1)
    hyp = np.array([np.concatenate([np.log(1.5 + rng.random(D)), [np.log(2.0 + 0.1 * s)], [np.log(0.05 + 0.01 * s)], [0.1],
                                    np.zeros(D), np.log(3.0) * np.ones(D)]) for s in range(S)])
    ogp = gp_ref.make_gp(X, y, hyp, gp_ref.MEAN_NEGQUAD)
    mix = mixture_ref.Mixture.make(0.5 * rng.standard_normal((D, 4)), [0.4, 0.5, 0.6, 0.7], np.ones(D), [0.1, 0.2, 0.3, 0.4])
    return ogp, mix


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ais_rows.json"))
    a = ap.parse_args()
    ctx = _lib.Context(0)
    _lib.set_default_context(ctx)
    D, N = 20, 800
    lines, worst = [], 0.0
    for S in (1, 8):
        ogp, mix = make_case(D, N, S, 100 + S)
        gp, vp = PlainGP(ogp), PlainVP(mix)
        for kind, cls, opts in (
            (ais_host.VIQR, AcqFcnVIQR, ais_host.Opts(active_importance_sampling_mcmc_samples=100)),
            (ais_host.IMIQR, AcqFcnIMIQR, ais_host.Opts(active_importance_sampling_vp_samples=100,
                                                       active_importance_sampling_box_samples=100,
                                                       active_importance_sampling_mcmc_samples=0)),
        ):
            acq = cls()

            def host_route():
                with np.errstate(all="ignore"):
                    st = ais_host.ais(mix, ogp, kind, opts)
                Xa, Ct, fs2 = _lib.f64(st["X"]), _lib.f64(st["C_tmp"]), _lib.f64(st["f_s2"])
                lnw = None if kind == ais_host.VIQR else _lib.f64(st["ln_weights"])
                ctx.check(ctx._lib.vbmc_acq_is_set(ctx._h, Xa.shape[0], _lib.ptr(Xa), 0, _lib.ptr(Ct), _lib.ptr(fs2),
                                                   _lib.ptr(lnw)))
                return st

            active_importance_sampling(vp, gp, acq, opts)  # (uploads the GP: not part of either column)
            np.random.seed(1)
            host_ms, host_lo, host_hi = timed(host_route, max(3, a.reps // 2), 1)
            # the device products against the host solves on the device's own points
            dev = active_importance_sampling(vp, gp, acq, opts, rng="philox", seed=3)
            with np.errstate(all="ignore"):
                ref = ais_host.from_points(ogp, mix, dev["X"], kind, 100, 100)
            rel = float(np.max(np.abs(dev["C_tmp"] - ref["C_tmp"])) / np.max(np.abs(ref["C_tmp"])))
            worst = max(worst, rel)
            for rng in ("numpy", "philox"):
                for products in (True, False):
                    ms, lo, hi = timed(lambda: active_importance_sampling(vp, gp, acq, opts, rng=rng, seed=3,
                                                                          products=products), a.reps, 2)
                    line = json.dumps({"row": f"{kind}_D{D}_N{N}_S{S}_{rng}_products{int(products)}",
                                       "device_ms": round(ms, 3), "device_min_max_ms": [round(lo, 3), round(hi, 3)],
                                       "host_route_ms": round(host_ms, 3),
                                       "host_min_max_ms": [round(host_lo, 3), round(host_hi, 3)],
                                       "host_over_device": round(host_ms / ms, 2), "ctmp_rel_err": float(f"{rel:.3e}")})
                    print(line, flush=True)
                    lines.append(line)
    line = json.dumps({"row": "ctmp_rel_err_max", "ctmp_rel_err": float(f"{worst:.3e}")})
    print(line, flush=True)
    lines.append(line)
    # the figure tests/test_ais_gpu.py asserts 10 x of: its D = 4, N = 150, S = 3 case (one non-Cholesky sample)
    ogp, mix, _, _ = ais_host.larger_case()
    gp, vp, acq, tile = PlainGP(ogp), PlainVP(mix), AcqFcnIMIQR(), 0.0
    for n_vp, n_box in ((40, 30), (70, 59)):
        opts = ais_host.Opts(active_importance_sampling_vp_samples=n_vp, active_importance_sampling_box_samples=n_box,
                             active_importance_sampling_mcmc_samples=0)
        np.random.seed(7)
        dev = active_importance_sampling(vp, gp, acq, opts)
        with np.errstate(all="ignore"):
            ref = ais_host.from_points(ogp, mix, dev["X"], ais_host.IMIQR, n_vp, n_box)
        tile = max(tile, float(np.max(np.abs(dev["C_tmp"] - ref["C_tmp"])) / np.max(np.abs(ref["C_tmp"]))))
    line = json.dumps({"row": "ctmp_rel_err_tile_edges_D4_N150_S3", "ctmp_rel_err": float(f"{tile:.3e}")})
    print(line, flush=True)
    lines.append(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
