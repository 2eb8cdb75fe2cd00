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
max|C_tmp(device) - C_tmp(host solves)| / max|C_tmp| over the rows' shapes (``ctmp_rel_err``).

    python tools/ais_rows.py --mcmc [--limit 400]

measures step 2, the MCMC, instead: IMIQR with 100 + 100 proposals and 100 MCMC samples at the reference's default thin
(1) and burn-in (50), at (D, N, S) = (10, 400, 8) and (20, 800, 8).  Per shape, in a fresh child process under
``timeout -k 10 <--limit>`` (after a child that does not exit with 0 nothing further is started): the whole call
without MCMC; with step 2 through the mirror's host loop handed ``tests/slice_host.sampler_class`` (the device chains'
algorithm, one device ``predict`` per evaluation); with ``sampler="device"`` at every workgroup size; the chains'
evaluation counts; and the launch's time between HIP events (``vbmc_last_kernel_ms(7)``).  ``step2_*_ms`` is the call's
time minus the call without MCMC.  The rows replace the ``mcmc_*`` rows of --out and leave its other rows alone."""
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


MCMC_SHAPES = [(10, 400, 8, 100), (20, 800, 8, 100)]  # (D, N, S, n_mcmc)


def mcmc_shape(i, reps):
    """(child) the rows of MCMC shape i, one JSON line each."""
    import slice_host

    D, N, S, n_mcmc = MCMC_SHAPES[i]
    ogp, mix = make_case(D, N, S, 100 + S)
    gp, vp, acq = PlainGP(ogp), PlainVP(mix), AcqFcnIMIQR()
    ctx = _lib.Context(0)
    _lib.set_default_context(ctx)

    def opts(n):
        return ais_host.Opts(active_importance_sampling_vp_samples=100, active_importance_sampling_box_samples=100,
                             active_importance_sampling_mcmc_samples=n, active_importance_sampling_mcmc_thin=1)

    def call(n, **kw):
        np.random.seed(1)
        t0 = time.perf_counter()
        out = active_importance_sampling(vp, gp, acq, opts(n), products=False, **kw)
        return (time.perf_counter() - t0) * 1e3, out

    call(0)  # (uploads the GP)
    base = statistics.median(call(0)[0] for _ in range(reps))
    tag = f"mcmc_D{D}_N{N}_S{S}_n{n_mcmc}"
    rows = [{"row": f"{tag}_no_mcmc", "call_ms": round(base, 3)}]
    ctx.set_timing(1)
    best = None
    for nt in (256, 512, 768):
        ctx.set_option("is_mcmc_threads", nt)
        call(n_mcmc, sampler="device", seed=3)
        ms, kms = [], []
        for _ in range(reps):
            ms.append(call(n_mcmc, sampler="device", seed=3)[0])
            kms.append(ctx.last_kernel_ms(_lib.T_IS_MCMC))
        st = ctx.__dict__["_is_mcmc_stats"]
        row = {"row": f"{tag}_device_threads{nt}", "call_ms": round(statistics.median(ms), 3),
               "step2_device_ms": round(statistics.median(ms) - base, 3), "kernel_ms": round(statistics.median(kms), 3),
               "evaluations_per_chain": st[:, 0].tolist(), "caps_hit": int(st[:, 2:].sum()),
               "us_per_evaluation": round(1e3 * statistics.median(kms) / float(st[:, 0].max()), 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        best = row if best is None or row["kernel_ms"] < best["kernel_ms"] else best
    ctx.set_timing(0)
    ctx.set_option("is_mcmc_threads", 512)
    cls = slice_host.sampler_class(3)
    host_ms, _ = call(n_mcmc, sampler=cls)  # once: tens of seconds
    row = {"row": f"{tag}_host_loop", "call_ms": round(host_ms, 3), "step2_host_loop_ms": round(host_ms - base, 3),
           "evaluations_per_chain": [int(r["stats"][0]) for r in cls.results],
           "host_loop_over_device": round((host_ms - base) / best["step2_device_ms"], 1), "device_row": best["row"]}
    rows.append(row)
    print(json.dumps(row), flush=True)
    print(json.dumps(rows[0]), flush=True)
    ctx.close()


def mcmc_rows(a):
    """(parent) every MCMC shape in a child of its own; the rows merged into --out."""
    lines = []
    for i, shape in enumerate(MCMC_SHAPES):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, str(Path(__file__).resolve()), "--mcmc-shape", str(i),
               "--reps", str(a.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        got = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        print("\n".join(got), flush=True)
        lines += got
        if p.returncode != 0:
            print(f"shape {shape}: child ended with status {p.returncode}; nothing further is started", file=sys.stderr)
            lines.append(json.dumps({"row": "mcmc_D%d_N%d_S%d_n%d" % shape,
                                     "status": f"not measured: the child process ended with status {p.returncode}"}))
            break
    out = Path(a.out)
    keep = [ln for ln in out.read_text().splitlines() if ln.strip() and not json.loads(ln)["row"].startswith("mcmc_")] \
        if out.exists() else []
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(keep + lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ais_rows.json"))
    ap.add_argument("--mcmc", action="store_true", help="measure step 2 (the MCMC) instead; rows merged into --out")
    ap.add_argument("--limit", type=int, default=400, help="--mcmc: seconds a shape's child process may take")
    ap.add_argument("--mcmc-shape", type=int, default=None, help="(child) run MCMC shape number MCMC_SHAPE in this process")
    a = ap.parse_args()
    if a.mcmc_shape is not None:
        return mcmc_shape(a.mcmc_shape, min(a.reps, 3))
    if a.mcmc:
        return mcmc_rows(a)
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
