#!/usr/bin/env python
"""Wall-clock milliseconds of the acquisition search of active_sample (vbmc/active_sample.py:310-349) at
M = 2**13 search points, two routes alternated on one box in one process:

  i   ``pyvbmc_amd.search(rng="philox")``: points drawn, scored and ranked on the device, one download;
  ii  the composed route it replaces: the reference's point generation in NumPy (tests/search_host.py ``points_numpy``,
      the reference's statements on NumPy's stream), this package's ``acq(X_search, ...)``, ``np.argsort`` and the gather.

    python tools/search_times.py [--reps 20] [--warm 3] [--out profiles/search_rows.json]

Shapes: config 3 (D = 10, K = 50, N = 400) and config 5 (D = 20, K = 100, N = 800) of pyvbmc_amd/synthetic.py, the GP of
the benchmark's synthetic fixture with one hyper-parameter sample, ``AcqFcnLog``, identity transformer, fractions
0.25 heavy / 0.25 mvn / 0.25 box, the rest from the posterior.  Per shape one JSON row: the median and min / max of
both routes, ``fused_lt_composed``, the composed route's parts (generation, evaluation, argsort + gather), and the device
phases of route i between HIP events (fill, evaluate + mask, sort + gather: ``vbmc_last_kernel_ms`` 9, 10, 11) taken in
calls of their own with timing on.  The process needs a GPU; it exits with an error without one."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import search_host as sh  # noqa: E402
from oracle import mixture_ref  # noqa: E402
from pyvbmc_amd import VariationalPosterior, _lib, acquisition, active_search, synthetic  # noqa: E402
from pyvbmc_amd import gp as gpm  # noqa: E402

M = 2**13
OPTIONS = dict(ns_search=M, cache_frac=0.5, search_cache_frac=0.0, heavy_tail_search_frac=0.25, mvn_search_frac=0.25,
               hpd_search_frac=0.0, box_search_frac=0.25, hpd_frac=0.8)


def setup(cfg, ctx):
    wl = synthetic.make_workload(cfg, Ns_total=1000)
    D = wl.D
    vp = VariationalPosterior(D, wl.K)
    vp.mu, vp.sigma, vp.lambd = wl.mu.copy(), wl.sigma.reshape(1, -1).copy(), wl.lambd.reshape(-1, 1).copy()
    vp.w, vp.eta = wl.w.reshape(1, -1).copy(), wl.eta.reshape(1, -1).copy()
    vp.ctx = ctx
    gp = gpm.GP(D, gpm.SquaredExponential(), gpm.NegativeQuadratic(), gpm.GaussianNoise(constant_add=True))
    gp.ctx = ctx
    gp.update(X_new=wl.X, y_new=wl.y, hyp=wl.hyp)
    mix = mixture_ref.Mixture.make(wl.mu, wl.sigma, wl.lambd, wl.w, wl.eta)
    lo, hi = wl.X.min(0), wl.X.max(0)
    state = {"cache": {"x_orig": np.zeros((0, D))}, "lb_search": (lo - 2.0).reshape(1, -1), "ub_search": (hi + 2.0).reshape(1, -1),
             "plb_tran": lo.reshape(1, -1), "pub_tran": hi.reshape(1, -1), "integer_vars": None,
             "lb_eps_orig": lo - 1.5, "ub_eps_orig": hi + 1.5, "variance_regularized_acq_fcn": True, "tol_gp_var": 1e-4,
             "gp_length_scale": np.exp(wl.hyp[0, :D])}
    flog = SimpleNamespace(X=wl.X, y=wl.y.reshape(-1, 1), X_flag=np.ones(wl.N, dtype=bool),
                           parameter_transformer=vp.parameter_transformer, y_max=float(np.max(wl.y)))
    return SimpleNamespace(D=D, K=wl.K, N=wl.N, vp=vp, gp=gp, mix=mix, state=state, flog=flog)


def med(t):
    return round(statistics.median(t), 4), [round(min(t), 4), round(max(t), 4)]


def run_shape(cfg, ctx, reps, warm):
    s = setup(cfg, ctx)
    acq = acquisition.AcqFcnLog()
    fused, composed, gen, ev, srt = [], [], [], [], []
    for i in range(warm + reps):  # the two routes alternate
        t0 = time.perf_counter()
        active_search.search(acq, s.gp, s.vp, s.flog, s.state, OPTIONS, rng="philox", seed=1000 + i, ctx=ctx)
        t1 = time.perf_counter()
        X, _ = sh.points_numpy(M, s.state, s.flog, s.mix, OPTIONS)
        t2 = time.perf_counter()
        v = acq(X, s.gp, s.vp, s.flog, s.state)
        t3 = time.perf_counter()
        order = np.argsort(v)
        Xs = X[order]  # noqa: F841  (the gather that becomes the next round's search cache)
        t4 = time.perf_counter()
        if i >= warm:
            fused.append((t1 - t0) * 1e3)
            composed.append((t4 - t1) * 1e3)
            gen.append((t2 - t1) * 1e3)
            ev.append((t3 - t2) * 1e3)
            srt.append((t4 - t3) * 1e3)
    row = {"row": f"config{cfg}_D{s.D}_K{s.K}_N{s.N}_M{M}", "acq": "AcqFcnLog", "reps": reps, "warm": warm}
    row["i_fused_ms"], row["i_fused_min_max_ms"] = med(fused)
    row["ii_composed_ms"], row["ii_composed_min_max_ms"] = med(composed)
    row["ii_generate_ms"], row["ii_evaluate_ms"], row["ii_argsort_gather_ms"] = med(gen)[0], med(ev)[0], med(srt)[0]
    row["fused_lt_composed"] = row["i_fused_ms"] < row["ii_composed_ms"]
    ctx.set_timing(1)
    phases = {_lib.T_SEARCH_FILL: [], _lib.T_SEARCH_EVAL: [], _lib.T_SEARCH_SORT: []}
    for i in range(warm + reps):
        active_search.search(acq, s.gp, s.vp, s.flog, s.state, OPTIONS, rng="philox", seed=2000 + i, ctx=ctx)
        for k in phases:
            phases[k].append(ctx.last_kernel_ms(k))
    ctx.set_timing(0)
    for k, name in ((_lib.T_SEARCH_FILL, "fill"), (_lib.T_SEARCH_EVAL, "evaluate"), (_lib.T_SEARCH_SORT, "sort")):
        row[f"i_device_{name}_ms"] = round(statistics.median(phases[k][warm:]), 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "search_rows.json"))
    a = ap.parse_args()
    ctx = _lib.Context(0)  # (raises without a device: nothing is measured on a CPU)
    _lib.set_default_context(ctx)
    lines = []
    for cfg in (3, 5):
        line = json.dumps(run_shape(cfg, ctx, a.reps, a.warm))
        print(line, flush=True)
        lines.append(line)
    ctx.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
