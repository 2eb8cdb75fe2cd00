#!/usr/bin/env python
"""Wall-clock milliseconds of the sieve (``pyvbmc_amd.sieve.sieve``: candidates drawn, scored and ranked on the device)
at the benchmark's two shapes, next to the routes that do the generation on the host.

    python tools/sieve_rows.py [--reps 7] [--warm 2] [--out profiles/sieve_rows.json]

Shapes: BASELINE config 3 (D = 10, K = 50, N = 400, init_N = 2 500) and config 5 (D = 20, K = 100, N = 800, init_N =
5 000), ``pyvbmc_amd.synthetic.make_workload``'s data, negative-quadratic mean, one hyper-parameter sample, ``K_new = K``,
``best_N = 2`` (the three-way split), all four blocks optimised.  Per (shape, route), medians over --reps calls after
--warm, with [min, max]; every call ends in the download's stream wait.

Routes:
  device_numpy / device_philox   ``sieve(device=True)`` with ``rng="numpy"`` / ``rng="philox"``, split into
      generate_ms   draws (numpy: on the host), constants and ``vbmc_sieve_fill`` with its uploads, host clock;
      fill_ms       the fill launch between HIP events (a timed call of its own: ``vbmc_last_kernel_ms`` 15);
      score_ms, rank_ms   ``vbmc_sieve_eval``'s scoring launches and its rank + gather between events (16, 17);
      eval_ms       the ``vbmc_sieve_eval`` call, host clock: scoring, rank and the one download;
      download_ms   eval_ms - score_ms - rank_ms of the timed call: the copy, its wait and the host's memcpy;
      to_vps_ms     ``Candidates.to_vps()`` and the two fancy-indexing sorts;
      sieve_ms      the whole call.
  host_numpy / host_philox       ``sieve(device=False)``: the same algorithm vectorised in NumPy, the rows uploaded
      (``vbmc_sieve_put``), scored and ranked on the device.
  statement                      the route ``dropin.make_sieve`` takes, as far as it exists without PyVBMC: the candidates
      one at a time by the reference's NumPy statements (tests/sieve_host.py ``candidates_host``: ``_vb_init``,
      ``get_parameters``, ``set_parameters``, WITHOUT the reference's ``copy.deepcopy(vp)`` per candidate and its object
      construction), then ONE ``_neg_elcbo_batch`` call and ``np.argsort``.  Where PyVBMC is not installed
      this row stands in for the reference's own ``_sieve`` and is a lower bound of its host time.
``order_equal``: device_numpy, host_numpy and statement rank the candidates identically under the same NumPy seed.
Every shape runs in a fresh child process under ``timeout -k 10 <--limit>``; after a child that does not exit with 0
nothing further is started and the tool exits with that status."""
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

SHAPES = ((3, 2500), (5, 5000))
OPTIONS = {"hpd_frac": 0.8, "tol_length": 1e-6, "tol_weight": 1e-2, "tol_con_loss": 0.01, "weight_penalty": 0.1,
           "ns_ent": lambda K: 100 + 15 * K, "ns_ent_fast": 0, "ns_elbo": lambda K: 50 * K}


def spread(t):
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def child(cfg, init_N, reps, warm):
    import sieve_host as sh
    from helpers import PlainGP

    from oracle import gp_ref
    from pyvbmc_amd import VariationalPosterior, _lib, synthetic
    from pyvbmc_amd import sieve as sv
    from pyvbmc_amd.variational_optimization import _neg_elcbo_batch

    ctx = _lib.Context(0)
    _lib.set_default_context(ctx)
    wl = synthetic.make_workload(cfg)
    D, K = wl.D, wl.K
    gp = PlainGP(gp_ref.make_gp(wl.X, wl.y, wl.hyp, gp_ref.MEAN_NEGQUAD))
    gp._ctx = ctx
    vp = VariationalPosterior(D, K)
    vp.mu, vp.sigma, vp.lambd = wl.mu.copy(), wl.sigma.reshape(1, -1).copy(), wl.lambd.reshape(-1, 1).copy()
    vp.w, vp.eta = wl.w.reshape(1, -1).copy(), wl.eta.reshape(1, -1).copy()
    vp.ctx = ctx
    state = {"entropy_switch": False}
    n3 = -(-init_N // 3)
    counts = (n3, n3, init_N - 2 * n3)
    X_star, y_star = sv.get_hpd(gp.X, gp.y, OPTIONS["hpd_frac"])[:2]
    row = {"cfg": cfg, "D": D, "K": K, "N": int(wl.X.shape[0]), "init_N": init_N, "N_star": int(X_star.shape[0]), "routes": {}}
    orders = {}

    def phases(rng, device, timed):
        """One sieve call in its phases (what ``sieve`` does, clocked between them)."""
        np.random.seed(11)
        ctx.set_timing(1 if timed else 0)
        t0 = time.perf_counter()
        bnd = vp.get_bounds(gp.X, OPTIONS, K)
        cand = sv._generate(vp, counts, K, X_star, y_star, rng, 5, device, ctx, want_thetas=False)
        ctx.synchronize()
        t1 = time.perf_counter()
        order, _ = sv.score(cand, gp, bnd, ctx=ctx, put=not device)
        t2 = time.perf_counter()
        vps, types = cand.to_vps()[order], cand.types[order]
        t3 = time.perf_counter()
        out = {"generate_ms": 1e3 * (t1 - t0), "eval_ms": 1e3 * (t2 - t1), "to_vps_ms": 1e3 * (t3 - t2)}
        if timed:
            if device:
                out["fill_ms"] = ctx.last_kernel_ms(_lib.T_SIEVE_FILL)
            out["score_ms"], out["rank_ms"] = ctx.last_kernel_ms(_lib.T_SIEVE_SCORE), ctx.last_kernel_ms(_lib.T_SIEVE_RANK)
            out["download_ms"] = out["eval_ms"] - out["score_ms"] - out["rank_ms"]
        ctx.set_timing(0)
        assert len(vps) == init_N and len(types) == init_N
        return out, order

    for name, rng, device in (("device_numpy", "numpy", True), ("device_philox", "philox", True),
                              ("host_numpy", "numpy", False), ("host_philox", "philox", False)):
        whole, parts, timed = [], [], None
        for i in range(warm + reps):
            np.random.seed(11)
            t0 = time.perf_counter()
            out = sv.sieve(OPTIONS, state, vp, gp, init_N, 2, K, rng=rng, seed=5, device=device, ctx=ctx, return_candidates=True)
            dt = 1e3 * (time.perf_counter() - t0)
            p, order = phases(rng, device, False)
            if i >= warm:
                whole.append(dt)
                parts.append(p)
            assert np.array_equal(out[7], order)
        timed, _ = phases(rng, device, True)
        orders[name] = order
        r = {"sieve_ms": spread(whole)}
        for k in ("generate_ms", "eval_ms", "to_vps_ms"):
            r[k] = spread([p[k] for p in parts])
        for k in ("fill_ms", "score_ms", "rank_ms", "download_ms"):
            if k in timed:
                r[k] = timed[k]
        row["routes"][name] = r
        print(cfg, name, "sieve_ms %.2f" % r["sieve_ms"]["median"], flush=True)

    # the per-candidate NumPy statement + one batched device call
    base = {"mu": vp.mu, "sigma": vp.sigma, "lambd": vp.lambd, "w": vp.w, "eta": vp.eta}
    whole, gen, ev = [], [], []
    for i in range(warm + reps):
        np.random.seed(11)
        t0 = time.perf_counter()
        bnd = vp.get_bounds(gp.X, OPTIONS, K)
        _, thetas, _, types = sh.candidates_host(base, (1, 1, 1, 1), counts, K, X_star, y_star, sh.NumpySource())
        t1 = time.perf_counter()
        F = _neg_elcbo_batch(thetas, gp, vp, bnd, ctx=ctx)
        order = np.argsort(F)
        t2 = time.perf_counter()
        if i >= warm:
            whole.append(1e3 * (t2 - t0))
            gen.append(1e3 * (t1 - t0))
            ev.append(1e3 * (t2 - t1))
    orders["statement"] = order
    row["routes"]["statement"] = {"sieve_ms": spread(whole), "generate_ms": spread(gen), "eval_ms": spread(ev)}
    print(cfg, "statement", "sieve_ms %.2f" % statistics.median(whole), flush=True)
    row["order_equal"] = bool(np.array_equal(orders["device_numpy"], orders["host_numpy"])
                              and np.array_equal(orders["device_numpy"], orders["statement"]))
    row["ratio_statement_over_device_numpy"] = (row["routes"]["statement"]["sieve_ms"]["median"]
                                                / row["routes"]["device_numpy"]["sieve_ms"]["median"])
    row["ratio_statement_over_device_philox"] = (row["routes"]["statement"]["sieve_ms"]["median"]
                                                 / row["routes"]["device_philox"]["sieve_ms"]["median"])
    info = ctx.device_info()
    ctx.close()
    print("ROW " + json.dumps({"device": info["name"], "row": row}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sieve_rows.json"))
    ap.add_argument("--child", nargs=2, type=int)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.reps, a.warm)
        return 0
    rows, device = [], None
    for cfg, init_N in SHAPES:
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, __file__, "--reps", str(a.reps), "--warm",
                            str(a.warm), "--child", str(cfg), str(init_N)], stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            return p.returncode
        rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")][-1][4:])
        rows.append(rec["row"])
        device = rec["device"]
    Path(a.out).write_text(json.dumps({"tool": "tools/sieve_rows.py", "reps": a.reps, "warm": a.warm, "device": device,
                                       "statement_route": "tests/sieve_host.candidates_host (the reference's statements per "
                                       "candidate, no deepcopy, no objects) + one _neg_elcbo_batch call: PyVBMC was not "
                                       "installed where this was measured", "rows": rows}, indent=1) + "\n")
    print(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
