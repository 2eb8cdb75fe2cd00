#!/usr/bin/env python
"""Wall-clock milliseconds of ``optimize_vp``'s last stage through the new entry points, next to the route they replace.

    python tools/optimize_vp_rows.py [--reps 7] [--warm 2] [--out profiles/optimize_vp_rows.json]

Shapes: BASELINE config 3 (D = 10, K = 50, N = 400) and config 5 (D = 20, K = 100, N = 800),
``pyvbmc_amd.synthetic.make_workload``'s data, negative-quadratic mean, S = 1 and S = 8 hyper-parameter samples, all four
blocks optimised, ``ns_ent_fine = 2**12 K`` (the default), Philox draws.  Per (shape, S), medians over --reps calls after
--warm, with [min, max]; every call ends in its own stream wait.

  full_ms        one full evaluation: ``vbmc_elcbo_full`` (theta -> mixture, GP sums and variance, entropy, statistics).
  full_composed_ms   the same evaluation on the route it replaces: ``_neg_elcbo(..., compute_var=True, separate_K=True)``.
  trial_ms       one pruning trial: ``vbmc_elcbo_prune_trial`` of a middle component (not accepted: every rep is the same trial).
  trial_composed_ms  the route it replaces: ``_neg_elcbo(theta_pruned, gp, vp_pruned, 0, ns, False, True, None, 0, True)`` on
                 the pruned posterior, timed in the same process.
  gp_launches_per_trial, waits_per_trial (and ``*_composed``)   ``vbmc_elcbo_record_info``'s counters around the timed
                 trials: launches of the GP expected log joint (the sums' launch, the variance product, the gram kernel)
                 and stream waits of the context, per trial, on either route.
  whole_ms       the whole ``optimize_vp`` call (``fast_opts_N = 50 K``, one slow start, ``max_iter_stochastic = 100 (2 + D)``,
                 ``tol_weight = 0.01``; --whole-reps calls after one warm-up), with ``pruned`` and the number of trials.
The waits and the GP launches are counted; the other launches of a trial are not instrumented and are read off the entry's
code (csrc/api_elcbo_full.hip): the mixture pack's upload, the entropy's three launches, the re-weighting's two, two small
uploads (weights, alive list), two small downloads (H; G, varG, var_ss).
Every (shape, S) runs in a fresh child process under ``timeout -k 10 <--limit>``; after a child that does not exit with 0
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

SHAPES = ((3, 1), (3, 8), (5, 1), (5, 8))


def spread(t):
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def options_for(D):
    return {"hpd_frac": 0.8, "tol_length": 1e-6, "tol_weight": 1e-2, "tol_con_loss": 0.01, "weight_penalty": 0.1,
            "ns_ent": lambda K: 100 * K ** (2 / 3), "ns_ent_fast": 0, "ns_elbo": lambda K: 50 * K,
            "ns_ent_fine": lambda K: 2**12 * K, "stochastic_optimizer": "adam", "sgd_step_size": 0.005,
            "tol_fun_stochastic": 1e-3, "max_iter_stochastic": 100 * (2 + D), "elcbo_midpoint": True,
            "det_entropy_tol_opt": 1e-3, "elcbo_impro_weight": 3, "tol_improvement": 0.01,
            "pruning_threshold_multiplier": lambda K: 1 / np.sqrt(K)}


def child(cfg, S, reps, warm, whole_reps):
    import importlib

    from helpers import PlainGP

    from oracle import gp_ref
    from pyvbmc_amd import VariationalPosterior, _lib, synthetic
    from pyvbmc_amd.variational_optimization import _neg_elcbo

    ov = importlib.import_module("pyvbmc_amd.optimize_vp")
    ctx = _lib.Context(0)
    _lib.set_default_context(ctx)
    wl = synthetic.make_workload(cfg, S=S)
    D, K = wl.D, wl.K
    gp = PlainGP(gp_ref.make_gp(wl.X, wl.y, wl.hyp, gp_ref.MEAN_NEGQUAD))
    gp._ctx = ctx
    opts = options_for(D)

    def fresh_vp():
        vp = VariationalPosterior(D, K)
        vp.mu, vp.sigma, vp.lambd = wl.mu.copy(), wl.sigma.reshape(1, -1).copy(), wl.lambd.reshape(-1, 1).copy()
        vp.w, vp.eta = wl.w.reshape(1, -1).copy(), wl.eta.reshape(1, -1).copy()
        vp.ctx = ctx
        return vp

    vp = fresh_vp()
    theta0 = vp.get_parameters()
    row = {"cfg": cfg, "D": D, "K": K, "N": int(wl.X.shape[0]), "S": S}
    stage = ov._Stage(ctx, gp, opts, "philox", ov._Seeds(77), True)
    ns = stage.ns(K)
    row["ns_per_comp"] = ns

    def timed(fn, n_warm, n):
        t = []
        for i in range(n_warm + n):
            ctx.synchronize()
            t0 = time.perf_counter()
            r = fn()
            dt = 1e3 * (time.perf_counter() - t0)
            if i >= n_warm:
                t.append(dt)
        return spread(t), r

    row["full_ms"], (out, I, J) = timed(lambda: stage.full(1, theta0.copy(), vp), warm, reps)
    vp_c = fresh_vp()  # (one object for every repeat, like the device side: _neg_elcbo at the same theta leaves it as it finds it)
    row["full_composed_ms"], r11 = timed(
        lambda: _neg_elcbo(theta0.copy(), gp, vp_c, 0, ns, False, True, None, 0.0, True, rng="philox", seed=78, ctx=ctx), warm, reps)
    row["full_G_rel_diff"] = float(abs(out[1] - r11[2]) / abs(r11[2]))
    # one trial: the record of the last device evaluation, a middle component
    vp.set_parameters(theta0)
    out, I, J = stage.full(1, theta0.copy(), vp)
    pos = K // 2
    vp_pruned, theta_pruned = ov._prune_vp(vp, pos)
    alive = list(range(K))
    alive.pop(pos)
    stage.trial(vp_pruned, alive, pos)  # (buffers grown)
    i0 = stage.record_info()
    row["trial_ms"], t_out = timed(lambda: stage.trial(vp_pruned, alive, pos), warm, reps)
    i1 = stage.record_info()
    row["gp_launches_per_trial"] = (i1["gp_launches"] - i0["gp_launches"]) / (warm + reps)
    row["waits_per_trial"] = (i1["waits"] - i0["waits"]) / (warm + reps) - 1  # (timed()'s own synchronize is one of them)
    ns1 = stage.ns(K - 1)
    row["trial_composed_ms"], r11 = timed(
        lambda: _neg_elcbo(theta_pruned.copy(), gp, vp_pruned, 0, ns1, False, True, None, 0.0, True, rng="philox", seed=79, ctx=ctx),
        warm, reps)
    i2 = stage.record_info()  # (the composed calls leave the record alone: its counters go on)
    row["gp_launches_per_trial_composed"] = (i2["gp_launches"] - i1["gp_launches"]) / (warm + reps)
    row["waits_per_trial_composed"] = (i2["waits"] - i1["waits"]) / (warm + reps) - 1
    row["trial_G_rel_diff"] = float(abs(t_out[1] - r11[2]) / abs(r11[2]))
    row["trial_varG_diff"] = float(abs(t_out[4] - np.ravel(r11[7])[0]))
    row["ratio_trial_composed_over_device"] = row["trial_composed_ms"]["median"] / row["trial_ms"]["median"]
    row["ratio_full_composed_over_device"] = row["full_composed_ms"]["median"] / row["full_ms"]["median"]
    print(cfg, S, "full %.3f (composed %.3f) trial %.3f (composed %.3f) ms" % (
        row["full_ms"]["median"], row["full_composed_ms"]["median"], row["trial_ms"]["median"], row["trial_composed_ms"]["median"]),
          flush=True)
    # the whole call
    n_trials = [0]
    orig_trial = ov._Stage.trial

    def counting(self, *a):
        n_trials[0] += 1
        return orig_trial(self, *a)

    ov._Stage.trial = counting
    state = {"warmup": False, "entropy_switch": False}

    def whole():
        n_trials[0] = 0
        return ov.optimize_vp(opts, state, fresh_vp(), gp, 50 * K, 1, K, rng="philox", seed=5, ctx=ctx)

    row["whole_ms"], (vp1, _, pruned) = timed(whole, 1, whole_reps)
    row["whole_pruned"], row["whole_trials"], row["whole_elbo"] = int(pruned), n_trials[0], float(vp1.stats["elbo"])
    print(cfg, S, "whole %.1f ms, pruned %d of %d trials" % (row["whole_ms"]["median"], pruned, n_trials[0]), flush=True)
    info = ctx.device_info()
    ctx.close()
    print("ROW " + json.dumps({"device": info["name"], "row": row}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--whole-reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "optimize_vp_rows.json"))
    ap.add_argument("--child", nargs=2, type=int)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.reps, a.warm, a.whole_reps)
        return 0
    rows, device = [], None
    for cfg, S in SHAPES:
        p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, __file__, "--reps", str(a.reps), "--warm",
                            str(a.warm), "--whole-reps", str(a.whole_reps), "--child", str(cfg), str(S)], stdout=subprocess.PIPE,
                           text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            return p.returncode
        rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")][-1][4:])
        rows.append(rec["row"])
        device = rec["device"]
    Path(a.out).write_text(json.dumps({"tool": "tools/optimize_vp_rows.py", "reps": a.reps, "warm": a.warm,
                                       "whole_reps": a.whole_reps, "device": device, "rows": rows}, indent=1) + "\n")
    print(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
