#!/usr/bin/env python
"""Trajectories of the optimiser loop and the ELBO calls that share its theta block map, for a fixed list of small cases,
written to an .npz: run once per library (VBMC_HIP_LIB names the one to load, as in tools/ab_libs.sh) and compare.
    VBMC_HIP_LIB=$PWD/variants/libvbmc_parent.so python tools/adam_traj_dump.py parent.npz
    python tools/adam_traj_dump.py new.npz
    python tools/adam_traj_dump.py --compare parent.npz new.npz      # np.array_equal per array; exit status 1 on a mismatch
The cases are the smallest shapes that reach the step kernel, the tail kernel (writer and non-writer blocks), the fused
kernel (NU = 2 and 3, the stopping rule on the device), the stand-alone pre launch, the global-memory kernels, the partial
masks with active soft bounds, and vbmc_neg_elcbo / vbmc_neg_elcbo_batch under all sixteen masks."""
import itertools
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SCHED = dict(master_min=0.001, master_max=0.1, master_decay=200)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    cases = {}
    for k in sorted(set(A.files) & set(B.files)):
        same = A[k].shape == B[k].shape and np.array_equal(A[k], B[k])
        cases.setdefault(k.split("/")[0], []).append(same)
        if not same:
            bad.append(k)
    for c, v in cases.items():
        print(f"{c}: {len(v)} arrays, {'equal' if all(v) else 'NOT equal'}")
    print("ALL EQUAL" if not bad else f"MISMATCH: {bad}")
    return 1 if bad else 0


def main(out):
    from oracle import mixture_ref
    from pyvbmc_amd import VariationalPosterior, _lib, synthetic
    from pyvbmc_amd import gp as gpm
    from pyvbmc_amd.minimize_adam import minimize_adam_elbo
    from pyvbmc_amd.variational_optimization import _neg_elcbo, _neg_elcbo_batch

    ctx = _lib.Context(0)
    res = {}

    def objects(wl, flags=None):
        vp = VariationalPosterior(wl.D, wl.K)
        vp.mu, vp.sigma, vp.lambd = wl.mu.copy(), wl.sigma.reshape(1, -1).copy(), wl.lambd.reshape(-1, 1).copy()
        vp.w, vp.eta = wl.w.reshape(1, -1).copy(), wl.eta.reshape(1, -1).copy()
        vp.ctx = ctx
        if flags is not None:
            vp.optimize_mu, vp.optimize_sigma, vp.optimize_lambd, vp.optimize_weights = flags
        s2 = wl.s2 if wl.s2 is not None and np.size(wl.s2) else None
        gp = gpm.GP(wl.D, gpm.SquaredExponential(), gpm.NegativeQuadratic(),
                    gpm.GaussianNoise(constant_add=True, user_provided_add=s2 is not None))
        gp.ctx = ctx
        gp.update(X_new=wl.X, y_new=wl.y, s2_new=s2, hyp=wl.hyp)
        return vp, gp

    def workload(s):
        return synthetic.make_workload(s["cfg"], S=s["S"], D=s["D"], K=s["K"], N=s["N"], Ns_total=s["NsK"] * s["K"])

    def loop(tag, wl, theta0, bnd, flags=None, **kw):
        vp, gp = objects(wl, flags)
        r = minimize_adam_elbo(theta0.copy(), gp, vp, wl.NsK, bnd, rng="philox", return_parts=True, **SCHED, **kw)
        for name, v in zip(("x", "y", "x_tab", "y_tab", "iterations", "G", "H"), r):
            res[f"{tag}/{name}"] = np.asarray(v)
        for name in ("mu", "sigma", "lambd", "w", "eta"):
            res[f"{tag}/vp_{name}"] = np.asarray(getattr(vp, name)).copy()
        res[f"{tag}/kernel"] = np.array(str(ctx.last_entmc_plan()["kernel"]))

    def masked_bounds(wl, flags):
        full = synthetic.default_theta_bnd(wl)
        DK, K = wl.D * wl.K, wl.K
        keep = np.concatenate([np.full(DK, flags[0]), np.full(DK, flags[1] or flags[2]), np.full(K, flags[3])])
        out = dict(full)
        out["lb"], out["ub"] = full["lb"][keep], full["ub"][keep]
        return out

    # the step kernel and the tail kernel: TAIL_SHAPES[0] of tests/test_adam.py, with a box
    tail = dict(cfg=2, D=6, K=20, N=60, S=2, NsK=9000)
    wl = workload(tail)
    th = wl.theta.copy()
    th[1] += 3.0
    for form in (2, 0):
        ctx.set_option("adam_tail", form)
        loop(f"tail{form}", wl, th, synthetic.default_theta_bnd(wl), lb=th - 0.05, ub=th + 0.02, max_iter=27, seed=77,
             tol_fun=0.05, use_early_stopping=False)
    ctx.set_option("adam_tail", 1)
    # the fused kernel: FUSED_SHAPES[2] and [9] (the NU = 3 build), against the four-launch iteration
    for i, s in ((2, dict(cfg=2, D=4, K=20, N=200, S=2, NsK=22)), (9, dict(cfg=5, D=20, K=50, N=400, S=1, NsK=22))):
        wl = workload(s)
        th = wl.theta.copy()
        th[0] += 4.0
        for fused in (1, 0):
            ctx.set_option("adam_fused", fused)
            loop(f"fused{i}_{fused}", wl, th, synthetic.default_theta_bnd(wl), max_iter=47, seed=77, tol_fun=1e-9)
        ctx.set_option("adam_fused", 1)
        # (those ran through vbmc_adam_run_auto where fused; this one through vbmc_adam_run's one-launch batches, rule on the host)
        loop(f"fused{i}_batches", wl, th, synthetic.default_theta_bnd(wl), max_iter=47, seed=77, tol_fun=1e-9, device_stop=False)
        if i == 2:  # vbmc_adam_run_auto: the stopping rule on the device
            loop("fused2_auto", wl, th, synthetic.default_theta_bnd(wl), max_iter=170, seed=21, tol_fun=0.05, device_stop=True)
    # the stand-alone pre launch (K > 128) and the global-memory step kernel
    for tag, s, n_it in (("pre_alone", dict(cfg=5, D=3, K=130, N=40, S=1, NsK=6), 30),
                         ("global", dict(cfg=5, D=20, K=100, N=60, S=1, NsK=24), 12)):
        wl = workload(s)
        th = wl.theta.copy()
        th[1] += 4.0
        loop(tag, wl, th, synthetic.default_theta_bnd(wl), max_iter=n_it, seed=31, tol_fun=0.05)
    # the partial masks of test_device_loop_partial_masks on c2s, soft bounds active
    c2s = synthetic.make_workload(2, Ns_total=20 * 100)
    for flags in ((True, True, True, False), (True, True, False, True), (False, True, True, True)):
        mix = mixture_ref.Mixture.make(c2s.mu, c2s.sigma, c2s.lambd, c2s.w, c2s.eta)
        mix.optimize_mu, mix.optimize_sigma, mix.optimize_lambd, mix.optimize_weights = flags
        th = mixture_ref.get_parameters(mix)
        th[0] += 5.0
        loop("mask" + "".join("01"[f] for f in flags), c2s, th, masked_bounds(c2s, flags), flags=flags, max_iter=40, seed=99,
             tol_fun=0.05)
    # vbmc_neg_elcbo (F, dF, G, H) and vbmc_neg_elcbo_batch (F, G, H of 8 candidates) under every mask, with bounds
    rng = np.random.default_rng(5)
    for flags in itertools.product((False, True), repeat=4):
        if not any(flags):
            continue
        tag = "elbo" + "".join("01"[f] for f in flags)
        mix = mixture_ref.Mixture.make(c2s.mu, c2s.sigma, c2s.lambd, c2s.w, c2s.eta)
        mix.optimize_mu, mix.optimize_sigma, mix.optimize_lambd, mix.optimize_weights = flags
        th = mixture_ref.get_parameters(mix)
        th[0] += 5.0
        bnd = masked_bounds(c2s, flags)
        vp, gp = objects(c2s, flags)
        F, dF, G, H, _ = _neg_elcbo(th.copy(), gp, vp, 0.0, c2s.NsK, True, False, bnd, rng="philox", seed=3)
        res[f"{tag}/F"], res[f"{tag}/dF"], res[f"{tag}/G"], res[f"{tag}/H"] = (np.asarray(v) for v in (F, dF, G, H))
        vp, gp = objects(c2s, flags)
        thetas = th[None, :] + 0.3 * rng.standard_normal((8, th.size))
        Fb, Gb, Hb = _neg_elcbo_batch(thetas, gp, vp, bnd, return_parts=True)[:3]
        res[f"{tag}/batch_F"], res[f"{tag}/batch_G"], res[f"{tag}/batch_H"] = np.asarray(Fb), np.asarray(Gb), np.asarray(Hb)
    ctx.close()
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    np.savez(out, **res)
    print(f"{out}: {len(res)} arrays from {_lib.LIB_PATH}")


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main(sys.argv[1])
