#!/usr/bin/env python
"""Generate tests/golden/sieve.npz by RUNNING THE REFERENCE's ``_sieve``, ``_vb_init`` and ``get_hpd``
(vbmc/variational_optimization.py:660-988, stats/get_hpd.py).  TEST INFRASTRUCTURE, like
tools/make_active_sample_golden.py: it runs only where the reference checkout is present (VBMC_REFERENCE, default
/root/reference), imports it at run time, with oracle/_stubs for the packages it needs, and stores numbers only.

    python tools/make_sieve_golden.py                   # rewrites tests/golden/sieve.npz
    python tools/make_sieve_golden.py --batch FILE.npz  # copies FILE's ``<case>_batch_F/G/H`` arrays into the fixture

``<case>_batch_F/G/H`` are ``vbmc_neg_elcbo_batch``'s outputs on the case's thetas, recorded on an MI355X from the build
before the evaluator's scoring part was factored out (tests/test_sieve_gpu.py pins them bit for bit); they cannot be made
here, so a rewrite keeps those of every case whose thetas did not change.

Shapes (D, K, K_new, N): (2, 2, 2, 20), (2, 2, 4, 20), (3, 1, 1, 20) and (3, 1, 3, 20) -- the ``K == 1`` variance branch --
and (2, 3, 5, 5), where N_star = 4 < K_new: the cycling branch.  hpd_frac = 0.8, so N_star = 16 or 4.  Each shape runs
``init_N = 7, best_N = 3`` (split 3 / 3 / 1) and ``init_N = 4, best_N = 1``, with the optimise flags all on, weights off
(warm-up), lambd off, and -- where K_new == K -- mu off.  The GP is the gpyreg stand-in on
``pyvbmc_amd.synthetic.make_workload``'s data (negative-quadratic mean, one hyper-parameter sample).

Per case: the inputs (base posterior, flags, X, y, hyper-parameters, the option values read), the NumPy seed, every
candidate's ``mu, sigma, lambd, w, eta`` as ``_vb_init`` returns it (``raw_*``, candidate order) and as the sieve leaves it
after ``get_parameters`` / ``_neg_elcbo`` (``fin_*``), the theta rows, the types, the scores (the reference's
``_neg_elcbo``, candidate order), the order, and the MT19937 state afterwards.  ``hpd_*``: ``get_hpd`` on three inputs,
one with ``hpd_N = 0``.

Asserted while generating, or the file is not written: in every case adjacent entries of the sorted scores differ by
more than 1e-6 max(1, |F|), so the recorded order is a fair yardstick for a scorer that is right to 1e-10.  A case whose
seed fails that is re-run with the next seed; the seed used is stored.
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("VBMC_REFERENCE", "/root/reference"))
sys.path.insert(0, str(ROOT / "oracle" / "_stubs"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(REF))
sys.path.insert(0, str(ROOT / "tests"))

OUT = ROOT / "tests" / "golden" / "sieve.npz"
SHAPES = ((2, 2, 2, 20), (2, 2, 4, 20), (3, 1, 1, 20), (3, 1, 3, 20), (2, 3, 5, 5))
RUNS = ((7, 3), (4, 1))
MIN_GAP = 1e-6
ATTRS = ("mu", "sigma", "lambd", "w", "eta")


def main():
    import gpyreg as gpr  # the stand-in
    import pyvbmc.vbmc.variational_optimization as vo
    import sieve_host as sh
    from pyvbmc.stats import get_hpd
    from pyvbmc.variational_posterior import VariationalPosterior as RefVP
    from pyvbmc.vbmc import Options
    from pyvbmc_amd import synthetic

    def setup_options(D):
        base = REF / "pyvbmc" / "vbmc" / "option_configs"
        o = Options(str(base / "basic_vbmc_options.ini"), evaluation_parameters={"D": D}, user_options={})
        o.load_options_file(str(base / "advanced_vbmc_options.ini"), evaluation_parameters={"D": D})
        return o

    out = {}
    names = []
    for D, K, Kn, N in SHAPES:
        wl = synthetic.make_workload(2, D=D, K=K, N=N)
        gp = gpr.GP(D=D, covariance=gpr.covariance_functions.SquaredExponential(), mean=gpr.mean_functions.NegativeQuadratic(),
                    noise=gpr.noise_functions.GaussianNoise(constant_add=True))
        gp.update(X_new=wl.X, y_new=wl.y, hyp=wl.hyp)
        options = setup_options(D)
        for fname, flags in sh.FLAG_SETS.items():
            if fname == "nomu" and Kn != K:
                continue
            for init_N, best_N in RUNS:
                name = f"d{D}k{K}n{Kn}_{fname}_{init_N}"
                seed = 100 + len(names)
                while True:
                    c = run_case(vo, RefVP, wl, gp, options, flags, Kn, init_N, best_N, seed)
                    F = np.sort(c["F"])
                    gaps = np.diff(F) / np.maximum(1.0, np.abs(F[1:]))
                    if np.all(np.isfinite(F)) and np.all(gaps > MIN_GAP):
                        break
                    print(name, "seed", seed, "min gap", gaps.min(), "-> next seed", flush=True)
                    seed += 1
                    assert seed < 100 + len(names) + 50, name
                c["options"] = np.array([float(options.eval(k, {"K": Kn})) if k in ("ns_ent", "ns_ent_fast", "ns_elbo")
                                         else float(options[k]) for k in sh.OPTION_KEYS])
                c["shape"] = np.array([D, K, Kn, N, init_N, best_N])
                c["flags"] = np.array(flags)
                print(name, "seed", seed, "min gap %.2e" % gaps.min(), "order", c["order"], flush=True)
                names.append(name)
                for k, v in c.items():
                    out[f"{name}_{k}"] = np.asarray(v)
    # get_hpd: the default fraction, a small one, and one that rounds to an empty set
    r = np.random.default_rng(5)
    for i, (n, frac) in enumerate(((12, 0.8), (9, 0.3), (3, 0.1))):
        X, y = r.standard_normal((n, 2)), r.standard_normal((n, 1))
        hX, hy, hr, hi = get_hpd(X, y, frac)
        out.update({f"hpd{i}_X": X, f"hpd{i}_y": y, f"hpd{i}_frac": np.array(frac), f"hpd{i}_hX": hX, f"hpd{i}_hy": hy,
                    f"hpd{i}_range": hr, f"hpd{i}_idx": hi})
    out["cases"] = np.array(names)
    if OUT.exists():  # the recorded device values of a case whose thetas did not change stay (they cannot be made here)
        old = np.load(OUT)
        for name in names:
            if f"{name}_batch_F" in old.files and np.array_equal(old[f"{name}_thetas"], out[f"{name}_thetas"]):
                for q in ("batch_F", "batch_G", "batch_H"):
                    out[f"{name}_{q}"] = old[f"{name}_{q}"]
    for k, v in out.items():
        assert v.dtype != object, k  # arrays of numbers and names only
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes,", len(names), "cases")


def run_case(vo, RefVP, wl, gp, options, flags, Kn, init_N, best_N, seed):
    vp = RefVP(wl.D, wl.K)
    vp.mu = wl.mu.copy()
    vp.sigma, vp.lambd = wl.sigma.reshape(1, -1).copy(), wl.lambd.reshape(-1, 1).copy()
    vp.w, vp.eta = wl.w.reshape(1, -1).copy(), wl.eta.reshape(1, -1).copy()
    vp.optimize_mu, vp.optimize_sigma, vp.optimize_lambd, vp.optimize_weights = (bool(f) for f in flags)
    c = {"base_" + a: np.array(getattr(vp, a), dtype=np.float64) for a in ATTRS}
    c.update(X=np.array(gp.X), y=np.array(gp.y), hyp=np.array(wl.hyp), seed=np.array(seed))
    raw, scores, thetas = [], [], []
    ref_init, ref_elcbo = vo._vb_init, vo._neg_elcbo

    def rec_init(*a, **kw):
        vps, types = ref_init(*a, **kw)
        raw.extend({x: np.array(getattr(v, x), dtype=np.float64) for x in ATTRS} for v in vps)
        return vps, types

    def rec_elcbo(theta, *a, **kw):
        res = ref_elcbo(theta, *a, **kw)
        scores.append(float(res[0]))
        thetas.append(np.array(theta, dtype=np.float64))  # (after the call: the eta tail is shifted in place)
        return res

    optim_state = {"warmup": False, "entropy_switch": False, "delta": np.zeros((1, wl.D))}
    vo._vb_init, vo._neg_elcbo = rec_init, rec_elcbo
    try:
        np.random.seed(seed)
        vps, types, beta, cvar, ns_ent_K, ns_ent_K_fast = vo._sieve(options, optim_state, vp, gp, init_N, best_N, Kn)
        st = np.random.get_state(legacy=True)
    finally:
        vo._vb_init, vo._neg_elcbo = ref_init, ref_elcbo
    B = len(raw)
    assert len(scores) == B == len(vps) and ns_ent_K_fast == 0 and beta == 0
    F = np.array(scores)
    order = np.argsort(F)
    assert np.array_equal(types, np.concatenate([t * np.ones(n) for t, n in zip((1, 2, 3), split_of(init_N, best_N))])[order])
    inv = np.empty(B, dtype=int)
    inv[order] = np.arange(B)
    for a in ATTRS:
        c["raw_" + a] = np.stack([r[a] for r in raw])
        c["fin_" + a] = np.stack([np.array(getattr(vps[inv[b]], a), dtype=np.float64).reshape(raw[b][a].shape) for b in range(B)])
    c.update(thetas=np.stack(thetas), F=F, order=order, types=np.asarray(types)[inv], ns_ent_K=np.array(ns_ent_K),
             mt_key=np.array(st[1], dtype=np.uint32), mt_pos=np.array(st[2]), mt_has_gauss=np.array(st[3]),
             mt_gauss=np.array(st[4]))
    return c


def split_of(init_N, best_N):
    import sieve_host as sh

    return sh.split(init_N, best_N)


def merge_batch(path):
    z = dict(np.load(OUT))
    add = np.load(path)
    n = 0
    for k in add.files:
        if k.endswith(("_batch_F", "_batch_G", "_batch_H")):
            z[k] = add[k]
            n += 1
    np.savez_compressed(OUT, **z)
    print(OUT, OUT.stat().st_size, "bytes,", n, "batch arrays merged")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--batch":
        merge_batch(sys.argv[2])
    else:
        main()
