#!/usr/bin/env python
"""Generate tests/golden/ais_mcmc.npz by RUNNING THE REFERENCE's ``active_importance_sampling`` through its MCMC
step (pyvbmc/vbmc/active_importance_sampling.py:195-262).  TEST INFRASTRUCTURE, like oracle/make_golden.py and
tools/make_transform_golden.py: it runs only where the reference checkout is present (REF below, or the
VBMC_REFERENCE environment variable), imports it at run time with oracle/_stubs standing in for gpyreg, and stores
numbers only -- the inputs, the ``np.random`` seed and the reference's outputs.

    python tools/make_ais_golden.py        # rewrites tests/golden/ais_mcmc.npz

The stub package's ``SliceSampler`` is import-only, so the deterministic stand-in of tests/ais_host.py
(``StandInSampler``: moves that do not depend on ``log_p``) is bound to ``gpyreg.slice_sample.SliceSampler`` at run
time: the file pins the function's data flow around the sampler -- resampling weights, ``np.random.choice``, the
clipped start, burn-in and thinning, ``ln_weights = ln_y - log_p``, the per-sample products -- not a sampler.

Case: IMIQR, D = 3, N = 60, S = 2, 30 + 18 proposals, mcmc_samples = 12, thin = 2.  The seed is the first whose
``np.random.choice`` draws all lie at least 1e-6 from every boundary of the cumulative weights, so that a
restatement whose weights differ in the last bits picks the same start points.
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("VBMC_REFERENCE", "/root/reference"))
sys.path.insert(0, str(ROOT / "oracle" / "_stubs"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(REF))

import gpyreg as gpr  # noqa: E402  (the stand-in)
from pyvbmc.acquisition_functions import AcqFcnIMIQR  # noqa: E402
from pyvbmc.variational_posterior import VariationalPosterior  # noqa: E402
from pyvbmc.vbmc.active_importance_sampling import active_importance_sampling  # noqa: E402

import ais_host  # noqa: E402

OUT = ROOT / "tests" / "golden" / "ais_mcmc.npz"
D, N, S, K = 3, 60, 2, 2
OPTS = dict(active_importance_sampling_vp_samples=30, active_importance_sampling_box_samples=18,
            active_importance_sampling_mcmc_samples=12, active_importance_sampling_mcmc_thin=2)
MARGIN = 1e-6


def inputs():
    rng = np.random.default_rng(777)
    X = rng.standard_normal((N, D))
    y = (-0.5 * np.sum(X**2, axis=1) + 0.2 * np.cos(1.5 * X[:, 1]) + 0.05 * rng.standard_normal(N)).reshape(-1, 1)
    hyp = np.array([np.concatenate([np.log(np.array([0.9, 1.2, 1.0]) * (1.0 + 0.3 * i)), [np.log(1.8 + 0.4 * i)], [ls],
                                    [0.2], 0.1 * np.ones(D), np.log(2.0) * np.ones(D)])
                    for i, ls in enumerate((np.log(0.05), np.log(0.09)))])
    mu = np.array([[0.2, -0.5], [-0.3, 0.4], [0.1, 0.3]])
    sigma = np.array([0.5, 0.8])
    lambd = np.array([1.1, 0.9, 1.0])
    lambd = lambd / np.sqrt(np.mean(lambd**2))
    w = np.array([0.4, 0.6])
    return X, y, hyp, mu, sigma, lambd, w


def run(seed, X, y, hyp, mu, sigma, lambd, w):
    """The reference's result for ``seed`` and the smallest distance of a choice draw from a cdf boundary."""
    gp = gpr.GP(D=D, covariance=gpr.covariance_functions.SquaredExponential(),
                mean=gpr.mean_functions.NegativeQuadratic(), noise=gpr.noise_functions.GaussianNoise(constant_add=True))
    gp.update(X_new=X, y_new=y, s2_new=None, hyp=hyp)
    vp = VariationalPosterior(D, K)
    vp.mu, vp.sigma, vp.lambd, vp.w = mu.copy(), sigma.reshape(1, -1).copy(), lambd.reshape(-1, 1).copy(), w.reshape(1, -1).copy()
    vp.eta = np.log(vp.w)
    margins = []
    real_choice = np.random.choice

    def watched_choice(a, size=None, replace=True, p=None):
        if replace or size is not None:
            return real_choice(a, size=size, replace=replace, p=p)
        before = np.random.get_state()
        idx = real_choice(a, size=size, replace=replace, p=p)
        after = np.random.get_state()
        np.random.set_state(before)
        u = np.random.random_sample((1,))[0]  # the one uniform the call consumed
        np.random.set_state(after)
        cdf = np.cumsum(p)
        cdf = cdf / cdf[-1]
        assert int(cdf.searchsorted(u, side="right")) == int(idx), "np.random.choice is not drawn as assumed"
        margins.append(float(np.min(np.abs(cdf - u))))
        return idx

    gpr.slice_sample.SliceSampler = ais_host.StandInSampler
    np.random.choice = watched_choice
    try:
        np.random.seed(seed)
        with np.errstate(all="ignore"):
            res = active_importance_sampling(vp, gp, AcqFcnIMIQR(), ais_host.Opts(OPTS))
    finally:
        np.random.choice = real_choice
    return res, margins


def main():
    args = inputs()
    for seed in range(1, 200):
        res, margins = run(seed, *args)
        if len(margins) == S and min(margins) >= MARGIN:
            break
    else:
        raise SystemExit("no seed keeps the choice draws clear of the cdf boundaries")
    assert len(margins) == S and min(margins) >= MARGIN
    n = OPTS["active_importance_sampling_mcmc_samples"]
    assert res["X"].shape == (S, n, D) and res["f_s2"].shape == (n, S) and res["ln_weights"].shape == (S, n)
    X, y, hyp, mu, sigma, lambd, w = args
    out = dict(X=X, y=y, hyp=hyp, vp_mu=mu, vp_sigma=sigma, vp_lambd=lambd, vp_w=w, seed=seed,
               choice_margin=np.array(margins), **{k: np.int64(v) for k, v in OPTS.items()},
               out_X=res["X"], out_f_s2=res["f_s2"], out_ln_weights=res["ln_weights"], out_K_Xa_X=res["K_Xa_X"],
               out_C_tmp=res["C_tmp"])
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT.name}: seed {seed}, choice margins {margins}, {OUT.stat().st_size} bytes")


if __name__ == "__main__":
    main()
