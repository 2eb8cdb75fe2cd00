"""Targets of the VBMC driver's GPU tests and profile rows (tests/test_vbmc_driver_gpu.py, tools/vbmc_driver_rows.py).
TEST INFRASTRUCTURE.

The problems are those of the reference's own end-to-end tests (testing/vbmc/test_vbmc_optimize.py:98-246), stated here
as formulas: each is ``Case(f, x0, lb, ub, plb, pub, lnZ, mu_bar, options)`` with the true log normalisation constant and
posterior mean, against which the reference asserts ``RMS(mean error) < 0.5`` and ``|elbo - lnZ| < 0.5``.

  mvn(D)          independent normals with SD 1 .. D, unbounded, plausible box +-2 D, start -1
  half_normal(D)  the same density on (-10 D, 0): lnZ = -D log 2, mean -sqrt(2 / pi) (1 .. D)
  cigar(bounded)  D = 3 correlated normal, SD 1 along one axis and 0.01 across, mean linspace(-0.5, 0.5); the axis is the
                  first column of a fixed rotation built here (the reference tabulates its own matrix)
  uniform()       D = 1, flat on (0, 1), with a flat log-prior passed separately
  noisy(sd)       half_normal(2) observed with Gaussian noise of the reported SD (uncertainty handling level 2)
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "f x0 lb ub plb pub lnZ mu_bar options log_prior")
BASE = {"warp_rotoscaling": False, "display": "off"}  # (input warping is not wired into the loop: refused when on)


def _scaled_normal(x):
    x = np.ravel(x)
    s = np.arange(1, x.size + 1)
    return float(np.sum(-0.5 * (x / s) ** 2) - np.sum(np.log(s)) - 0.5 * x.size * np.log(2 * np.pi))


def mvn(D=2, **options):
    return Case(_scaled_normal, -np.ones((1, D)), np.full((1, D), -np.inf), np.full((1, D), np.inf), np.full((1, D), -2.0 * D),
                np.full((1, D), 2.0 * D), 0.0, np.zeros((1, D)), dict(BASE, **options), None)


def half_normal(D=2, **options):
    return Case(_scaled_normal, -np.ones((1, D)), np.full((1, D), -D * 10.0), np.full((1, D), 0.0), np.full((1, D), -6.0),
                np.full((1, D), -0.05), -D * np.log(2), -2 / np.sqrt(2 * np.pi) * np.arange(1, D + 1).reshape(1, -1),
                dict(BASE, **options), None)


def _cigar_density(D):
    mean = np.linspace(-0.5, 0.5, D)
    R, _ = np.linalg.qr(np.random.default_rng(2024).standard_normal((D, D)))
    ell = np.full(D, 0.01)
    ell[-1] = 1.0
    log_norm = -np.sum(np.log(ell)) - 0.5 * D * np.log(2 * np.pi)

    def f(x):
        z = (R @ (np.ravel(x) - mean)) / ell
        return float(-0.5 * np.sum(z**2) + log_norm)

    return f, mean.reshape(1, -1)


def cigar(bounded=False, **options):
    D = 3
    f, mean = _cigar_density(D)
    lim = 4.0 if bounded else np.inf
    return Case(f, 0.5 * np.ones((1, D)), np.full((1, D), -lim), np.full((1, D), lim), np.full((1, D), -1.0),
                np.full((1, D), 1.0), 0.0, mean, dict(BASE, **options), None)


def uniform(**options):
    return Case(lambda x: 0.0, 0.5 * np.ones((1, 1)), np.zeros((1, 1)), np.ones((1, 1)), np.full((1, 1), 0.05),
                np.full((1, 1), 0.95), 0.0, 0.5 * np.ones((1, 1)), dict(BASE, search_optimizer="Nelder-Mead", **options),
                lambda x: 0.0)


def noisy(sd=0.3, seed=0, **options):
    base = half_normal(2, specify_target_noise=True, **options)
    draws = np.random.default_rng(seed)  # (the target's own stream: a run does not depend on NumPy's global one)

    def f(x):
        return _scaled_normal(x) + sd * draws.standard_normal(), sd

    return base._replace(f=f)


def errors(case, vp, results):
    """``(err_mean, err_lnZ)`` as the reference's ``run_optim_block`` forms them (:91-93)."""
    vmu = vp.moments(rng="philox", seed=12345)  # (1e6 samples drawn and reduced on the device)
    return float(np.sqrt(np.mean((vmu - case.mu_bar) ** 2))), float(np.abs(results["elbo"] - case.lnZ))


def make(case, seed, VBMC=None, **kw):
    if VBMC is None:
        from pyvbmc_amd import VBMC
    return VBMC(case.f, case.x0.copy(), case.lb.copy(), case.ub.copy(), case.plb.copy(), case.pub.copy(), dict(case.options),
                log_prior=case.log_prior, seed=seed, **kw)
