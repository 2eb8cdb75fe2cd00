"""The replay cases of ``vbmc_is_mcmc`` shared by tests/test_slice_host.py (their preconditions, on the CPU) and
tests/test_ais_mcmc_gpu.py (the replay itself): oracle GPs built like ``ais_host.larger_case``, the chain's arguments as
``active_importance_sampling`` forms them from the training points, and the host chains (tests/slice_host.py over
``ais_host.is_log_full`` on ``gp_ref.predict``), computed once per process.  TEST INFRASTRUCTURE."""
from functools import lru_cache

import numpy as np

import ais_host
import slice_host
from oracle import gp_ref, mixture_ref

N_KEEP, THIN, BURN = 24, 2, 24
# (D, N, S): one 64-block edge of L^-1; two edges; ais_host.larger_case (its middle sample is not a Cholesky sample)
# the workload's dimensions (bench.py: D = 10 and 20): the chain's D-strided rows in LDS at their size
SHAPES = {"d3_n70": (3, 70, 2), "d2_n130": (2, 130, 2), "larger": (4, 150, 3), "d10_n70": (10, 70, 2), "d20_n130": (20, 130, 2)}
KINDS = (ais_host.IMIQR, ais_host.VIQR)  # ln_y_fmu = 1, 0
# the chains' Philox key per case: the first of 1, 2, ... under which every chain of the case keeps a margin
# |f - ly| >= 1e-6 at every comparison and hits no cap (tests/test_slice_host.py asserts both)
SEEDS = {("d3_n70", ais_host.IMIQR): 1, ("d3_n70", ais_host.VIQR): 1, ("d2_n130", ais_host.IMIQR): 1,
         ("d2_n130", ais_host.VIQR): 1, ("larger", ais_host.IMIQR): 1, ("larger", ais_host.VIQR): 1,
         ("d10_n70", ais_host.IMIQR): 1, ("d10_n70", ais_host.VIQR): 1, ("d20_n130", ais_host.IMIQR): 1,
         ("d20_n130", ais_host.VIQR): 1}
CASES = [(name, kind) for name in SHAPES for kind in KINDS]


@lru_cache(maxsize=None)
def gp_of(name):
    """(oracle GP, mixture) of a shape."""
    if name == "larger":
        ogp, mix, _, _ = ais_host.larger_case()
        return ogp, mix
    return gp_at(*SHAPES[name])


@lru_cache(maxsize=None)
def gp_at(D, N, S):
    """(oracle GP, mixture) at a shape: standard-normal inputs under a noisy negative quadratic, S <= 3 hyper-parameter
    samples that differ in their noise, a three-component mixture.  Above D = 4 the length scales grow with sqrt(D / 4):
    the squared distance of two inputs grows with D, and at unit length scales the median covariance of two inputs would be
    2e-10 sf^2 at D = 20 and 1e-15 sf^2 at D = 32 (largest 3e-3 and 6e-6) -- at or below the 1e-10 sf^2 it is held to,
    so that a wrong sum over the dimensions could hardly show."""
    rng = np.random.default_rng(100 * D + N)
    grow = max(1.0, np.sqrt(D / 4.0))
    X = rng.standard_normal((N, D))
    y = (-0.5 * np.sum(X**2, axis=1) + 0.05 * rng.standard_normal(N)).reshape(-1, 1)
    hyp = np.array([np.concatenate([np.log(grow * (0.8 + 0.3 * rng.random(D))), [np.log(2.0)], [ls], [0.1], np.zeros(D), np.zeros(D)])
                    for ls in (np.log(0.05), np.log(0.1), np.log(0.07))[:S]])
    ogp = gp_ref.make_gp(X, y, hyp, gp_ref.MEAN_NEGQUAD)
    mix = mixture_ref.Mixture.make(rng.standard_normal((D, 3)), [0.5, 0.7, 0.9], np.ones(D), [0.2, 0.3, 0.5])
    return ogp, mix


def chain_args(ogp):
    """(x0 (S, D), widths, lb, ub): the scales and bounds of active_importance_sampling.py:48-53, every chain started at
    a training point of its own."""
    X = ogp.X
    widths = np.std(X, axis=0, ddof=1)
    diam = np.amax(X, axis=0) - np.amin(X, axis=0)
    lb, ub = np.amin(X, axis=0) - 0.5 * diam, np.amax(X, axis=0) + 0.5 * diam
    S = len(ogp.posteriors)
    return X[5 : 5 + S].copy(), widths, lb, ub


def one_sample_gp(ogp, s):
    return gp_ref.GPData(ogp.D, ogp.X, ogp.y, ogp.s2, ogp.mean_kind, [ogp.posteriors[s]], ogp.noise_user)


def run_host(name, kind, seed, scale=1.0):
    """The S host chains of a case: a list of slice_host.chain results; ``scale`` multiplies f (the perturbation test)."""
    ogp, _ = gp_of(name)
    x0, widths, lb, ub = chain_args(ogp)
    out = []
    for s in range(len(ogp.posteriors)):
        g1 = one_sample_gp(ogp, s)
        out.append(slice_host.chain(lambda x, g=g1: scale * ais_host.is_log_full(kind, g, x), x0[s], widths, lb, ub, N_KEEP,
                                    THIN, BURN, seed=seed, s=s))
    return out


@lru_cache(maxsize=None)
def host_replay(name, kind):
    """The host side of a replay case, computed once: the chains, and f_mu / noise-free f_s2 at their kept points."""
    ogp, _ = gp_of(name)
    chains = run_host(name, kind, SEEDS[(name, kind)])
    f_mu = np.empty((N_KEEP, len(chains)))
    f_s2 = np.empty((N_KEEP, len(chains)))
    for s, c in enumerate(chains):
        mu, s2 = gp_ref.predict(one_sample_gp(ogp, s), c["samples"], separate_samples=True)
        f_mu[:, s], f_s2[:, s] = mu.ravel(), s2.ravel()
    return chains, f_mu, f_s2
