"""A NumPy / SciPy restatement of the reference's ``active_importance_sampling`` module
(pyvbmc/vbmc/active_importance_sampling.py) over the oracle's plain objects (oracle/gp_ref.py ``GPData``,
oracle/mixture_ref.py ``Mixture``).  TEST INFRASTRUCTURE: the device mirror (pyvbmc_amd/active_importance_sampling.py)
is compared with it, and it is itself held to the reference's recorded outputs (tests/test_ais_host.py:
tests/golden/gpcov.npz, is_known.npz, ais_mcmc.npz).  Line numbers cite the reference's file.

What is restated:

* ``sample_vp``       VariationalPosterior.sample(orig_flag=False) on NumPy's global stream
                      (variational_posterior.py:316-327 / :341-347)
* ``smoothed``        the smoothed posterior of step 1 (:126-137)
* ``proposal_pdf``    active_sample_proposal_pdf (:317-390)
* ``fess``            fess (:426-478)
* ``products``        step 3 (:264-308): K_Xa_X and C_tmp by SciPy's triangular solves
* ``ais``             the whole function (:10-314), ``np.random`` consumed in the reference's order
* ``from_points``     steps 1 (weights only) and 3 for GIVEN proposal points -- what a run on another draw source must
                      reproduce from the points it returned
* ``StandInSampler``  a deterministic stand-in for ``gpyreg.slice_sample.SliceSampler`` in step 2: its moves do not
                      depend on ``log_p`` (x <- clip(x + widths c_t), c_t from a fixed generator), so rounding in
                      ``log_p`` cannot change a trajectory; it records ``f_vals = log_p(x)``.
"""
import sys
from math import ceil
from pathlib import Path

import numpy as np
import scipy.linalg as sla
from scipy.stats import norm

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import acq_ref, gp_ref, mixture_ref  # noqa: E402

VIQR, IMIQR = "viqr", "imiqr"
U75 = norm.ppf(0.75)  # the classes' default quantile
SCALES = (0.05, 0.2, 1.0)


class Opts(dict):
    """The options object of oracle/make_golden.py:229-231: a dict with ``eval``."""

    def eval(self, key, env):
        return self[key]


# ---------------------------------------------------------------------------------------------- acquisition pieces
def is_log_added(f_s2, u=U75):
    """acq_fcn_viqr.py / acq_fcn_imiqr.py ``is_log_added``: log sinh(u f_s) up to a constant."""
    f_s = np.sqrt(f_s2)
    return u * f_s + np.log1p(-np.exp(-2 * u * f_s))


def is_log_base(kind, f_mu, f_s2):
    return np.zeros(f_s2.shape) if kind == VIQR else f_mu


def is_log_full(kind, gp, x, u=U75):
    """``is_log_full(x, gp=gp)``: the averaged noisy prediction at x (gp.predict(add_noise=True))."""
    f_mu, f_s2 = gp_ref.predict(gp, np.atleast_2d(x), add_noise=True)
    return is_log_base(kind, f_mu, f_s2) + is_log_added(f_s2, u)


# ---------------------------------------------------------------------------------------------- mixture pieces
def sample_vp(mix, N):
    """vp.sample(N, orig_flag=False) on np.random (variational_posterior.py:316-327; K = 1: :341-347)."""
    lam = mix.lambd.reshape(1, -1)
    sigma = mix.sigma.reshape(1, -1)
    if mix.K > 1:
        i = np.random.choice(range(mix.K), size=N, p=mix.w.ravel())
        return mix.mu.T[i] + lam * np.random.randn(N, mix.D) * sigma[:, i].T
    return mix.mu.T + lam * np.random.randn(N, mix.D) * sigma


def smoothed(mix):
    """:126-137"""
    mu, sg, w = mix.mu, mix.sigma.reshape(1, -1), mix.w.reshape(1, -1)
    mus, sgs, ws = mu, sg, w
    for s in SCALES:
        ws = np.hstack((ws, w))
        mus = np.hstack((mus, mu))
        sgs = np.hstack((sgs, np.sqrt(sg**2 + s**2)))
    ws = ws / np.sum(ws)
    return mixture_ref.Mixture.make(mus, sgs.ravel(), mix.lambd, ws.ravel())


# ---------------------------------------------------------------------------------------------- the module's functions
def renormalize_weights(ln_w):
    M = np.amax(ln_w)
    return ln_w - (M + np.log(np.sum(np.exp(ln_w - M))))


def proposal_pdf(Xa, gp, mix_is, w_vp, rect_delta, kind):
    """:317-390"""
    N = gp.X.shape[0]
    Na = Xa.shape[0]
    f_mu, f_s2 = gp_ref.predict(gp, Xa, separate_samples=True)
    t = np.zeros((Na, 1 + N if w_vp < 1 else 1))
    if w_vp > 0:
        t[:, 0] = mixture_ref.pdf(mix_is, Xa, log_flag=True).ravel() + np.log(w_vp)
    else:
        t[:, 0] = -np.inf
    ln_y = is_log_base(kind, f_mu, f_s2)
    if w_vp < 1:
        VV = np.prod(2 * rect_delta)
        for i in range(N):
            inside = np.all(np.abs(Xa - gp.X[i, :]) < rect_delta, axis=1)
            t[inside, i + 1] = np.log((1 - w_vp) / VV / N)
            t[~inside, i + 1] = -np.inf
        m = np.amax(t, axis=1)
        if np.any(m == -np.inf):
            raise ValueError("Invalid value.")
        l_pdf = np.log(np.sum(np.exp(t - m.reshape(-1, 1)), axis=1))
        return ln_y - (l_pdf + m).reshape(-1, 1), f_s2
    return ln_y - t, f_s2


def fess(mix, gp, X):
    """:426-478 with the points given; ``gp``: a GPData, or the (N, Ns_gp) array of separate means."""
    N = X.shape[0]
    if isinstance(gp, np.ndarray):
        f_bar = np.mean(gp, axis=1)
    else:
        f_bar = gp_ref.predict(gp, X)[0].ravel()
    v = np.maximum(mixture_ref.pdf(mix, X, log_flag=True), np.log(sys.float_info.min)).ravel()
    ln_w = f_bar - np.atleast_2d(v)
    w = np.exp(ln_w - np.amax(ln_w))
    w = w / np.sum(w)
    return (1 / np.sum(w**2)) / N


def products(gp, X):
    """Step 3 (:264-308): K_Xa_X (S, Na, N) and C_tmp (S, N, Na); ``X`` (Na, D) or (S, Na, D)."""
    S, N, D = len(gp.posteriors), gp.X.shape[0], gp.D
    Na = X.shape[-2]
    K = np.zeros((S, Na, N))
    Ct = np.zeros((S, N, Na))
    for s, p in enumerate(gp.posteriors):
        Xa = X[s] if X.ndim == 3 else X
        K[s] = gp_ref.se_ard(p.hyp[: D + 1], Xa, gp.X)
        if p.L_chol:
            sn2_eff = 1 / p.sW[0] ** 2
            Ct[s] = sla.solve_triangular(p.L, sla.solve_triangular(p.L, K[s].T, trans=True, check_finite=False),
                                         check_finite=False) / sn2_eff
        else:
            Ct[s] = p.L @ K[s].T
    return K, Ct


def from_points(gp, mix, X, kind, n_vp=0, n_box=0):
    """The importance state for GIVEN proposal points ``X`` (Na, D): VIQR's step 0 after the draw, or IMIQR's
    step 1 after the draws (both parts go through the same proposal density, so the rows need not be split), then
    step 3 and the renormalisation."""
    if kind == VIQR:
        f_mu, f_s2 = gp_ref.predict(gp, X, separate_samples=True)
        ln_w = is_log_base(kind, f_mu, f_s2).T
    else:
        w_vp = n_vp / (n_vp + n_box)
        rect_delta = 2 * np.std(gp.X, ddof=1, axis=0)
        lw, f_s2 = proposal_pdf(X, gp, smoothed(mix) if n_vp > 0 else None, w_vp, rect_delta, kind)
        ln_w = lw.T
        ln_w[~np.isfinite(ln_w)] = -np.inf
    K, Ct = products(gp, X)
    return {"X": X, "f_s2": f_s2, "ln_weights": renormalize_weights(ln_w), "K_Xa_X": K, "C_tmp": Ct}


def ais(mix, gp, kind, options, sampler=None, mcmc_importance_sampling=False):
    """The whole function (:10-314) on np.random; ``sampler``: the slice-sampler class of the MCMC steps;
    ``mcmc_importance_sampling``: the acquisition's flag of that name (step 0's fESS / MCMC sub-branch)."""
    X = gp.X
    N, D = X.shape
    S = len(gp.posteriors)
    widths = np.std(X, axis=0, ddof=1)
    diam = np.amax(X, axis=0) - np.amin(X, axis=0)
    lb = np.amin(X, axis=0) - 0.5 * diam
    ub = np.amax(X, axis=0) + 0.5 * diam
    if kind == VIQR:
        Na = ceil(options.eval("active_importance_sampling_mcmc_samples", {"K": mix.K, "n_vars": D, "D": D}))
        if not np.isfinite(Na) or not np.isscalar(Na) or Na <= 0:
            raise ValueError("options['active_importance_sampling_mcmc_samples']should evaluate to a positive integer.")
        Xa = sample_vp(mix, Na)
        f_mu, f_s2 = gp_ref.predict(gp, Xa, separate_samples=True)
        if mcmc_importance_sampling and fess(mix, f_mu, Xa) < options["active_importance_sampling_fess_thresh"]:
            # one MCMC pass over all samples (:80-108)
            n_mcmc = Na * options["active_importance_sampling_mcmc_thin"]
            chain = sampler(lambda x: is_log_full(kind, gp, x), Xa, widths, lb, ub, {"display": "off", "diagnostics": False})
            Xa = chain.sample(n_mcmc, 1, 0)["samples"][-Na:, :]
            f_mu, f_s2 = gp_ref.predict(gp, Xa, separate_samples=True)
        out = {"X": Xa, "f_s2": f_s2, "ln_weights": is_log_base(kind, f_mu, f_s2).T}
    else:
        n_vp = options["active_importance_sampling_vp_samples"]
        n_box = options["active_importance_sampling_box_samples"]
        w_vp = n_vp / (n_vp + n_box)
        rect_delta = 2 * np.std(X, ddof=1, axis=0)
        mix_is = smoothed(mix) if n_vp > 0 else None
        xs, lws, fs = [], [], []
        if n_vp > 0:
            Xa = sample_vp(mix_is, n_vp)
            lw, f_s2 = proposal_pdf(Xa, gp, mix_is, w_vp, rect_delta, kind)
            xs.append(Xa), lws.append(lw.T), fs.append(f_s2)
        if n_box > 0:
            jj = np.random.randint(0, N, size=(n_box,))
            Xa = X[jj, :] + (2 * np.random.rand(jj.size, D) - 1) * rect_delta
            lw, f_s2 = proposal_pdf(Xa, gp, mix_is, w_vp, rect_delta, kind)
            xs.append(Xa), lws.append(lw.T), fs.append(f_s2)
        out = {"X": np.concatenate(xs, axis=0), "f_s2": np.concatenate(fs, axis=0),
               "ln_weights": np.concatenate(lws, axis=1)}
        out["ln_weights"][~np.isfinite(out["ln_weights"])] = -np.inf
        n_mcmc = options["active_importance_sampling_mcmc_samples"]
        if n_mcmc > 0:
            old = out
            out = {"X": np.zeros((S, n_mcmc, D)), "f_s2": np.zeros((n_mcmc, S)), "ln_weights": np.zeros((S, n_mcmc))}
            for s in range(S):
                gp1 = gp_ref.GPData(gp.D, gp.X, gp.y, gp.s2, gp.mean_kind, [gp.posteriors[s]], gp.noise_user)
                thin = options["active_importance_sampling_mcmc_thin"]
                burn_in = ceil(thin * n_mcmc / 2)
                f_mu, f_s2 = gp_ref.predict(gp1, old["X"], separate_samples=True)
                ln_w = old["ln_weights"][s, :].reshape(-1, 1) + is_log_added(f_s2)
                ln_w_max = np.amax(ln_w, axis=1).reshape(-1, 1)
                if np.any(ln_w_max == -np.inf):
                    raise ValueError("Invalid value.")
                w = np.exp(ln_w - ln_w_max).ravel()
                w = w / np.sum(w)
                index = np.random.choice(a=len(w), p=w, replace=False)
                x0 = np.maximum(np.minimum(old["X"][index, :], ub), lb)
                chain = sampler(lambda x, g=gp1: is_log_full(kind, g, x), x0, widths, lb, ub,
                                {"display": "off", "diagnostics": False})
                res = chain.sample(n_mcmc, thin, burn_in)
                Xa, log_p = res["samples"], res["f_vals"]
                f_mu, f_s2 = gp_ref.predict(gp1, Xa, separate_samples=True)
                out["f_s2"][:, s] = f_s2.ravel()
                out["ln_weights"][s, :] = is_log_base(kind, f_mu, f_s2).T - log_p.T
                out["X"][s, :, :] = Xa
    out["K_Xa_X"], out["C_tmp"] = products(gp, out["X"])
    out["ln_weights"] = renormalize_weights(out["ln_weights"])
    return out


class StandInSampler:
    """``SliceSampler(log_p, x0, widths, lb, ub, opts).sample(N, thin, burn_in)`` with moves that ignore ``log_p``.
    ``x0`` (D,) is one walker; a matrix (R, D) -- step 0 hands over all its samples (:100-103) -- is R walkers moved
    in turn, step t moving and recording walker t mod R."""

    SEED = 20240611

    def __init__(self, log_p, x0, widths, lb, ub, opts=None):
        self.log_p = log_p
        self.x0 = np.atleast_2d(np.array(x0, dtype=np.float64))
        self.widths, self.lb, self.ub = (np.asarray(a, dtype=np.float64).ravel() for a in (widths, lb, ub))

    def sample(self, N, thin=1, burn_in=0):
        rng = np.random.default_rng(self.SEED)
        rows = self.x0.copy()
        R, D = rows.shape
        samples, f_vals = [], []
        for t in range(burn_in + N * thin):
            r = t % R
            rows[r] = np.clip(rows[r] + self.widths * rng.uniform(-0.5, 0.5, size=D), self.lb, self.ub)
            if t >= burn_in and (t - burn_in + 1) % thin == 0:
                samples.append(rows[r].copy())
                f_vals.append(float(np.ravel(self.log_p(rows[r]))[0]))
        return {"samples": np.array(samples), "f_vals": np.array(f_vals)}


def larger_case():
    """D = 4, N = 150, S = 3 with one non-Cholesky sample (the construction of tests/test_acquisition.py's larger case):
    oracle GP, mixture, 200 evaluation points and the per-point noise table."""
    rng = np.random.default_rng(31)
    D, N = 4, 150
    X = rng.standard_normal((N, D))
    y = (-0.5 * np.sum(X**2, axis=1) + 0.05 * rng.standard_normal(N)).reshape(-1, 1)
    hyp = np.array([np.concatenate([np.log(0.8 + 0.3 * rng.random(D)), [np.log(2.0)], [ls], [0.1], np.zeros(D), np.zeros(D)])
                    for ls in (np.log(0.05), np.log(3e-4), np.log(0.1))])
    ogp = gp_ref.make_gp(X, y, hyp, gp_ref.MEAN_NEGQUAD)
    assert [p.L_chol for p in ogp.posteriors] == [True, False, True]
    mix = mixture_ref.Mixture.make(rng.standard_normal((D, 3)), [0.5, 0.7, 0.9], np.ones(D), [0.2, 0.3, 0.5])
    Xs = 1.3 * rng.standard_normal((200, D))
    return ogp, mix, Xs, 0.01 + rng.random(N)


# ---------------------------------------------------------------------------------------------- derived quantities
def implied(gp, ais_dict):
    """What oracle/make_golden.py gpcov stores from a state: sf^2 -/+ sum_n K(xa, X_n) C_tmp[n, a] as (Na, S), and the
    cross terms K(xa, X) C_tmp between the first 8 points, (S, 8, 8)."""
    K, Ct = ais_dict["K_Xa_X"], ais_dict["C_tmp"]
    sf2 = np.array([np.exp(2 * p.hyp[gp.D]) for p in gp.posteriors])
    sign = np.array([-1.0 if p.L_chol else 1.0 for p in gp.posteriors])
    vr = np.einsum("san,sna->as", K, Ct)
    return sf2[None, :] + sign[None, :] * vr, np.einsum("san,snb->sab", K[:, :8, :], Ct[:, :, :8])


def quantile_acq(gp, Xs, sn2, ais_dict, kind):
    """The acquisition value of a state (oracle/acq_ref.py quantile_acq); per-sample points (S, Na, D) go through it
    one GP sample at a time and the reference's log-mean-exp over the samples."""
    X = ais_dict["X"]
    if X.ndim == 2:
        return acq_ref.quantile_acq(gp, Xs, sn2, ais_dict, U75, kind == IMIQR)
    S = len(gp.posteriors)
    per = np.stack([acq_ref.quantile_acq(gp_ref.GPData(gp.D, gp.X, gp.y, gp.s2, gp.mean_kind, [gp.posteriors[s]], gp.noise_user),
                                         Xs, sn2, dict(X=X[s], f_s2=ais_dict["f_s2"][:, s:s + 1],
                                                       ln_weights=ais_dict["ln_weights"][s:s + 1]), U75, kind == IMIQR)
                    for s in range(S)], axis=1)
    mx = per.max(axis=1)
    return mx + np.log(np.sum(np.exp(per - mx[:, None]), axis=1) / S)
