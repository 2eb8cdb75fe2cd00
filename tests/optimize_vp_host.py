"""The last stage of ``optimize_vp``, stated in NumPy.  TEST INFRASTRUCTURE: the yardstick of tests/test_optimize_vp_host.py
(against the reference's recorded trials, tests/golden/optimize_vp.npz) and of tests/test_optimize_vp_gpu.py (the device's
re-weighting kernel).  No device, no package kernels.

``reweight``      G, varG, var_ss of a posterior whose components are the alive columns of a recorded ``I_sk`` (S, K0) and
                  ``J_sjk`` (S, K0, K0) with weights ``w``: the reference's ``_gp_log_joint`` tail
                  (pyvbmc/vbmc/variational_optimization.py:1578-1596), one statement per statement, over the upper triangle
                  j <= k with both clamps at ``np.spacing(1)``.
``prune_mixture`` the posterior with one component removed, as the pruning loop forms it (:335-340, then ``get_parameters``,
                  variational_posterior.py:642-676, and ``set_parameters``, :720-756, with ``_neg_elcbo``'s eta, :1082-1085).
``prune_loop``    the loop itself (:322-378) around an evaluator of trials.
"""
import math
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "optimize_vp.npz"
TINY = np.spacing(1)
OPTION_KEYS = ("tol_weight", "tol_improvement", "elcbo_impro_weight", "sgd_step_size", "tol_fun_stochastic",
               "max_iter_stochastic", "elcbo_midpoint", "det_entropy_tol_opt", "hpd_frac", "tol_length", "tol_con_loss",
               "weight_penalty")
K_OPTION_KEYS = ("ns_ent", "ns_ent_fast", "ns_ent_fine", "ns_elbo", "pruning_threshold_multiplier")  # stored at K = 1 .. K0
ATTRS = ("mu", "sigma", "lambd", "w", "eta")
OUT11 = ("nelbo", "G", "H", "varF", "var_ss", "varG", "varH")  # the scalars of _neg_elcbo's 11-tuple that are recorded


def reweight(I_sk, J_sjk, alive, w, terms=False):
    """(G, varG, var_ss) over the alive columns; ``J_sjk`` None: no variance (0, 0).  ``terms``: also the per-sample sums
    of |term| of G_s and of varG_s and the number of terms of each (the error bound's inputs)."""
    I_sk = np.asarray(I_sk, dtype=np.float64)
    S = I_sk.shape[0]
    alive = [int(a) for a in alive]
    w = np.asarray(w, dtype=np.float64).ravel()
    Ka = len(alive)
    G = np.zeros(S)
    vG = np.zeros(S)
    absG, absV = np.zeros(S), np.zeros(S)
    for s in range(S):
        for a in range(Ka):
            t = w[a] * I_sk[s, alive[a]]
            G[s] += t
            absG[s] += abs(t)
        if J_sjk is None:
            continue
        for b in range(Ka):
            for a in range(b + 1):
                J = J_sjk[s, alive[a], alive[b]]
                t = w[b] ** 2 * np.maximum(TINY, J) if a == b else 2 * w[a] * w[b] * J
                vG[s] += t
                absV[s] += abs(t)
        vG[s] = np.maximum(vG[s], TINY)
    if S > 1:
        G_out = np.mean(G)
        varG_ss = np.sum((G - G_out) ** 2) / (S - 1)
        var_ss = varG_ss + np.std(vG, ddof=1)
        varG = np.sum(vG, axis=0) / S + varG_ss
    else:
        G_out, varG, var_ss = G[0], vG[0], 0.0
    if J_sjk is None:
        varG = var_ss = 0.0
    if terms:
        return G_out, varG, var_ss, {"G_s": G, "vG_s": vG, "absG": absG, "absV": absV, "nG": Ka, "nV": Ka * (Ka + 1) // 2}
    return G_out, varG, var_ss


def prune_mixture(m, idx):
    """``m``: dict of mu (D, K), sigma (1, K), lambd (D, 1), w (1, K), eta (1, K).  The posterior without component
    ``idx``: the reference's own NumPy statements on copies."""
    D = m["mu"].shape[0]
    w = np.delete(np.array(m["w"], dtype=np.float64), idx)
    sigma = np.delete(np.array(m["sigma"], dtype=np.float64), idx)
    mu = np.delete(np.array(m["mu"], dtype=np.float64), idx, axis=1)
    lambd = np.array(m["lambd"], dtype=np.float64)
    K = mu.shape[1]
    # get_parameters
    nl = np.sqrt(np.sum(lambd**2) / D)
    lambd = lambd.reshape(-1, 1) / nl
    sigma = sigma.reshape(1, -1) * nl
    w = w.reshape(1, -1) / np.sum(w)
    theta = np.concatenate((mu.ravel(order="F"), np.log(np.concatenate((sigma.ravel(), lambd.ravel(), w.ravel())))))
    # set_parameters
    mu = np.reshape(theta[: D * K], (D, K), order="F")
    sigma = np.exp(theta[D * K : D * K + K])
    lambd = np.exp(theta[D * K + K : D * K + K + D]).T
    eta = theta[-K:]
    eta = eta - np.amax(eta)
    w = np.exp(eta.T)[:, np.newaxis]
    nl = np.sqrt(np.sum(lambd**2) / D)
    lambd = lambd.reshape(-1, 1) / nl
    sigma = sigma.reshape(1, -1) * nl
    w = w.reshape(1, -1) / np.sum(w)
    return {"mu": mu, "sigma": sigma, "lambd": lambd, "w": w, "eta": eta.reshape(1, -1)}, theta


def ns_ent_fine_K(ns_ent_fine, K):
    """``_eval_full_elcbo``'s samples per component at K components (:467); ``ns_ent_fine``: a number or a callable of K."""
    v = ns_ent_fine(K) if callable(ns_ent_fine) else ns_ent_fine
    return math.ceil(v / K)


def prune_loop(m, elbo, elbo_sd, I_sk, J_sjk, tol_weight, threshold, impro_weight, trial, choose):
    """The pruning loop (:322-378).  ``trial(m_pruned, alive, pos) -> dict(nelbo, G, H, varF, varG, varH, var_ss)``
    evaluates a candidate (``alive``: its components' columns in the first evaluation, ``pos``: the position removed);
    ``choose(n) -> int`` is ``np.random.randint(0, n)``.  Returns the final mixture, the values of the last accepted
    evaluation (None without one), ``pruned``, the stats arrays and the log of the trials."""
    K0 = np.size(m["w"])
    alive = list(range(K0))
    already_checked = np.full((K0,), False)
    pruned = 0
    kept = None
    log = []
    I_sk = np.array(I_sk)
    J_sjk = None if J_sjk is None else np.array(J_sjk)
    while np.any((m["w"] < tol_weight) & ~already_checked):
        cand = np.argwhere((m["w"] < tol_weight).ravel() & ~already_checked).ravel()
        r = choose(np.size(cand))
        idx = int(cand[r])
        m_pruned, _ = prune_mixture(m, idx)
        alive_pruned = alive[:idx] + alive[idx + 1 :]
        res = trial(m_pruned, alive_pruned, idx)
        elbo_pruned = -res["nelbo"]
        elbo_pruned_sd = np.sqrt(res["varF"])
        delta = np.abs((elbo_pruned - impro_weight * elbo_pruned_sd) - (elbo - impro_weight * elbo_sd))
        accept = bool(delta < threshold)
        log.append({"cand": cand, "r": r, "idx": idx, "delta": float(delta), "threshold": float(threshold), "accept": accept,
                    "K": len(alive_pruned)})
        if accept:
            m, alive, elbo, elbo_sd, kept = m_pruned, alive_pruned, elbo_pruned, elbo_pruned_sd, res
            pruned += 1
            already_checked = np.delete(already_checked, idx)
            I_sk = np.delete(I_sk, idx, axis=1)
            if J_sjk is not None:
                J_sjk = np.delete(J_sjk, idx, axis=2)  # (axis 2 only: the reference's statement, :376)
        else:
            already_checked[idx] = True
    return m, kept, pruned, I_sk, J_sjk, alive, log


# ---- the fixture ---------------------------------------------------------------------------------------------------------

def case_names(z):
    return [str(n) for n in z["cases"]]


def load_case(z, name):
    p = name + "_"
    return {k[len(p):]: z[k] for k in z.files if k.startswith(p)}


class CaseOptions(dict):
    """The option values a case recorded, read like the reference's ``Options``: ``[]`` and ``eval(name, {"K": K})``."""

    def eval(self, name, params):
        v = self[name]
        return v(**params) if callable(v) else v


def options_of(c):
    o = CaseOptions({k: float(v) for k, v in zip(OPTION_KEYS, c["options"])})
    o["elcbo_midpoint"] = bool(o["elcbo_midpoint"])
    o["max_iter_stochastic"] = int(o["max_iter_stochastic"])
    o["stochastic_optimizer"] = "adam"
    for i, k in enumerate(K_OPTION_KEYS):
        table = np.array(c["k_options"][i])
        o[k] = (lambda t: (lambda K: float(t[int(K) - 1])))(table)
    return o


def trials_of(c):
    """The recorded trials of a case as a list of dicts."""
    n = int(c["n_trials"])
    out = []
    for t in range(n):
        lo, hi = int(c["trial_cand_off"][t]), int(c["trial_cand_off"][t + 1])
        out.append({"cand": c["trial_cand"][lo:hi], "r": int(c["trial_r"][t]), "idx": int(c["trial_idx"][t]),
                    "delta": float(c["trial_delta"][t]), "threshold": float(c["trial_threshold"][t]),
                    "accept": bool(c["trial_accept"][t]), "eval": int(c["trial_eval"][t])})
    return out


def eval_of(c, e):
    """Recorded ``_eval_full_elcbo`` call ``e``: theta, K, the scalars, I_sk, J_sjk (cut to K)."""
    K = int(c["eval_K"][e])
    n = int(c["eval_ntheta"][e])
    out = {k: float(c["eval_" + k][e]) for k in OUT11}
    out.update(theta=np.array(c["eval_theta"][e, :n]), K=K, slot=int(c["eval_slot"][e]), I_sk=np.array(c["eval_I_sk"][e][:, :K]),
               J_sjk=np.array(c["eval_J_sjk"][e][:, :K, :K]))
    return out
