"""The decisions of the VBMC loop as pure functions: arrays and scalars in, flags and numbers out.  No object state, no
device.  Each mirrors a method of the reference's ``vbmc/vbmc.py`` (line numbers below cite that file) or, for
``update_K``, ``vbmc/variational_optimization.py:19-87``; ``pyvbmc_amd/vbmc.py`` applies the results to its state.

History arguments (``elbo``, ``elbo_sd``, ``sKL``, ``func_count``, ``lcb_max``, ``r_index``, ``stable``, ...) are sequences
with one entry per finished iteration, the present one included where the reference has recorded it by then.
``options`` is anything with ``[]``.
"""
import math
from collections import namedtuple

import numpy as np

MSG_MAX_FUN_EVALS = "Inference terminated: reached maximum number of function evaluations options.max_fun_evals."
MSG_MAX_ITER = "Inference terminated: reached maximum number of iterations options.max_iter."
MSG_STABLE = "Inference terminated: variational solution stable for options.tol_stable_count fcn evaluations."

Termination = namedtuple("Termination", "finished message r_index elcbo_impro stable entropy_switch actions")
AfterWarmup = namedtuple("AfterWarmup", "warmup last_warmup threshold keep X_flag data_trim_list actions "
                                        "skip_active_sampling recompute_var_post")
BoostPlan = namedtuple("BoostPlan", "do_boost K_new n_fast_opts n_slow_opts overrides")


def _f(a):
    return np.asarray(a, dtype=np.float64)


def tol_stable_iters(entropy_switch, options):
    """The window of the stability check (:1764-1773): shorter while the deterministic entropy is on."""
    if entropy_switch:
        return options["tol_stable_entropy_iters"]
    return int(math.ceil(options["tol_stable_count"] / options["fun_evals_per_iter"]))


def reliability_index(iteration, elbo, elbo_sd, sKL, func_count, sn2_hpd, stable_iters, options):
    """``(r_index, elcbo_impro)`` of iteration ``iteration`` (:1845-1901): the mean of the ELBO change, the ELBO SD (both in
    units of a noise-adjusted ``tol_sd``) and ``sKL / tol_skl``; and the slope of the ELCBO over the function count in the
    last half window."""
    if iteration < 2:
        return np.inf, np.nan
    elbo, elbo_sd = _f(elbo), _f(elbo_sd)
    sn = np.sqrt(sn2_hpd)
    tol_sn = np.sqrt(sn / options["tol_sd"]) * options["tol_sd"]
    tol_sd = min(max(options["tol_sd"], tol_sn), options["tol_sd"] * 10)
    r = np.full(3, np.nan)
    r[0] = np.abs(elbo[iteration] - elbo[iteration - 1]) / tol_sd
    r[1] = elbo_sd[iteration] / tol_sd
    r[2] = _f(sKL)[iteration] / options["tol_skl"]
    idx0 = int(max(0, iteration - math.ceil(0.5 * stable_iters) + 1))
    xx = _f(func_count)[idx0 : iteration + 1]
    yy = elbo[idx0 : iteration + 1] - options["elcbo_impro_weight"] * elbo_sd[idx0 : iteration + 1]
    slope = np.polyfit(list(map(float, xx)), list(map(float, yy)), 1)[0]
    return np.mean(r), slope


def termination(iteration, func_count_now, elbo, elbo_sd, sKL, func_count, r_index_past, sn2_hpd, entropy_switch,
                last_successful_warping, options):
    """:1735-1843.  ``r_index_past``: the reliability indices of the iterations before this one.  Returns a ``Termination``:
    the finished flag and its message, the iteration's ``r_index`` / ``elcbo_impro`` / ``stable``, ``entropy_switch`` as
    it is afterwards (a stable iteration under the deterministic entropy turns it off and does not finish), and the
    logging actions."""
    finished, message, actions = False, "", []
    if func_count_now >= options["max_fun_evals"]:
        finished, message = True, MSG_MAX_FUN_EVALS
    if iteration + 1 >= options["max_iter"]:
        finished, message = True, MSG_MAX_ITER
    n_iters = tol_stable_iters(entropy_switch, options)
    r_index, impro = reliability_index(iteration, elbo, elbo_sd, sKL, func_count, sn2_hpd, n_iters, options)

    stable = False
    if iteration + 1 >= n_iters and r_index < 1 and impro < options["tol_improvement"]:
        # how many good iterations in the recent past (the present one excluded)
        stable_count = np.sum(_f(r_index_past)[iteration - n_iters + 1 : iteration] < 1)
        if stable_count >= n_iters - np.floor(n_iters * options["tol_stable_excpt_frac"]) - 1:
            if entropy_switch:
                entropy_switch = False
                actions.append("entropy switch")
            else:
                if iteration - last_successful_warping >= n_iters / 3:  # only when distant from the last warping
                    finished, message = True, MSG_STABLE
                stable = True
                actions.append("stable")
    if func_count_now < options["min_fun_evals"] or iteration < options["min_iter"]:  # no early termination
        finished = False
    return Termination(finished, message, r_index, impro, stable, entropy_switch, actions)


def warmup_should_end(iteration, elbo, elbo_sd, lcb_max, func_count, func_count_now, data_trim_list, N, options):
    """:1587-1667 -- warm-up stops when the ELCBO has stopped rising over the last ``tol_stable_warmup`` evaluations and the
    best lower confidence bound of the target has not improved recently, or when that bound has not improved for
    ``warmup_no_impro_threshold`` evaluations; never within 10 points of a data trim."""
    per_iter = options["fun_evals_per_iter"]
    thresh = options["stop_warmup_thresh"] * per_iter
    n_iters = math.ceil(options["tol_stable_warmup"] / per_iter)
    stable_count_flag = False
    if iteration > n_iters:
        elcbo = _f(elbo) - options["elcbo_impro_weight"] * _f(elbo_sd)
        cut = max(3, len(elcbo) - n_iters)  # (the first two iterations are left out: their ELCBO is unreliable)
        stable_count_flag = (np.amax(elcbo[cut:]) - np.amax(elcbo[2:cut])) < thresh
    lcb = _f(lcb_max)[: iteration + 1]
    if options["warmup_check_max"]:
        last = np.full(lcb.shape, False)
        last[max(1, iteration - int(n_iters + 1)) :] = True
        impro_fcn = max(0, np.amax(lcb[last]) - np.amax(lcb[~last]))
    else:
        impro_fcn = 0
    no_recent_improvement_flag = impro_fcn < thresh
    first = np.ravel(np.argwhere(lcb > np.amax(lcb) - options["tol_improvement"]))[0]
    pos = np.asarray(func_count)[: iteration + 1][first]
    no_longterm_improvement_flag = (func_count_now - pos) > options["warmup_no_impro_threshold"]
    last_trim = data_trim_list[-1] if len(data_trim_list) > 0 else -np.inf
    no_recent_trim_flag = (N - last_trim) >= 10
    return bool(((stable_count_flag and no_recent_improvement_flag) or no_longterm_improvement_flag) and no_recent_trim_flag)


def after_warmup(iteration, r_index, data_trim_list, N, y_orig, Xn, X_flag, D, warmup, last_warmup, options):
    """:1669-1733 -- what follows a positive ``warmup_should_end``: a real end (the solution is reliable enough, or data
    have been trimmed before) or a false alarm that only trims.  Either way the training set keeps the points within
    ``threshold`` of the best ``y_orig`` (at least D + 1 of them).  Returns an ``AfterWarmup``; ``keep`` is the mask over
    the logger's rows before it is combined with ``X_flag``."""
    actions = []
    trims = len(data_trim_list)
    if r_index < options["stop_warmup_reliability"] or trims >= 1:
        warmup = False
        actions.append("end warm-up")
        threshold = options["warmup_keep_threshold"] * (trims + 1)
        last_warmup = iteration
    else:
        keep_fa = options["warmup_keep_threshold_false_alarm"]
        if keep_fa is None:
            keep_fa = options["warmup_keep_threshold"]
        threshold = keep_fa * (trims + 1)
        data_trim_list = np.append(data_trim_list, [N])
        actions.append("trim data")
    y_orig = np.asarray(y_orig)
    y_max = max(y_orig[: Xn + 1])
    n_keep_min = D + 1
    with np.errstate(invalid="ignore"):
        keep = (y_max - y_orig) < threshold
    if np.sum(keep) < n_keep_min:
        y_temp = np.copy(y_orig)
        y_temp[~np.isfinite(y_temp)] = -np.inf
        order = np.argsort(y_temp * -1, axis=0)
        keep[order[: min(n_keep_min, Xn + 1)]] = True
    return AfterWarmup(warmup, last_warmup, threshold, keep[:, 0], np.logical_and(keep[:, 0], X_flag), data_trim_list, actions,
                       options["skip_active_sampling_after_warmup"], True)


def best_iteration(stable, elbo, elbo_sd, r_index, max_idx=None, safe_sd=5, frac_back=0.25, rank_criterion_flag=False):
    """The index ``determine_best_vp`` returns (:2077-2139): the last iteration when it is stable; else by rank (position,
    ELCBO, reliability, stability) or the best ELCBO since the last stable iteration -- with none, over the last
    ``frac_back`` of the run."""
    stable = np.asarray(stable, dtype=bool)
    if max_idx is None:
        max_idx = len(stable) - 1
    if stable[max_idx]:
        return int(max_idx)
    n = max_idx + 1
    elbo, elbo_sd = _f(elbo), _f(elbo_sd)
    if rank_criterion_flag:
        rank = np.zeros((n, 4))
        rank[:, 0] = np.arange(1, n + 1)[::-1]
        order = (elbo[:n] - safe_sd * elbo_sd[:n]).argsort()[::-1]
        rank[order, 1] = np.arange(1, n + 1)
        order = _f(r_index)[:n].argsort()
        rank[order, 2] = np.arange(1, n + 1)
        rank[:, 3] = max_idx
        rank[stable[:n], 3] = 1
        return int(np.argmin(np.sum(rank, 1)))
    last_stable = np.argwhere(stable[:n])
    if len(last_stable) == 0:
        idx_start = max(0, int(math.ceil(max_idx - max_idx * frac_back)))
    else:
        idx_start = int(np.ravel(last_stable)[-1])
    elcbo = elbo[idx_start:n] - safe_sd * elbo_sd[idx_start:n]
    return int(idx_start + np.argmax(elcbo))


def _is_unset(v):
    return isinstance(v, (list, tuple)) and len(v) == 0


def _eval(options, key, K):
    v = options[key]
    return v(K) if callable(v) else v


def final_boost_plan(K, options):
    """:1965-2021 -- whether the final boost runs (fewer than ``min_final_components``, or other entropy sample counts for
    the boost) and the options it runs under: no pruning, the boost's entropy samples, no iteration limit."""
    K_new = max(K, options["min_final_components"])
    n_sent, n_fast, n_fine = (_eval(options, k, K_new) for k in ("ns_ent", "ns_ent_fast", "ns_ent_fine"))
    b_sent, b_fast, b_fine = (base if _is_unset(options[k]) else _eval(options, k, K_new) for k, base in (
        ("ns_ent_boost", n_sent), ("ns_ent_fast_boost", n_fast), ("ns_ent_fine_boost", n_fine)))
    do_boost = bool(K < options["min_final_components"] or n_sent != b_sent or n_fine != b_fine)
    n_fast_opts = int(math.ceil(math.ceil(_eval(options, "ns_elbo", K_new)) * options["ns_elbo_incr"]))
    overrides = {"tol_weight": 0, "ns_ent": b_sent, "ns_ent_fast": b_fast, "ns_ent_fine": b_fine,
                 "max_iter_stochastic": np.inf}
    return BoostPlan(do_boost, K_new, n_fast_opts, 1, overrides)


def running_moments(run_mean, run_cov, last_run_avg, mubar, sigma, N, weight):
    """The running mean and covariance of the posterior in transformed space (:1241-1259): ``(run_mean, run_cov,
    last_run_avg)``.  The reference starts afresh when ``len(run_mean) == 0 or len(run_cov == 0)``; its second test takes
    the length of a comparison, which is non-zero for every non-empty ``run_cov``, so in a run the moments are ALWAYS the
    present iteration's.  That test is kept as it is; the weighted branch is the reference's too."""
    mubar = np.reshape(mubar, (1, -1))
    if len(run_mean) == 0 or len(np.asarray(run_cov) == 0):
        return mubar, sigma, N
    w = weight ** (N - last_run_avg)
    return w * run_mean + (1 - w) * mubar, w * run_cov + (1 - w) * sigma, N


def update_K(optim_state, iteration_history, options):
    """The number of mixture components of the next variational fit (``variational_optimization.py:19-87``): after
    warm-up one more while the ELCBO improves and nothing was pruned, ``adaptive_k`` more for a stable solution, at most
    ``k_fun_max(n_eff)`` and never fewer than now."""
    K_new = optim_state["vp_K"]
    k_fun_max = options["k_fun_max"]
    K_max = math.ceil(k_fun_max(optim_state["n_eff"]) if callable(k_fun_max) else k_fun_max)
    adaptive_k = options["adaptive_k"]
    K_bonus = round(adaptive_k(K_new) if callable(adaptive_k) else adaptive_k)
    it = optim_state["iter"]
    if not optim_state["warmup"] and it > 0:
        recent_iters = math.ceil(0.5 * options["tol_stable_count"] / options["fun_evals_per_iter"])
        lo = max(0, it - recent_iters)
        elcbos = _f(iteration_history["elbo"][lo:]) - options["elcbo_impro_weight"] * _f(iteration_history["elbo_sd"][lo:])
        warmups = np.asarray(iteration_history["warmup"][lo:]).astype(bool)
        after = elcbos[~warmups]
        after[0 : min(2, it + 1)] = -np.inf  # (the two iterations right after warm-up do not count)
        improving = bool(after[-1] >= np.max(after) and np.isfinite(after[-1]))
        pruned = np.asarray(iteration_history["pruned"])
        if pruned[-1] == 0 and improving:
            K_new += 1
        if iteration_history["r_index"][-1] < 1 and not optim_state["recompute_var_post"] and improving:
            if np.all(pruned[max(0, it - math.ceil(0.5 * recent_iters)) :] == 0):
                K_new += K_bonus
        K_new = max(optim_state["vp_K"], min(K_new, K_max))
    return K_new


__all__ = ["reliability_index", "termination", "warmup_should_end", "after_warmup", "best_iteration", "final_boost_plan",
           "running_moments", "update_K", "tol_stable_iters", "Termination", "AfterWarmup", "BoostPlan", "MSG_MAX_FUN_EVALS",
           "MSG_MAX_ITER", "MSG_STABLE"]
