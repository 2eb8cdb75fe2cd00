#!/usr/bin/env python
"""Generate tests/golden/vbmc_driver.npz by RUNNING THE REFERENCE's ``VBMC`` constructor, ``Options`` and decision methods
(vbmc/vbmc.py).  TEST INFRASTRUCTURE in the manner of tools/make_optimize_vp_golden.py: it runs only where the reference
checkout is present (VBMC_REFERENCE), imports it at run time with oracle/_stubs for the packages it needs, never calls a
target or a GP, and stores numbers and name lists only.

    python tools/make_vbmc_driver_golden.py             # rewrites tests/golden/vbmc_driver.npz

Three groups (read by tests/test_vbmc_driver_host.py):

init cases   ``INIT_CASES`` below: D in {1, 2, 4}; no bounds, both, mixed per dimension; ``x0`` of one and of several rows;
             missing plausible bounds; ``x0`` outside the plausible box; the three bounded transforms.  Per case the inputs,
             the reference transformer's fields, every numeric ``optim_state`` entry and the first posterior's ``mu``,
             ``sigma``, ``lambd`` after ``np.random.seed(INIT_SEED)``.  ``RAISING``: ``_bounds_check`` inputs that raise
             (a lower bound only among them).
options      every numeric default at D in {1, 2, 10}, the K-dependent ones at K in {1, 2, 5, 50}, the string-valued ones,
             and the full list of names.
traces       ``TRACES`` below: synthetic histories of 30-45 iterations fed, iteration by iteration, through the reference's
             ``_check_termination_conditions``, ``_check_warmup_end_conditions``, ``_setup_vbmc_after_warmup`` and, at every
             iteration as ``max_idx``, ``determine_best_vp`` with and without ``rank_criterion_flag``.  Each trace is built
             so that only the path it is named after can be taken (see ``TRACES``); the tool asserts the events it must
             show before the file is written.
"""
import logging
import os
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("VBMC_REFERENCE", "/root/reference"))
sys.path.insert(0, str(ROOT / "oracle" / "_stubs"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(REF))

OUT = ROOT / "tests" / "golden" / "vbmc_driver.npz"
INIT_SEED = 77
INF = np.inf


def row(*v):
    return np.array([v], dtype=np.float64)


# name, x0, lb, ub, plb, pub, bounded_transform   (None: the argument is not given)
INIT_CASES = (
    ("d1_none", row(0.3), None, None, row(-2.0), row(3.0), "logit"),
    ("d2_none_infs", row(-1.0, -1.0), row(-INF, -INF), row(INF, INF), row(-4.0, -4.0), row(4.0, 4.0), "probit"),
    ("d2_both_logit", row(-1.0, -1.0), row(-20.0, -20.0), row(0.0, 0.0), row(-6.0, -6.0), row(-0.05, -0.05), "logit"),
    ("d2_both_probit", row(-1.0, -1.0), row(-20.0, -20.0), row(0.0, 0.0), row(-6.0, -6.0), row(-0.05, -0.05), "probit"),
    ("d2_both_student4", row(-1.0, -1.0), row(-20.0, -20.0), row(0.0, 0.0), row(-6.0, -6.0), row(-0.05, -0.05), "student4"),
    ("d1_both_student4", row(0.5), row(0.0), row(1.0), row(0.05), row(0.95), "student4"),
    ("d4_mixed", row(0.5, 1.0, -0.5, 2.0), row(-4.0, -INF, -3.0, -INF), row(4.0, INF, 5.0, INF), row(-1.0, -2.0, -1.5, 0.5),
     row(1.0, 3.0, 2.5, 4.0), "probit"),
    ("d2_rows_noplb_both", np.array([[0.5, 1.0], [1.5, -1.0], [-0.5, 0.25], [0.75, 2.0], [1.0, 0.0]]), row(-4.0, -5.0),
     row(4.0, 5.0), None, None, "logit"),
    ("d2_rows_noplb_none", np.array([[0.5, 1.0], [1.5, -1.0], [-0.5, 0.25]]), None, None, None, None, "logit"),
    ("d2_single_noplb_both", row(0.5, 1.0), row(-4.0, -5.0), row(4.0, 5.0), None, None, "probit"),
    ("d4_x0_outside_pb", row(3.0, -2.5, 0.1, 0.2), row(-10.0, -10.0, -INF, -INF), row(10.0, 10.0, INF, INF),
     row(-1.0, -1.0, -1.0, -1.0), row(1.0, 1.0, 1.0, 1.0), "student4"),
    ("d2_rows_plb_given", np.array([[0.5, 1.0], [1.5, -1.0], [0.0, 0.0], [2.5, 0.5]]), row(-8.0, -8.0), row(8.0, 8.0),
     row(-2.0, -2.0), row(2.0, 2.0), "logit"),
)
# name, x0, lb, ub, plb, pub: ``_bounds_check`` raises ValueError
RAISING = (
    ("lower_only", row(1.0, 1.0), row(0.0, 0.0), row(INF, INF), row(0.5, 0.5), row(2.0, 2.0)),
    ("x0_outside_hard", row(5.0, 0.0), row(-4.0, -4.0), row(4.0, 4.0), row(-1.0, -1.0), row(1.0, 1.0)),
    ("plb_equals_pub", row(0.0, 0.0), row(-4.0, -4.0), row(4.0, 4.0), row(-1.0, 1.0), row(1.0, 1.0)),
    ("fixed_variable", row(0.0, 1.0), row(-4.0, 1.0), row(4.0, 1.0), row(-1.0, 1.0), row(1.0, 1.0)),
    ("pb_not_finite", row(0.0, 0.0), None, None, None, None),
    ("order_violated", row(0.0, 0.0), row(-4.0, -4.0), row(4.0, 4.0), row(-5.0, -1.0), row(1.0, 1.0)),
    ("wrong_dimension", row(0.0, 0.0), row(-4.0, -4.0, -4.0), row(4.0, 4.0, 4.0), row(-1.0, -1.0), row(1.0, 1.0)),
)
OPTION_DS = (1, 2, 10)
OPTION_KS = (1, 2, 5, 50)

# ---- decision traces.  All at D = 2 with the default schedule: 10 evaluations at iteration 0, then 5 per iteration, so
# tol_stable_count = 60 is a window of 12 iterations, tol_stable_warmup = 15 one of 3, stop_warmup_thresh 0.2 x 5 = 1.0 in
# ELCBO and warmup_no_impro_threshold = 30 evaluations.  A trace is (name, T, options, shape) with ``shape`` the arguments
# of ``make_trace``:
#   rise      ELBO gain per iteration while rising       rise_until  iteration from which the ELBO is flat
#   lcb_step  gain of lcb_max per iteration: 0.02 > tol_improvement keeps the no-long-term-improvement route shut (the
#             first index within tol_improvement of the maximum is always the present one); 0 opens it after 30 evaluations
#   skl_hi    sKL before ``calm``: 5.0 puts r_index above stop_warmup_reliability = 100 (a false alarm), 0.5 below it
#   calm      iteration from which Delta ELBO, ELBO SD and sKL are small enough for r_index < 1
TRACES = (
    # ELBO flat from iteration 6, lcb_max rising: only the stable-count route can end warm-up; calm from 22: stability
    # terminates 10 iterations later, and the last iteration is stable (determine_best_vp's first branch)
    ("stable_count_then_stable", 45, {}, dict(rise=2.0, rise_until=6, lcb_step=0.02, skl_hi=0.5, calm=22, sn2=1e-4)),
    # ELBO rising by 0.5 for ever (1.5 per window > 1.0: no stable count), lcb_max flat: only the long-term route;
    # never calm: no stable iteration (frac_back), ends by max_fun_evals
    ("no_longterm_then_budget", 32, {"max_fun_evals": 160}, dict(rise=0.5, rise_until=10**6, lcb_step=0.0, skl_hi=0.5,
                                                                 calm=10**6, sn2=0.25)),
    # as the first, but r_index >= 100 at the alarm: data are trimmed, the end is blocked while N is within 10 of the
    # trim (no_recent_trim), then warm-up ends because a trim has happened
    ("false_alarm_trim_block_end", 45, {"max_iter": 45}, dict(rise=2.0, rise_until=4, lcb_step=0.02, skl_hi=5.0, calm=24,
                                                              sn2=1e-2)),
    # the same through the long-term route
    ("false_alarm_longterm", 30, {"max_iter": 30}, dict(rise=0.5, rise_until=10**6, lcb_step=0.0, skl_hi=5.0, calm=10**6,
                                                        sn2=1e-4)),
    # max_iter reached at iteration 31, before any budget
    ("max_iter", 32, {"max_iter": 32, "max_fun_evals": 1000}, dict(rise=0.5, rise_until=10**6, lcb_step=0.02, skl_hi=0.5,
                                                                   calm=10**6, sn2=1e-4)),
    # max_iter reached at iteration 29 with 155 evaluations < min_fun_evals = 200: vetoed until 200 are made
    ("min_fun_evals_veto", 45, {"max_iter": 30, "max_fun_evals": 1000, "min_fun_evals": 200},
     dict(rise=0.5, rise_until=10**6, lcb_step=0.02, skl_hi=0.5, calm=10**6, sn2=1e-4)),
    # deterministic entropy on: the first stable iteration (window of 6) flips the switch and does not finish; the window
    # is 12 from then on and stability terminates later
    ("entropy_switch", 45, {"entropy_switch": True, "det_entropy_min_d": 1}, dict(rise=2.0, rise_until=5, lcb_step=0.02,
                                                                                  skl_hi=0.5, calm=24, sn2=1e-4)),
    # stability reached (12 calm iterations), then lost: determine_best_vp searches from the last stable iteration
    ("stable_then_lost", 34, {"max_iter": 34, "min_iter": 34}, dict(rise=2.0, rise_until=5, lcb_step=0.02, skl_hi=0.5, calm=7,
                                                                   sn2=1e-4, lost=26)),
)
MSG_CLASS = {"": 0, "max_fun_evals": 1, "max_iter": 2, "stable": 3}


def make_trace(seed, T, rise, rise_until, lcb_step, skl_hi, calm, sn2, lost=10**6):
    r = np.random.RandomState(seed)
    elbo, elbo_sd, sKL, lcb = np.zeros(T), np.zeros(T), np.zeros(T), np.zeros(T)
    level = -20.0
    for i in range(T):
        quiet = calm <= i < lost
        if i < rise_until:
            level += rise * (1 + 0.05 * r.rand())
        elif lost <= i:
            level += 0.4 * np.sin(i)
        else:
            level += 1e-3 * r.rand()
        elbo[i] = level
        elbo_sd[i] = (0.02 if quiet else 0.15) * (1 + 0.1 * r.rand())
        sKL[i] = (0.002 if quiet else skl_hi) * (1 + 0.1 * r.rand())
        lcb[i] = -3.0 + (lcb_step * i if i >= 2 else -5.0 + 2.0 * i) + 1e-4 * r.rand()
    n_max = 10 + 5 * (T - 1)
    y = -np.abs(r.standard_normal(n_max)) * np.linspace(600.0, 8.0, n_max)  # early points far below the best
    y[7] = 0.0
    return elbo, elbo_sd, sKL, lcb, np.full(T, sn2) * (1 + 0.05 * r.rand(T)), y


def numeric(v):
    """``v`` as a float array when it is a number, a bool or a numeric array; else None."""
    if isinstance(v, (bool, int, float, np.bool_, np.integer, np.floating)):
        return np.array(float(v))
    if isinstance(v, np.ndarray) and v.dtype.kind in "bif" and v.size > 0:
        return v.astype(np.float64)
    return None


def opt_arr(a):
    return np.zeros(0) if a is None else np.asarray(a, dtype=np.float64)


def main():
    logging.disable(logging.CRITICAL)
    from pyvbmc.vbmc import VBMC
    from pyvbmc.vbmc.options import Options

    def target(x):
        raise AssertionError("the target is never called")

    out = {}
    # ---- init cases
    for name, x0, lb, ub, plb, pub, kind in INIT_CASES:
        np.random.seed(INIT_SEED)
        vb = VBMC(target, None if x0 is None else x0.copy(), *(None if a is None else a.copy() for a in (lb, ub, plb, pub)),
                  options={"bounded_transform": kind})
        p = f"init_{name}_"
        for k, a in (("x0", x0), ("lb", lb), ("ub", ub), ("plb", plb), ("pub", pub)):
            out[p + "in_" + k] = opt_arr(a)
        out[p + "transform"] = np.array(kind)
        pt = vb.parameter_transformer
        assert pt.R_mat is None and pt.scale is None
        for f in ("type", "lb_orig", "ub_orig", "mu", "delta"):
            out[p + "pt_" + f] = np.asarray(getattr(pt, f), dtype=np.float64)
        keys = []
        for k, v in vb.optim_state.items():
            a = numeric(v)
            if a is not None:
                keys.append(k)
                out[p + "os_" + k] = a
        for k, v in vb.optim_state["cache"].items():
            keys.append("cache__" + k)
            out[p + "os_cache__" + k] = np.asarray(v, dtype=np.float64)
        out[p + "os_keys"] = np.array(keys)
        out[p + "n_os_keys"] = np.array(len(vb.optim_state))
        out[p + "x0_tran"] = np.asarray(vb.x0, dtype=np.float64)
        for f in ("mu", "sigma", "lambd"):
            out[p + "vp_" + f] = np.asarray(getattr(vb.vp, f), dtype=np.float64)
        out[p + "vp_K"] = np.array(vb.vp.K)
        print(name, "type", pt.type, len(vb.optim_state), "optim_state keys,", len(keys), "numeric")
    out["init_cases"] = np.array([c[0] for c in INIT_CASES])
    out["init_seed"] = np.array(INIT_SEED)

    for name, x0, lb, ub, plb, pub in RAISING:
        try:
            VBMC(target, x0.copy(), *(None if a is None else a.copy() for a in (lb, ub, plb, pub)))
        except ValueError as e:
            print("raises:", name, "--", " ".join(str(e).split())[:70])
        else:
            raise AssertionError(f"{name} does not raise in the reference")
        for k, a in (("x0", x0), ("lb", lb), ("ub", ub), ("plb", plb), ("pub", pub)):
            out[f"raise_{name}_{k}"] = opt_arr(a)
    out["raising_cases"] = np.array([c[0] for c in RAISING])

    # ---- options
    base = REF / "pyvbmc" / "vbmc" / "option_configs"
    for D in OPTION_DS:
        o = Options(str(base / "basic_vbmc_options.ini"), evaluation_parameters={"D": D})
        o.load_options_file(str(base / "advanced_vbmc_options.ini"), evaluation_parameters={"D": D})
        names = sorted(k for k in dict.keys(o) if k != "useroptions")
        num, strs, kdep, ndep, other = [], [], [], [], []
        for k in names:
            v = dict.__getitem__(o, k)
            if callable(v):
                args = v.__code__.co_varnames[: v.__code__.co_argcount]
                (kdep if args == ("K",) else ndep if args == ("N",) else other).append(k)
            elif isinstance(v, str):
                strs.append(k)
            elif numeric(v) is not None and np.ndim(v) == 0:
                num.append(k)
            else:
                other.append(k)
        p = f"opt_d{D}_"
        out[p + "names"] = np.array(names)
        out[p + "numeric_names"] = np.array(num)
        out[p + "numeric"] = np.array([float(dict.__getitem__(o, k)) for k in num])
        out[p + "numeric_is_bool"] = np.array([isinstance(dict.__getitem__(o, k), (bool, np.bool_)) for k in num])
        out[p + "string_names"] = np.array(strs)
        out[p + "strings"] = np.array([dict.__getitem__(o, k) for k in strs])
        out[p + "k_names"] = np.array(kdep)
        out[p + "k_values"] = np.array([[float(o.eval(k, {"K": K})) for K in OPTION_KS] for k in kdep])
        out[p + "n_names"] = np.array(ndep)
        out[p + "n_values"] = np.array([[float(o.eval(k, {"N": K})) for K in OPTION_KS] for k in ndep])
        out[p + "other_names"] = np.array(other)  # None, empty lists, the acquisition list, annealed_gp_mean
        print("options at D =", D, ":", len(names), "names,", len(num), "numeric,", len(kdep), "of K,", len(ndep), "of N,",
              len(strs), "strings, other:", other)
    out["option_Ds"], out["option_Ks"] = np.array(OPTION_DS), np.array(OPTION_KS)

    # ---- decision traces
    for ti, (name, T, user, shape) in enumerate(TRACES):
        elbo, elbo_sd, sKL, lcb, sn2, y = make_trace(500 + ti, T, **shape)
        np.random.seed(INIT_SEED)
        vb = VBMC(target, row(0.0, 0.0), None, None, row(-3.0, -3.0), row(3.0, 3.0), options=dict(user))
        log, s, h = vb.function_logger, vb.optim_state, vb.iteration_history
        n_max = y.size
        log.y_orig = np.full((max(500, n_max), 1), np.nan)
        log.X_flag = np.full((max(500, n_max),), False)
        rec = {k: [] for k in ("r_index", "elcbo_impro", "stable", "finished", "msg", "warmup", "alarm", "n_trims",
                               "skip", "recompute", "entropy_switch", "last_warmup", "actions")}
        flags = np.zeros((T, n_max), dtype=bool)
        t_end = T
        for it in range(T):
            fc = 10 + 5 * it
            new = slice(0 if it == 0 else fc - 5, fc)
            log.y_orig[new, 0] = y[new]
            log.X_flag[new] = True
            log.Xn, log.func_count = fc - 1, fc
            s["iter"], s["N"], s["sn2_hpd"] = it, fc, sn2[it]
            vb.iteration = it
            vb.logging_action = []
            h.record_iteration({"iter": it, "elbo": elbo[it], "elbo_sd": elbo_sd[it], "sKL": sKL[it], "func_count": fc,
                                "lcb_max": lcb[it], "vp": SimpleNamespace(stats={}), "pruned": 0, "n_eff": fc}, it)
            finished, message = vb._check_termination_conditions()
            alarm = False
            if s["warmup"] and it > 0:
                alarm = bool(vb._check_warmup_end_conditions())
                if alarm:
                    vb._setup_vbmc_after_warmup()
            h.record("warmup", s["warmup"], it)
            rec["r_index"].append(h["r_index"][it])
            rec["elcbo_impro"].append(h["elcbo_impro"][it])
            rec["stable"].append(bool(h["stable"][it]))
            rec["finished"].append(bool(finished))
            rec["msg"].append(3 if "stable" in message else 2 if "max_iter" in message else 1 if message else 0)
            rec["warmup"].append(bool(s["warmup"]))
            rec["alarm"].append(alarm)
            rec["n_trims"].append(len(s["data_trim_list"]))
            rec["skip"].append(bool(s["skip_active_sampling"]))
            rec["recompute"].append(bool(s["recompute_var_post"]))
            rec["entropy_switch"].append(bool(s["entropy_switch"]))
            rec["last_warmup"].append(float(s["last_warmup"]))
            rec["actions"].append("|".join(vb.logging_action))
            s["recompute_var_post"] = False  # (the loop's variational fit resets it)
            flags[it] = log.X_flag[:n_max]
            if finished:
                t_end = it + 1
                break
        # determine_best_vp at every max_idx, both ways.  The history holds object arrays; the rank branch indexes with
        # history["stable"], which NumPy takes only as a boolean array: cast for that call, as a run's caller would have to
        best, best_rank = [], []
        for i in range(t_end):
            best.append(vb.determine_best_vp(max_idx=i)[3])
            try:
                best_rank.append(vb.determine_best_vp(max_idx=i, rank_criterion_flag=True)[3])
            except IndexError:
                kept = h["stable"]
                dict.__setitem__(h, "stable", np.array(list(kept), dtype=bool))
                dict.__setitem__(h, "r_index", np.array(list(h["r_index"]), dtype=np.float64))
                dict.__setitem__(h, "elbo", np.array(list(h["elbo"]), dtype=np.float64))
                dict.__setitem__(h, "elbo_sd", np.array(list(h["elbo_sd"]), dtype=np.float64))
                best_rank.append(vb.determine_best_vp(max_idx=i, rank_criterion_flag=True)[3])
        p = f"trace_{name}_"
        out[p + "T"] = np.array(t_end)
        for k, a in (("elbo", elbo), ("elbo_sd", elbo_sd), ("sKL", sKL), ("lcb_max", lcb), ("sn2_hpd", sn2)):
            out[p + k] = a[:t_end]
        out[p + "y_orig"] = y
        out[p + "option_names"] = np.array(sorted(user))
        out[p + "option_values"] = np.array([float(user[k]) for k in sorted(user)])
        for k in ("r_index", "elcbo_impro", "last_warmup"):
            out[p + k] = np.array(rec[k], dtype=np.float64)
        for k in ("stable", "finished", "warmup", "alarm", "skip", "recompute", "entropy_switch"):
            out[p + k] = np.array(rec[k], dtype=bool)
        out[p + "msg"] = np.array(rec["msg"])
        out[p + "n_trims"] = np.array(rec["n_trims"])
        out[p + "actions"] = np.array(rec["actions"])
        out[p + "data_trim_list"] = np.asarray(s["data_trim_list"], dtype=np.float64)
        out[p + "X_flag"] = np.packbits(flags[:t_end], axis=1)
        out[p + "best"] = np.array(best)
        out[p + "best_rank"] = np.array(best_rank)
        print(name, "T", t_end, "alarms", np.flatnonzero(rec["alarm"]), "warm-up ends",
              int(np.argmin(rec["warmup"])) if not all(rec["warmup"]) else None, "stable", np.flatnonzero(rec["stable"]),
              "msg", rec["msg"][-1], "trims", rec["n_trims"][-1], "best", best[-1], "rank", best_rank[-1])
        check_trace(name, rec, t_end, best, out[p + "data_trim_list"])
    out["traces"] = np.array([t[0] for t in TRACES])
    for k, v in out.items():
        assert v.dtype != object, k  # arrays of numbers and names only
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes")


def check_trace(name, rec, T, best, trims):
    """The events each trace is there for."""
    alarms = list(np.flatnonzero(rec["alarm"]))
    stable = list(np.flatnonzero(rec["stable"]))
    if name == "stable_count_then_stable":
        assert len(alarms) == 1 and not rec["warmup"][alarms[0]] and rec["msg"][-1] == 3 and rec["finished"][-1]
        assert best[-1] == T - 1 and rec["stable"][-1]
    elif name == "no_longterm_then_budget":
        assert len(alarms) == 1 and alarms[0] == 9 and not rec["warmup"][9] and rec["msg"][-1] == 1 and not stable
        assert best[-1] >= (T - 1) - (T - 1) * 0.25
    elif name in ("false_alarm_trim_block_end", "false_alarm_longterm"):
        # the false alarm trims and warm-up goes on; the conditions stay as they are, and the end comes only when N is 10
        # past the trim: two iterations later, not one
        assert len(alarms) == 2 and rec["warmup"][alarms[0]] and not rec["warmup"][alarms[1]] and len(trims) == 1
        assert alarms[1] == alarms[0] + 2
    elif name == "max_iter":
        assert rec["msg"][-1] == 2 and rec["finished"][-1] and T == 32
    elif name == "min_fun_evals_veto":
        assert rec["msg"][29] == 2 and not rec["finished"][29] and rec["finished"][-1] and T == 39
    elif name == "entropy_switch":
        flip = int(np.argmin(rec["entropy_switch"]))
        assert rec["entropy_switch"][flip - 1] and not rec["stable"][flip] and not rec["finished"][flip]
        assert "entropy switch" in rec["actions"][flip] and rec["msg"][-1] == 3
    elif name == "stable_then_lost":
        assert stable and not rec["stable"][-1] and best[-1] >= stable[-1] and rec["msg"][-1] == 2


if __name__ == "__main__":
    main()
