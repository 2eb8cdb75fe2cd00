"""``VBMC``: the inference loop over the package's own device stages -- active sampling, GP training, the variational fit
-- with no PyVBMC and no gpyreg around them.  Mirror of the reference's ``vbmc/vbmc.py`` (line numbers below cite that
file): the constructor does the work of ``_bounds_check`` (:315-566) and ``_init_optim_state`` (:568-823), ``optimize``
runs the loop of :863-1585, and every decision of the loop is a pure function of ``driver_rules.py``.

    vbmc = VBMC(log_density, x0, lb, ub, plb, pub, {"warp_rotoscaling": False}, seed=1)
    vp, results = vbmc.optimize()

Per iteration: ``active_sample`` (the initial design at iteration 0) with ``train_gp`` and ``optimize_vp`` of this package
for its local updates; ``train_gp``; ``update_K``; ``optimize_vp``; sKL by ``vp.kl_div``; the best lower confidence bound by
``gp.predict`` at the training inputs; the running moments; the history record; termination; the end of warm-up with
``gp.reupdate`` after the trim.  After the loop ``determine_best_vp`` and ``final_boost``.  The module adds no kernel.

Draws.  ``rng`` ("philox" by default) and a seed derived from ``seed``, the iteration and the stage go down to every
stage.  What the stages still draw from NumPy's global stream (the initial design, the perturbation of the first
posterior, the sub-sampling of GP starting points) follows ``seed`` too: with a ``seed`` the constructor and ``optimize``
seed that stream for their own duration and put the caller's state back when they return, so two runs with one seed are
the same run and the caller's stream is as it was.  ``seed=None`` uses the caller's stream as it is and draws the base seed
from it.

Refused, with ``_lib.UnsupportedShape`` from the constructor before the target is called once: D > 32;
``uncertainty_handling_level`` 1; ``warp_rotoscaling`` (ON in the reference's defaults: pass ``False``) and
``warp_nonlinear``; ``separate_search_gp``; a ``stochastic_optimizer`` other than adam; and what a stage would refuse
later -- a ``gp_hyp_sampler`` other than slicesample, a ``gp_mean_fun`` other than zero / const / negquad,
``noise_shaping``, a ``search_optimizer`` other than none / cmaes (Nelder-Mead at D = 1), an acquisition function the
package has not, ``variable_means`` off, ``ns_ent_fast`` / ``ns_ent_fast_active`` / ``ns_ent_fast_boost`` above 0, ``k_warmup``
or ``min_final_components`` above 128.

Save, load, checkpoints (:2148-2273).  ``save(file)`` writes the whole driver in one dump, atomically (_persist.py);
``VBMC.load(file, new_options, iteration, set_random_state)`` reads it back without touching a device.
``optimize(checkpoint=path, checkpoint_every=n)`` saves at the bottom of every n-th iteration and once more after the loop;
iteration boundaries are the granularity (no signal handlers).  What a checkpoint promises:

* An exact resume.  A run that is stopped and resumed from its checkpoint (``load`` with ``iteration=None``, then
  ``optimize()``) is, bit for bit, the run that was never stopped: the file holds the base seed, the per-stage call counters
  of the seeds, NumPy's global stream state at the save, the timings and the termination message; the first ``optimize()``
  after a load continues at ``iteration + 1`` with them and first puts the live GP's posterior back on the device as the
  device built it (``gp.reinstall``), so that the next one-point append takes the arithmetic route it took in the
  uninterrupted run.  With a ``seed`` the run's stream is set to the saved state instead of being seeded, and the
  caller's stream is put back on return as always; with ``seed=None`` the caller's stream is used as it is unless
  ``set_random_state`` is given.  A driver whose ``optimize`` raised in the middle of an iteration is not resumable in
  memory: resume from the file.
* A valid, not exact, rewind.  ``iteration=k`` takes the posterior, the GP, the logger and the state from the history's
  snapshots of iteration k, which are taken at different points of that iteration (the logger and the GP before the
  warm-up trim, the state after it): a state to go on from, not the continuation of the run.
* Nothing about the target.  The file is a pickle: a target (and a ``log_prior``) defined at module level is saved by
  name; a lambda or a closure needs ``dill`` (used only where it imports) or cannot be saved, and whatever state a closure
  carries -- a private ``Generator`` of a noisy target -- is the user's to save and restore.  Loading a pickle runs
  code: load only files you wrote yourself.

Left out: plotting, ``__str__``; the ``varactivesample`` branch; ``_recompute_lcb_max`` (a stub in the reference as well); a
separate ``prior`` object (``log_prior`` is taken).
"""
import contextlib
import copy
import logging
import math
import os
import sys
import time

import numpy as np

from . import _lib
from . import _persist
from . import driver_rules as rules
from . import gp as gp_mod
from .acquisition import as_package_acq
from .active_sample import active_sample
from .function_logger import FunctionLogger
from .gaussian_process_train import train_gp
from .optimize_vp import optimize_vp
from .options import Options
from .parameter_transformer import ParameterTransformer
from .variational_posterior import VariationalPosterior, _rng_mode

ALGORITHM = "Variational Bayesian Monte Carlo (pyvbmc_amd)"
VERSION = "0.1"
HISTORY_KEYS = ("r_index", "elcbo_impro", "stable", "elbo", "vp", "warmup", "iter", "elbo_sd", "lcb_max", "data_trim_list",
                "gp", "gp_hyp_full", "Ns_gp", "timer", "optim_state", "sKL", "sKL_true", "pruned", "var_ss", "func_count",
                "n_eff", "logging_action", "function_logger", "random_state")
VALID_GP_MEAN_FUNS = ("zero", "const", "negquad", "se", "negquadse", "negquadfixiso", "negquadfix", "negquadsefix",
                      "negquadonly", "negquadfixonly", "negquadlinonly", "negquadmix")
STAGES = ("active_sampling", "gp_train", "variational_fit", "finalize", "boost")
_K_MAX = 128  # (sieve.check_supported)


class StageTimer:
    """Seconds per stage of one iteration: ``start_timer`` / ``stop_timer`` (what ``active_sample`` calls) over a dict."""

    def __init__(self):
        self.durations, self._t0 = {}, {}

    def reset(self):
        self.durations, self._t0 = {}, {}

    def start_timer(self, name):
        self._t0[name] = time.perf_counter()

    def stop_timer(self, name):
        t0 = self._t0.pop(name, None)
        if t0 is not None:
            self.durations[name] = self.durations.get(name, 0.0) + time.perf_counter() - t0

    def get_duration(self, name):
        return self.durations.get(name)


def stage_seed(seed, iteration, stage, n=0):
    """The 62-bit seed of call ``n`` of stage ``stage`` (an index into ``STAGES``) in iteration ``iteration``."""
    words = np.random.SeedSequence([int(seed) % 2**64, int(iteration) + 1, int(stage), int(n)]).generate_state(1, np.uint64)
    return int(words[0] >> np.uint64(2))


@contextlib.contextmanager
def _numpy_stream(seed, use, resume_state=None):
    """With a ``seed``: NumPy's global stream seeded for the block (``use`` 0: the constructor, 1: the run) -- or, for a
    run resumed from a checkpoint, set to the state the checkpoint recorded -- and the caller's state put back after it.
    ``seed=None``: the caller's stream is used as it is."""
    if seed is None:
        yield
        return
    state = np.random.get_state()
    if resume_state is None:
        np.random.seed(stage_seed(seed, -1, use) % 2**32)
    else:
        np.random.set_state(resume_state)
    try:
        yield
    finally:
        np.random.set_state(state)


def _copy_value(v):
    if isinstance(v, np.ndarray):
        return v.copy()
    if isinstance(v, dict):
        return {k: _copy_value(x) for k, x in v.items()}
    return list(v) if isinstance(v, list) else v


def _copy_state(optim_state):
    """``optim_state`` for the history: a new dict with its arrays, lists and nested dicts (cache, search bounds,
    ``data_trim_list``, ``hyp_dict``, ``iter_list``) copied."""
    return {k: _copy_value(v) for k, v in optim_state.items()}


def _copy_logger(log):
    """The function logger for the history: its own arrays, the same target and transformer."""
    new = copy.copy(log)
    for k, v in vars(log).items():
        if isinstance(v, np.ndarray):
            setattr(new, k, v.copy())
    return new


def bounds_check(x0, lower_bounds, upper_bounds, plausible_lower_bounds=None, plausible_upper_bounds=None, logger=None):
    """:315-566 -- the bounds as (1, D) float rows in the order LB < PLB < PUB < UB, plausible bounds that are missing
    estimated from ``x0`` (several rows) or taken from the hard bounds, ``x0`` moved inside the effective bounds and the
    plausible box widened to hold it.  Raises the reference's ``ValueError``s."""
    logger = logging.getLogger("VBMC") if logger is None else logger
    N0, D = x0.shape
    plb, pub, lb, ub = plausible_lower_bounds, plausible_upper_bounds, lower_bounds, upper_bounds
    if plb is None or pub is None:
        if N0 > 1:
            logger.warning("PLB and/or PUB not specified. Estimating plausible bounds from starting set X0...")
            width = x0.max(0) - x0.min(0)
            if plb is None:
                plb = np.maximum(x0.min(0) - width / N0, lb)
            if pub is None:
                pub = np.minimum(x0.max(0) + width / N0, ub)
            same = plb == pub
            if np.any(same):
                plb[same], pub[same] = lb[same], ub[same]
                logger.warning("vbmc:pbInitFailed: Some plausible bounds could not be determined from starting set. "
                               "Using hard upper/lower bounds for those instead.")
        else:
            logger.warning("vbmc:pbUnspecified: Plausible lower/upper bounds PLB and/or PUB not specified and X0 is not a "
                           "valid starting set. Using hard upper/lower bounds instead.")
            plb = np.copy(lb) if plb is None else plb
            pub = np.copy(ub) if pub is None else pub
    try:
        lb, ub, plb, pub = (np.atleast_1d(b) if np.atleast_1d(b).shape == (1, D) else np.atleast_1d(b).reshape((1, D))
                            for b in (lb, ub, plb, pub))
    except ValueError as exc:
        raise ValueError("Bounds must match problem dimension D=%d." % D) from exc
    if np.any(~np.isfinite(plb)) or np.any(~np.isfinite(pub)):
        raise ValueError("Plausible interval bounds PLB and PUB need to be finite.")
    if any(np.any(~np.isreal(a)) for a in (x0, lb, ub, plb, pub)):
        raise ValueError("All input vectors (x0, lower_bounds, upper_bounds, plausible_lower_bounds, "
                         "plausible_upper_bounds), if specified, need to be real valued.")
    x0, lb, ub, plb, pub = (a.astype(np.float64) if np.issubdtype(a.dtype, np.integer) else a for a in (x0, lb, ub, plb, pub))

    if np.any((lb == ub) & (ub == plb) & (plb == pub)):
        raise ValueError("vbmc:FixedVariables VBMC does not support fixed variables. Lower and upper bounds should be "
                         "different.")
    if np.any(plb == pub):
        raise ValueError("vbmc:MatchingPB:For all variables, plausible lower and upper bounds need to be distinct.")
    if np.any(x0 < lb) or np.any(x0 > ub):
        raise ValueError("vbmc:InitialPointsNotInsideBounds: The starting points X0 are not inside the provided hard "
                         "bounds LB and UB.")

    # the effective bounds, slightly inside the hard ones; infinities stay
    span = ub - lb
    span[np.isinf(span)] = 1e3
    frac, realmin = 1e-3, sys.float_info.min
    lb_eff = lb + frac * span
    lb_eff[np.abs(lb) <= realmin] = frac * span[np.abs(lb) <= realmin]
    ub_eff = ub - frac * span
    ub_eff[np.abs(ub) <= realmin] = -frac * span[np.abs(ub) <= realmin]
    lb_eff[np.isinf(lb)] = lb[np.isinf(lb)]
    ub_eff[np.isinf(ub)] = ub[np.isinf(ub)]
    if np.any(lb_eff >= ub_eff):
        raise ValueError("vbmc:StrictBoundsTooClose: Hard bounds LB and UB are numerically too close. Make them more "
                         "separate.")
    if np.any(x0 < lb_eff) or np.any(x0 > ub_eff):
        logger.warning("vbmc:InitialPointsTooClosePB: The starting points X0 are on or numerically too close to the hard "
                       "bounds LB and UB. Moving the initial points more inside...")
        x0 = np.maximum(np.minimum(x0, ub_eff), lb_eff)

    order_msg = ("vbmc:StrictBounds: For each variable, hard and plausible bounds should respect the ordering "
                 "LB < PLB < PUB < UB.")
    if np.any(~((lb <= plb) & (plb < pub) & (pub <= ub))):
        raise ValueError(order_msg)
    if np.any(lb_eff > plb) or np.any(pub > ub_eff):
        logger.warning("vbmc:TooCloseBounds: For each variable, hard and plausible bounds should not be too close. "
                       "Moving plausible bounds.")
        plb, pub = np.maximum(plb, lb_eff), np.minimum(pub, ub_eff)
    if np.any(x0 <= plb) or np.any(x0 >= pub):
        logger.warning("vbmc:InitialPointsOutsidePB. The starting points X0 are not inside the provided plausible bounds "
                       "PLB and PUB. Expanding the plausible bounds...")
        plb, pub = np.minimum(plb, x0.min(0)), np.maximum(pub, x0.max(0))
    if np.any(~((lb < plb) & (plb < pub) & (pub < ub))):
        raise ValueError(order_msg)
    if np.any((np.isfinite(lb) & np.isinf(ub)) | (np.isinf(lb) & np.isfinite(ub))):
        raise ValueError("vbmc:HalfBounds: Each variable needs to be unbounded or bounded. Variables bounded only "
                         "below/above are not supported.")
    return x0, lb, ub, plb, pub


def init_optim_state(D, x0, lb, ub, plb, pub, parameter_transformer, options):
    """:568-823 -- the state the stages read and the loop updates, under the reference's keys."""
    y_orig = np.array(options["f_vals"]).ravel()
    if len(y_orig) == 0:
        y_orig = np.full([x0.shape[0]], np.nan)
    if len(x0) != len(y_orig):
        raise ValueError("vbmc:MismatchedStartingInputs The number of points in X0 and of their function values as "
                         "specified in self.options.f_vals are not the same.")
    s = {"cache": {"x_orig": x0, "y_orig": y_orig}}
    s["cache_active"] = np.any(np.isfinite(y_orig))
    s["integer_vars"] = np.full(D, False)
    if len(options["integer_vars"]) > 0:
        integeridx = np.asarray(options["integer_vars"]) != 0
        s["integer_vars"][integeridx] = True
        if (np.any(np.isinf(lb[:, integeridx])) or np.any(np.isinf(ub[:, integeridx]))
                or np.any(lb[:, integeridx] % 1 != 0.5) or np.any(ub[:, integeridx] % 1 != 0.5)):
            raise ValueError("Hard bounds of integer variables need to be set at +/- 0.5 points from their boundary values "
                             "(e.g., -0.5 and 10.5 for a variable that takes values from 0 to 10)")
    s["lb_orig"], s["ub_orig"], s["plb_orig"], s["pub_orig"] = lb.copy(), ub.copy(), plb.copy(), pub.copy()
    eps_orig = (ub - lb) * options["tol_bound_x"]
    with np.errstate(invalid="ignore"):  # (inf - inf)
        s["lb_eps_orig"], s["ub_eps_orig"] = lb + eps_orig, ub - eps_orig
    with np.errstate(divide="ignore"):
        s["lb_tran"], s["ub_tran"] = parameter_transformer(lb), parameter_transformer(ub)
    s["plb_tran"], s["pub_tran"] = parameter_transformer(plb), parameter_transformer(pub)
    s["iter"] = -1
    s["sn2_hpd"] = np.inf
    s["last_warping"] = -np.inf
    s["last_successful_warping"] = -np.inf
    s["warping_count"] = 0
    s["stop_sampling"] = 0 if options["ns_gp_max"] > 0 else np.inf
    s["recompute_var_post"] = True
    s["warmup"] = options["warmup"]
    s["last_warmup"] = np.inf if options["warmup"] else 0
    s["warmup_stable_count"] = 0
    s["proposal_fcn"] = "@(x)proposal_vbmc" if options["proposal_fcn"] is None else options["proposal_fcn"]
    s["R"] = np.inf
    s["skip_active_sampling"] = False
    s["run_mean"], s["run_cov"], s["last_run_avg"] = [], [], np.nan
    s["vp_K"] = options["k_warmup"]
    s["pruned"] = 0
    # the deterministic entropy only from det_entropy_min_d dimensions on
    s["entropy_switch"] = options["entropy_switch"] if D >= options["det_entropy_min_d"] else False
    s["tol_gp_var"] = options["tol_gp_var"]
    s["max_fun_evals"] = options["max_fun_evals"]
    # (the reference's key; its acquisition functions read "variance_regularized_acq_fcn", which is therefore unset
    # there and here: no variance regularisation)
    s["variance_regularized_acqfcn"] = True
    s["search_cache"] = []
    if options["specify_target_noise"]:
        s["uncertainty_handling_level"] = 2
    elif len(options["uncertainty_handling"]) > 0:
        s["uncertainty_handling_level"] = 1
    else:
        s["uncertainty_handling_level"] = 0
    if options["acq_hedge"]:
        s["hedge"] = []
    s["iter_list"] = {"u": [], "f_val": [], "f_sd": [], "fhyp": []}
    s["entropy_alpha"] = options["det_entropy_alpha"]
    s["repeated_observations_streak"] = 0
    s["data_trim_list"] = []
    prange = s["pub_tran"] - s["plb_tran"]
    s["lb_search"] = np.maximum(s["plb_tran"] - prange * options["active_search_bound"], s["lb_tran"])
    s["ub_search"] = np.minimum(s["pub_tran"] + prange * options["active_search_bound"], s["ub_tran"])
    s["gp_cov_fun"] = 1
    # constant noise for stability; inferred noise (level 1); user-provided per-point noise (level 2)
    s["gp_noise_fun"] = {0: [1, 0, 0], 1: [1, 2, 0], 2: [1, 1, 0]}[s["uncertainty_handling_level"]]
    if options["noise_shaping"] and s["gp_noise_fun"][1] == 0:
        s["gp_noise_fun"][1] = 1
    s["gp_mean_fun"] = options["gp_mean_fun"]
    if s["gp_mean_fun"] not in VALID_GP_MEAN_FUNS:
        raise ValueError("vbmc:UnknownGPmean:Unknown/unsupported GP mean function. Supported mean functions are zero, "
                         "const, negquad, and se")
    s["int_mean_fun"] = options["gp_int_mean_fun"]
    s["out_warp_delta"] = options["out_warp_thresh_base"] if options["fitness_shaping"] else []
    return s


def _refuse(D, options, optim_state):
    """Everything that is known up front to be outside the device stages."""
    def no(what):
        raise _lib.UnsupportedShape("VBMC: " + what)

    if D > 32:
        no(f"D={D} > 32 not supported")
    if optim_state["uncertainty_handling_level"] == 1:
        no("uncertainty_handling_level 1 (noise of unknown size) is not supported; report the noise with "
           "specify_target_noise")
    if options["warp_rotoscaling"]:
        no("warp_rotoscaling is not wired into the loop yet: pass options={'warp_rotoscaling': False}")
    if options["separate_search_gp"]:
        no("separate_search_gp is not supported")
    if options["stochastic_optimizer"] != "adam":
        no(f"stochastic_optimizer {options['stochastic_optimizer']!r} (adam only)")
    if options["gp_hyp_sampler"] != "slicesample":
        no(f"gp_hyp_sampler {options['gp_hyp_sampler']!r} (slicesample only)")
    if options["gp_mean_fun"] not in ("zero", "const", "negquad"):
        no(f"gp_mean_fun {options['gp_mean_fun']!r} (zero, const, negquad)")
    if options["noise_shaping"]:
        no("noise_shaping is not supported")
    opt = options["search_optimizer"]
    if opt not in ("none", "cmaes") and not (D == 1 and opt == "Nelder-Mead"):
        no(f"search_optimizer {opt!r} (none, cmaes and, for D = 1, Nelder-Mead)")
    for a in options["search_acq_fcn"]:
        as_package_acq(a)  # (raises UnsupportedShape for a class the package has not)
    if not options["variable_means"]:  # (components tied to the training inputs: K would grow with N inside the sieve)
        no("variable_means off is not supported")
    for key in ("ns_ent_fast", "ns_ent_fast_active", "ns_ent_fast_boost"):
        v = options[key]
        if callable(v) or not (v == 0 or (key.endswith("boost") and isinstance(v, list) and len(v) == 0)):
            no(f"{key} > 0 (Monte-Carlo entropy inside the sieve) is not supported")
    if options["k_warmup"] > _K_MAX or options["min_final_components"] > _K_MAX:
        no(f"more than {_K_MAX} mixture components")


class _LogJoint:
    """``log_likelihood + log_prior`` as one target; ``noisy``: the likelihood returns ``(value, noise SD)``.  A class at
    module level, so that a driver built from module-level functions pickles."""

    def __init__(self, log_likelihood, log_prior, noisy):
        self.log_likelihood, self.log_prior, self.noisy = log_likelihood, log_prior, noisy

    def __call__(self, theta):
        if self.noisy:
            ll, noise_est = self.log_likelihood(theta)
            return ll + self.log_prior(theta), noise_est
        return self.log_likelihood(theta) + self.log_prior(theta)


class VBMC:
    """``VBMC(log_density, x0, lower_bounds, upper_bounds, plausible_lower_bounds, plausible_upper_bounds, options=None, *,
    log_prior=None, ctx=None, rng="philox", seed=None)``; ``optimize()`` returns ``(vp, results)``.  Module docstring:
    the stages, the draws, the refusals."""

    def __init__(self, log_density, x0=None, lower_bounds=None, upper_bounds=None, plausible_lower_bounds=None,
                 plausible_upper_bounds=None, options=None, *, log_prior=None, ctx=None, rng="philox", seed=None):
        self.logger = logging.getLogger("VBMC")
        self.rng, self.seed, self._ctx = _rng_mode(rng), seed, ctx
        if x0 is None:
            if plausible_lower_bounds is None or plausible_upper_bounds is None:
                raise ValueError("vbmc:UnknownDims If no starting point is provided, PLB and PUB need to be specified.")
            x0 = np.full(np.shape(plausible_lower_bounds), np.nan)
        x0 = np.asarray(x0)
        if x0.ndim == 1:
            x0 = x0.reshape((1, -1))
        self.D = D = x0.shape[1]
        user = dict(options or {})
        if user.pop("warp_nonlinear", False):  # (not an option of the reference's files; named here to be refused)
            raise _lib.UnsupportedShape("VBMC: warp_nonlinear is not supported")
        self.options = Options(D, user)
        self._set_display()
        if D > 32:
            raise _lib.UnsupportedShape(f"VBMC: D={D} > 32 not supported")

        lb = np.ones((1, D)) * -np.inf if lower_bounds is None else np.asarray(lower_bounds)
        ub = np.ones((1, D)) * np.inf if upper_bounds is None else np.asarray(upper_bounds)
        plb = None if plausible_lower_bounds is None else np.asarray(plausible_lower_bounds)
        pub = None if plausible_upper_bounds is None else np.asarray(plausible_upper_bounds)
        (self.x0, self.lower_bounds, self.upper_bounds, self.plausible_lower_bounds,
         self.plausible_upper_bounds) = bounds_check(x0, lb, ub, plb, pub, self.logger)
        if not np.all(np.isfinite(self.x0)):  # no valid starting point: the centre of the plausible box
            self.x0 = 0.5 * (self.plausible_lower_bounds + self.plausible_upper_bounds)

        self.parameter_transformer = ParameterTransformer(D, self.lower_bounds, self.upper_bounds,
                                                          self.plausible_lower_bounds, self.plausible_upper_bounds,
                                                          transform_type=self.options["bounded_transform"])
        with _numpy_stream(seed, 0):
            self.vp = VariationalPosterior(D=D, K=self.options["k_warmup"], x0=self.x0,
                                           parameter_transformer=self.parameter_transformer)
        if ctx is not None:
            self.vp.ctx = ctx
        if not self.options["warmup"]:
            self.vp.optimize_mu = self.options["variable_means"]
            self.vp.optimize_weights = self.options["variable_weights"]
        self.gp = None
        self.hyp_dict = {}
        self.iteration = -1
        self.is_finished = False
        self.logging_action = []
        self.optim_state = init_optim_state(D, self.x0, self.lower_bounds, self.upper_bounds, self.plausible_lower_bounds,
                                            self.plausible_upper_bounds, self.parameter_transformer, self.options)
        _refuse(D, self.options, self.optim_state)

        level = self.optim_state["uncertainty_handling_level"]
        self.log_likelihood, self.log_prior = None, log_prior
        if log_prior is None:
            self.log_joint = log_density
        else:
            self.log_likelihood = log_density
            self.log_joint = _LogJoint(log_density, log_prior, level == 2)
        self.function_logger = FunctionLogger(self.log_joint, D, level > 0, level, self.options["cache_size"],
                                              self.parameter_transformer)
        self.x0 = self.parameter_transformer(self.x0)
        self.iteration_history = {k: [] for k in HISTORY_KEYS}
        self.timer = StageTimer()
        self.timings = {k: 0.0 for k in STAGES}
        # what a checkpoint carries beyond the above (module text): the calls made so far per seeded stage, the message,
        # and -- filled in by ``save`` / ``load`` -- the stream state and whether the device held the live GP as built
        self._stage_calls = {1: 0, 2: 0}
        self._termination_message = ""
        self._numpy_state = None
        self._gp_dev_at_save = False
        self._resume = None
        self.checkpoint_log = []  # (iteration, seconds, bytes) of every checkpoint this process wrote

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_ctx"] = None
        return st

    # ---- plumbing
    def _set_display(self):
        level = {"off": logging.WARN, "final": logging.WARN, "notify": logging.INFO, "iter": logging.INFO,
                 "full": logging.DEBUG}.get(self.options["display"], logging.INFO)
        self.logger.setLevel(level)

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.default_context()
        return self._ctx

    def _record(self, key, value, iteration):
        """``iteration_history[key][iteration] = value`` on a plain list."""
        lst = self.iteration_history[key]
        while len(lst) <= iteration:
            lst.append(None)
        lst[iteration] = value

    def _own(self, vp):
        """``vp`` on the driver's context and with the driver's transformer OBJECT (the stages return deep copies, whose
        transformers are equal by value): one transformer across the driver, the posterior and the logger."""
        if vp.parameter_transformer is not self.parameter_transformer and vp.parameter_transformer == self.parameter_transformer:
            vp.parameter_transformer = self.parameter_transformer
        vp.ctx = self.ctx
        return vp

    def _copy_vp(self, vp):
        new = copy.deepcopy(vp, {id(vp.parameter_transformer): vp.parameter_transformer})
        new.ctx = self.ctx
        return new

    def _copy_gp(self, gp):
        """A GP of its own for the history: data, hyper-parameters and host posterior records."""
        new = copy.deepcopy(gp)
        new.ctx = self.ctx
        return new

    def _seeded(self, fn, base, stage):
        """``fn`` with the run's ``rng`` and context and, per call, the next seed of (iteration, stage).  The count of a
        stage's calls runs on across the iterations of a run and is part of a checkpoint (``_stage_calls``)."""
        calls = self._stage_calls

        def call(*a, **kw):
            calls[stage] += 1
            return fn(*a, seed=stage_seed(base, self.iteration, stage, calls[stage]), ctx=self.ctx, **kw)

        return call

    def _skl(self, vp, vp_old, base, n):
        kls = vp.kl_div(vp2=vp_old, N=int(1e5), gauss_flag=self.options["kl_gauss"], rng=self.rng,
                        seed=stage_seed(base, self.iteration, 3, n))
        return max(0, 0.5 * np.sum(kls))

    # ---- the loop
    def optimize(self, on_iteration=None, *, checkpoint=None, checkpoint_every=1):
        """Run the inference: ``(vp, results)``.  ``on_iteration(driver)`` is called in every iteration right before the
        termination check, where the reference's tests wrap ``_check_termination_conditions``.  With a ``seed`` NumPy's
        global stream is seeded for the run and the caller's state is put back on return.

        ``checkpoint``: a path; ``save(checkpoint, overwrite=True)`` at the bottom of every ``checkpoint_every``-th
        iteration, after the history's ``random_state`` record, and once more after the loop with the final state.  On a
        driver that ``load`` returned unfinished, the call continues the saved run (module text)."""
        if checkpoint is not None and int(checkpoint_every) < 1:
            raise ValueError("optimize: checkpoint_every must be at least 1")
        resume, self._resume = self._resume, None
        if resume is not None:
            self._after_load(resume)
        go_on = resume is not None and resume["go_on"]
        with _numpy_stream(self.seed, 1, resume["numpy_state"] if go_on else None):
            return self._optimize(on_iteration, go_on, checkpoint, int(checkpoint_every))

    def _after_load(self, resume):
        """The device side of a load, at the first ``optimize`` after it: every kept object on the driver's context, the
        GP of a rewind re-updated where the logger's set is not the GP's, and the live GP's posterior installed again as
        the device built it where the device held it so at the save (and after a rewind)."""
        ctx, h = self.ctx, self.iteration_history
        for obj in [self.vp, self.gp] + list(h["vp"]) + list(h["gp"]):
            if obj is not None:
                obj.ctx = ctx
        if self.gp is None:
            return
        if resume["rewind"] and int(np.sum(self.function_logger.X_flag)) != self.gp.X.shape[0]:
            self.gp = gp_mod.reupdate(self.function_logger, self.gp, ctx=ctx)
        elif resume["rewind"] or self._gp_dev_at_save:
            if not gp_mod.reinstall(self.gp, ctx=ctx):
                self.logger.warning("The GP of the checkpoint could not be installed as the device had built it: the resumed "
                                    "run is not bit-exact.")

    def _optimize(self, on_iteration, resumed=False, checkpoint=None, checkpoint_every=1):
        options, timer = self.options, self.timer
        if resumed:  # the saved run goes on: its base seed, its call counters, its message
            base = self._base_seed
        else:
            base = int(self.seed) if self.seed is not None else int(np.random.randint(0, 2**62, dtype=np.int64))
            self._base_seed = base
            self._stage_calls = {1: 0, 2: 0}
            self._termination_message = ""
        self.logger.info("Beginning variational optimization assuming %s observations of the log-joint",
                         "NOISY" if self.optim_state["uncertainty_handling_level"] > 0 else "EXACT")
        if self.is_finished:
            self.logger.warning("Continuing optimization from previous state.")
            self.is_finished = False
            self.vp = self._copy_vp(self.iteration_history["vp"][-1])
            self.optim_state = _copy_state(self.iteration_history["optim_state"][-1])
        train = self._seeded(lambda *a, seed, ctx, **kw: train_gp(*a, seed=seed, ctx=ctx, **kw), base, 1)
        fit = self._seeded(lambda *a, seed, ctx, **kw: optimize_vp(*a, rng=self.rng, seed=seed, ctx=ctx, **kw), base, 2)
        vp_old = None

        while not self.is_finished:
            self.iteration += 1
            it = self.iteration
            timer.reset()
            optim_state = self.optim_state
            optim_state["iter"] = it
            optim_state["redo_roto_scaling"] = False
            vp_old = self._copy_vp(self.vp)
            self.logging_action = []
            if it == 0 and optim_state["warmup"]:
                self.logging_action.append("start warm-up")
            # the deterministic entropy is given up towards the end of the budget (:876-884; the fraction is an option:
            # the reference looks it up in optim_state, where it is never stored)
            if optim_state["entropy_switch"] and (
                    self.function_logger.func_count >= options["entropy_force_switch"] * optim_state["max_fun_evals"]):
                optim_state["entropy_switch"] = False
                self.logging_action.append("entropy switch")
            # (:886-1030 input warping: refused in the constructor)

            # ---- active sampling (:1032-1115)
            timer.start_timer("active_sampling")
            self.parameter_transformer = self.vp.parameter_transformer
            self.function_logger.parameter_transformer = self.parameter_transformer
            new_funevals = options["fun_eval_start"] if it == 0 else options["fun_evals_per_iter"]
            if self.function_logger.Xn >= 0:
                self.function_logger.y_max = np.max(self.function_logger.y[self.function_logger.X_flag])
            if optim_state["skip_active_sampling"]:
                optim_state["skip_active_sampling"] = False
            else:
                optim_state["hyp_dict"] = self.hyp_dict
                self.function_logger, optim_state, self.vp, self.gp = active_sample(
                    self.gp, new_funevals, optim_state, self.function_logger, self.iteration_history, self.vp, options,
                    rng=self.rng, seed=stage_seed(base, it, 0), ctx=self.ctx, timer=timer, train_gp=train, optimize_vp=fit)
                self.optim_state = optim_state
                self.hyp_dict = optim_state["hyp_dict"]
                self._own(self.vp)
            optim_state["N"] = self.function_logger.Xn + 1
            optim_state["n_eff"] = np.sum(self.function_logger.n_evals[self.function_logger.X_flag])
            timer.stop_timer("active_sampling")

            # ---- the GP (:1117-1139)
            timer.start_timer("gp_train")
            self.gp, Ns_gp, sn2_hpd, self.hyp_dict = train(self.hyp_dict, optim_state, self.function_logger,
                                                           self.iteration_history, options, optim_state["plb_tran"],
                                                           optim_state["pub_tran"])
            gp_mod.fetch_posteriors(self.gp, self.ctx)  # host records: a GP of the history can be installed again
            optim_state["sn2_hpd"] = sn2_hpd
            timer.stop_timer("gp_train")
            if Ns_gp == options["stable_gp_samples"] and optim_state["stop_sampling"] == 0:
                optim_state["stop_sampling"] = optim_state["N"]

            # ---- the variational fit (:1141-1192)
            timer.start_timer("variational_fit")
            if not self.vp.optimize_mu:  # components fixed to the training inputs
                self.vp.mu = self.gp.X.T.copy()
                Knew = self.vp.mu.shape[1]
            else:
                Knew = rules.update_K(optim_state, self.iteration_history, options)
            N_fastopts = math.ceil(options.eval("ns_elbo", {"K": self.vp.K}))
            if optim_state["recompute_var_post"] or options["always_refit_vp"]:
                N_slowopts = options["elbo_starts"]
                optim_state["recompute_var_post"] = False
            else:  # only an incremental change from the previous iteration
                N_fastopts = math.ceil(N_fastopts * options["ns_elbo_incr"])
                N_slowopts = 1
            self.vp, var_ss, pruned = fit(options, optim_state, self.vp, self.gp, N_fastopts, N_slowopts, Knew)
            self._own(self.vp)
            optim_state["vp_K"] = self.vp.K
            optim_state["H"] = self.vp.stats["entropy"]
            elbo, elbo_sd = self.vp.stats["elbo"], self.vp.stats["elbo_sd"]
            timer.stop_timer("variational_fit")

            # ---- finalize (:1194-1261)
            timer.start_timer("finalize")
            sKL = self._skl(self.vp, vp_old, base, 0)
            f_mu, f_s2 = self.gp.predict(self.gp.X, self.gp.y, self.gp.s2, add_noise=False, ctx=self.ctx)
            optim_state["lcb_max"] = np.amax(f_mu - options["elcbo_impro_weight"] * np.sqrt(f_s2))
            sKL_true = None  # (true_mean / true_cov are debugging options of the reference; not compared here)
            mubar, sigma = self.vp.moments(orig_flag=False, cov_flag=True)
            optim_state["run_mean"], optim_state["run_cov"], optim_state["last_run_avg"] = rules.running_moments(
                optim_state["run_mean"], optim_state["run_cov"], optim_state["last_run_avg"], mubar, sigma, optim_state["N"],
                options["moments_run_weight"])
            timer.stop_timer("finalize")

            # the history keeps SNAPSHOTS, as the reference's deep-copying record does: the live GP goes on into the next
            # active sampling, which appends to it in place, and is re-updated on the trimmed set at the end of warm-up
            for key, value in (("iter", it), ("vp", self._copy_vp(self.vp)), ("elbo", elbo), ("elbo_sd", elbo_sd), ("var_ss", var_ss),
                               ("sKL", sKL), ("sKL_true", sKL_true), ("gp", self._copy_gp(self.gp)),
                               ("gp_hyp_full", self.gp.get_hyperparameters(as_array=True)), ("Ns_gp", Ns_gp),
                               ("pruned", pruned), ("timer", dict(timer.durations)),
                               ("func_count", self.function_logger.func_count), ("lcb_max", optim_state["lcb_max"]),
                               ("n_eff", optim_state["n_eff"]), ("function_logger", _copy_logger(self.function_logger))):
                self._record(key, value, it)
            # (:1288-1296 the ``stop_gp_sampling`` / ``_is_gp_sampling_finished`` branch is dead in the reference --
            # ``optim_state`` never gets the key and ``gp_sample_var`` is not a history key -- and is not mirrored)

            # ---- termination (:1298-1307)
            if on_iteration is not None:
                on_iteration(self)
            self.is_finished, message = self._check_termination_conditions()
            if message:
                self._termination_message = message
            self.vp.stats["stable"] = self.iteration_history["stable"][it]

            # ---- still warming up? (:1309-1342)
            if optim_state["warmup"] and it > 0:
                if self._check_warmup_end_conditions():
                    self._setup_vbmc_after_warmup()
                    self.gp = gp_mod.reupdate(self.function_logger, self.gp, ctx=self.ctx)  # the GP of the trimmed set
                if not optim_state["warmup"]:
                    self.vp.optimize_mu = options["variable_means"]
                    self.vp.optimize_weights = options["variable_weights"]
                    self.hyp_dict["runcov"] = None
                    optim_state["vp_repo"] = []
            self._record("warmup", optim_state["warmup"], it)

            # ---- fitness shaping (:1344-1367)
            if optim_state["out_warp_delta"] != [] and optim_state["R"] is not None and (
                    optim_state["R"] < options["warp_tol_reliability"]):
                Xrnd, _ = self.vp.sample(N=int(2e4), orig_flag=False, rng=self.rng, seed=stage_seed(base, it, 3, 2))
                ymu, _ = self.gp.predict(Xrnd, add_noise=True, ctx=self.ctx)
                ydelta = max([0, self.function_logger.y_max - np.quantile(ymu, 1e-3)])
                if ydelta > optim_state["out_warp_delta"] * options["out_warp_thresh_tol"] and optim_state["R"] < 1:
                    optim_state["out_warp_delta"] = optim_state["out_warp_delta"] * options["out_warp_thresh_mult"]

            if Ns_gp == options["stable_gp_samples"] and (
                    self.iteration_history["Ns_gp"][max(0, it - 1)] > options["stable_gp_samples"]):
                self.logging_action.append("switch to GP opt" if Ns_gp == 0 else "stable GP sampling")
            self.logger.info("%5d %8d %12.2f %12.2f %12.2f %5d %10.3g   %s", it, self.function_logger.func_count, elbo,
                             elbo_sd, sKL, self.vp.K, optim_state["R"], ", ".join(self.logging_action))
            self._record("logging_action", self.logging_action, it)
            self._record("data_trim_list", list(optim_state["data_trim_list"]), it)
            self._record("optim_state", _copy_state(optim_state), it)
            self._record("random_state", np.random.get_state(), it)
            for k in STAGES[:4]:
                self.timings[k] += timer.durations.get(k, 0.0)
            if checkpoint is not None and (it + 1) % checkpoint_every == 0:
                self._write_checkpoint(checkpoint)

        # ---- after the loop (:1493-1585)
        t0 = time.perf_counter()
        self.vp, elbo, elbo_sd, idx_best = self.determine_best_vp()
        changed_flag = False
        if options["do_final_boost"]:
            self.vp, elbo, elbo_sd, changed_flag = self.final_boost(self.vp, self.iteration_history["gp"][idx_best])
        if changed_flag:
            sKL = self._skl(self.vp, vp_old, base, 1) if vp_old is not None else -1
            self.logger.info("  inf %8d %12.2f %12.2f %12.2f %5d %10.3g   finalize", self.function_logger.func_count, elbo,
                             elbo_sd, sKL, self.vp.K, self.iteration_history["r_index"][idx_best])
        self.timings["boost"] += time.perf_counter() - t0
        success_flag = bool(self.vp.stats["stable"])
        termination_message = self._termination_message
        self.logger.warning(termination_message)
        self.logger.warning("Estimated ELBO: {:.3f} +/-{:.3f}.".format(elbo, elbo_sd))
        if not success_flag:
            self.logger.warning("Caution: Returned variational solution may have not converged.")
        results = self._create_result_dict(idx_best, termination_message, success_flag)
        if checkpoint is not None:
            self._write_checkpoint(checkpoint)
        return self._copy_vp(self.vp), results

    # ---- save, load, checkpoints (module text)
    def _write_checkpoint(self, file):
        t0 = time.perf_counter()
        path = self.save(file, overwrite=True)
        self.checkpoint_log.append((self.iteration, time.perf_counter() - t0, os.path.getsize(path)))

    def save(self, file, overwrite=False):
        """Write the driver to ``file`` (:2148-2184): ``.pkl`` is appended to a name without a suffix, ``FileExistsError``
        for an existing file unless ``overwrite``.  One dump of the whole object, written atomically (_persist.py); with it
        go NumPy's global stream state at this moment and whether the context holds the live GP's posterior as the device
        built it.  A target that plain ``pickle`` refuses needs ``dill`` (module text).  Returns the path written."""
        self._numpy_state = np.random.get_state()
        ctx = self._ctx
        dev_key = getattr(ctx, "_gp_dev", None) if ctx is not None and self.gp is not None else None
        self._gp_dev_at_save = dev_key is not None and dev_key == gp_mod._gp_fingerprint(self.gp)[0]  # (no context: its caches stay)
        return _persist.save(self, file, overwrite)

    @classmethod
    def load(cls, file, new_options=None, iteration=None, set_random_state=False, *, ctx=None):
        """The driver ``save`` wrote (:2186-2273), on ``ctx`` (default: the default context, opened when first needed; the
        load itself touches no device).  Loading a pickle runs code: load only files you wrote yourself.

        ``new_options``: a dict of options to change, validated as the constructor validates them (an unknown name
        raises ``ValueError``; what the constructor refuses is refused here) -- a larger ``max_fun_evals``, say, to go on
        from a finished run, which ``optimize()`` then does from the last iteration's posterior.
        ``iteration=None``: the live state of the file; an unfinished run is then resumed EXACTLY by ``optimize()`` (module
        text).  ``iteration=k``, earlier than the last: the posterior, the GP, the logger and the state (with its
        ``hyp_dict``) are copies of the history's snapshots of iteration k, every history list is cut to ``k + 1`` entries
        and the posterior's ``optimize_mu`` / ``optimize_weights`` follow that state's ``warmup``.  Such a rewind is a valid
        state to go on from, NOT the exact continuation: the snapshots are taken at different points of an iteration.
        ``ValueError`` for a ``k`` outside ``0 .. last``.
        ``set_random_state``: NumPy's global stream is set to the state recorded at the end of that iteration."""
        vbmc = _persist.load(file)
        if not isinstance(vbmc, cls):
            raise TypeError(f"{file}: holds a {type(vbmc).__name__}, not a {cls.__name__}")
        last = vbmc.iteration
        if iteration is None:
            iteration = last
        elif not (0 <= iteration <= last):
            raise ValueError(f"Specified iteration ({iteration}) should be >= 0 and <= last stored iteration ({last}).")
        iteration = int(iteration)
        h, rewind = vbmc.iteration_history, iteration < last
        if rewind:
            tr = vbmc.parameter_transformer
            vbmc.vp = copy.deepcopy(h["vp"][iteration], {id(tr): tr})
            vbmc.gp = copy.deepcopy(h["gp"][iteration])
            vbmc.function_logger = _copy_logger(h["function_logger"][iteration])
            vbmc.optim_state = _copy_state(h["optim_state"][iteration])
            if vbmc.optim_state.get("hyp_dict") is not None:
                vbmc.hyp_dict = vbmc.optim_state["hyp_dict"]
            vbmc.iteration = iteration
            for k in h:
                h[k] = h[k][: iteration + 1]
            if not vbmc.optim_state["warmup"]:  # (as the loop sets them where warm-up ends)
                vbmc.vp.optimize_mu = vbmc.options["variable_means"]
                vbmc.vp.optimize_weights = vbmc.options["variable_weights"]
            vbmc.logging_action = list(h["logging_action"][iteration])
        if new_options is not None:
            vbmc.options.revise(new_options)
            _refuse(vbmc.D, vbmc.options, vbmc.optim_state)
            vbmc._set_display()
        if set_random_state and iteration >= 0:
            np.random.set_state(h["random_state"][iteration])
        vbmc._ctx = ctx
        # for the first ``optimize()``: ``go_on`` -- an unfinished run continues at ``iteration + 1`` on the saved seed,
        # counters and stream (a finished one takes the "Continuing optimization" branch, seeded as a run of its own)
        go_on = iteration >= 0 and not vbmc.is_finished
        state = None
        if go_on:
            state = h["random_state"][iteration] if rewind or vbmc._numpy_state is None else vbmc._numpy_state
        vbmc._resume = {"rewind": rewind, "go_on": go_on, "numpy_state": state}
        return vbmc

    # ---- the decisions: driver_rules.py applied to the driver's state
    def _check_termination_conditions(self):
        """:1735-1843 -- records ``r_index``, ``elcbo_impro`` and ``stable`` of the iteration; ``(finished, message)``."""
        h, s, it = self.iteration_history, self.optim_state, self.optim_state["iter"]
        t = rules.termination(it, self.function_logger.func_count, h["elbo"], h["elbo_sd"], h["sKL"], h["func_count"],
                              h["r_index"][:it], s["sn2_hpd"], s["entropy_switch"], s.get("last_successful_warping", 0),
                              self.options)
        self._record("r_index", t.r_index, it)
        self._record("elcbo_impro", t.elcbo_impro, it)
        self._record("stable", t.stable, it)
        s["R"] = t.r_index
        s["entropy_switch"] = t.entropy_switch
        self.logging_action.extend(t.actions)
        return t.finished, t.message

    def _check_warmup_end_conditions(self):
        """:1587-1667."""
        h, s = self.iteration_history, self.optim_state
        return rules.warmup_should_end(s["iter"], h["elbo"], h["elbo_sd"], h["lcb_max"], h["func_count"],
                                       self.function_logger.func_count, s["data_trim_list"], s["N"], self.options)

    def _setup_vbmc_after_warmup(self):
        """:1669-1733 -- ends warm-up or, on a false alarm, only trims the training set."""
        s, log = self.optim_state, self.function_logger
        a = rules.after_warmup(s["iter"], self.iteration_history["r_index"][s["iter"]], s["data_trim_list"], s["N"],
                               log.y_orig, log.Xn, log.X_flag, self.D, s["warmup"], s["last_warmup"], self.options)
        s["warmup"], s["last_warmup"], s["data_trim_list"] = a.warmup, a.last_warmup, a.data_trim_list
        self.logging_action.extend(a.actions)
        log.X_flag = a.X_flag
        s["skip_active_sampling"] = a.skip_active_sampling
        s["recompute_var_post"] = a.recompute_var_post

    # ---- finalizing
    def determine_best_vp(self, max_idx=None, safe_sd=5, frac_back=0.25, rank_criterion_flag=False):
        """The best posterior of the run, its ELBO, the ELBO's SD and its iteration (:2040-2146)."""
        h = self.iteration_history
        if max_idx is None:
            max_idx = h["iter"][-1]
        idx_best = rules.best_iteration(h["stable"], h["elbo"], h["elbo_sd"], h["r_index"], max_idx, safe_sd, frac_back,
                                        rank_criterion_flag)
        vp = h["vp"][idx_best]
        vp.stats["stable"] = h["stable"][idx_best]
        return vp, h["elbo"][idx_best], h["elbo_sd"][idx_best], idx_best

    def final_boost(self, vp, gp):
        """A last variational fit of ``vp`` on ``gp`` with ``min_final_components`` components and the boost's entropy
        samples (:1938-2038): ``(vp, elbo, elbo_sd, changed_flag)``."""
        vp = self._copy_vp(vp)
        plan = rules.final_boost_plan(vp.K, self.options)
        if plan.do_boost:
            options = self.options.with_overrides(**plan.overrides)
            self.optim_state["warmup"] = False
            vp.optimize_mu = options["variable_means"]
            vp.optimize_weights = options["variable_weights"]
            self.optim_state["entropy_alpha"] = 0
            stable_flag = np.copy(vp.stats["stable"])
            base = getattr(self, "_base_seed", 0 if self.seed is None else int(self.seed))
            vp, _, _ = optimize_vp(options, self.optim_state, vp, gp, plan.n_fast_opts, plan.n_slow_opts, plan.K_new,
                                   rng=self.rng, seed=stage_seed(base, self.iteration, 4), ctx=self.ctx)
            self._own(vp)
            vp.stats["stable"] = stable_flag
        return vp, vp.stats["elbo"], vp.stats["elbo_sd"], plan.do_boost

    def _create_result_dict(self, idx_best, termination_message, success_flag):
        """:2275-2319.  (``problem_type`` is the reference's test on the TRANSFORMED bounds, which are infinite for a
        bounded variable as well.)"""
        h, s = self.iteration_history, self.optim_state
        unconstrained = np.all(np.isinf(s["lb_tran"])) and np.all(np.isinf(s["ub_tran"]))
        return {"function": str(self.function_logger.fun), "problem_type": "unconstrained" if unconstrained else "bounded",
                "iterations": s["iter"], "func_count": self.function_logger.func_count, "best_iter": idx_best,
                "train_set_size": h["n_eff"][idx_best], "components": self.vp.K, "r_index": h["r_index"][idx_best],
                "convergence_status": "probable" if h["stable"][idx_best] else "no", "overhead": np.nan, "rng_state": "rng",
                "algorithm": ALGORITHM, "version": VERSION, "message": termination_message, "elbo": self.vp.stats["elbo"],
                "elbo_sd": self.vp.stats["elbo_sd"], "success_flag": success_flag, "timings": dict(self.timings)}


__all__ = ["VBMC", "bounds_check", "init_optim_state", "stage_seed", "StageTimer", "HISTORY_KEYS", "STAGES"]
