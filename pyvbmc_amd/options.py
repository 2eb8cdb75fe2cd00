"""``Options``: the option set of a VBMC run -- a ``dict`` with ``.eval(name, {"K": K})``, which is what every stage of the
package accepts (``sieve._opt``).

The defaults are the table below: one row per option, ``name: (line, value)``, written by hand from the reference's two
option files -- ``B`` lines cite ``vbmc/option_configs/basic_vbmc_options.ini``, ``A`` lines
``advanced_vbmc_options.ini``.  A value that depends on the problem dimension is ``AtD(f)`` and is evaluated once, at
construction; a value that depends on K (or N) stays a callable and is evaluated by ``.eval``.  The acquisition functions
are named by their constructor strings, which ``acquisition.as_package_acq`` turns into the package's classes.

User options override the defaults; an unknown name raises ``ValueError`` (the reference's ``validate_option_names``).
After construction an item is set only with ``options.__setitem__(key, value, force=True)``, as in the reference.

Pickling.  The table holds lambdas, which plain ``pickle`` does not take, so an ``Options`` is written as its items with
every callable that is still the table's own named by its key and looked up in ``DEFAULTS`` again on load; every other
value is pickled as it is.  A user's callable that plain ``pickle`` refuses (a lambda, a closure) is written with ``dill``
where ``dill`` imports, and raises a ``TypeError`` naming the option where it does not.
"""
import copy
import pickle
from math import ceil

import numpy as np


class AtD:
    """A default that is a function of the dimension D."""

    def __init__(self, f):
        self.f = f


def _zero(N, NMAX):
    return 0


DEFAULTS = {
    # ---- basic
    "display": ("B3", "iter"),
    "plot": ("B5", False),
    "max_iter": ("B7", AtD(lambda D: 50 * (2 + D))),
    "max_fun_evals": ("B9", AtD(lambda D: 50 * (2 + D))),
    "fun_evals_per_iter": ("B11", 5),
    "tol_stable_count": ("B13", 60),
    "min_final_components": ("B15", 50),
    "specify_target_noise": ("B17", False),
    "log_file_name": ("B19", None),
    "log_file_level": ("B21", "iter"),
    "log_file_mode": ("B23", "a"),
    "print_iteration_header": ("B25", None),
    # ---- advanced
    "uncertainty_handling": ("A3", []),
    "integer_vars": ("A5", []),
    "noise_size": ("A7", []),
    "max_repeated_observations": ("A9", 0),
    "fun_eval_start": ("A11", AtD(lambda D: np.maximum(D, 10))),
    "sgd_step_size": ("A13", 0.005),
    "skip_active_sampling_after_warmup": ("A15", False),
    "rank_criterion": ("A17", True),
    "tol_stable_entropy_iters": ("A19", 6),
    "variable_means": ("A21", True),
    "variable_weights": ("A23", True),
    "weight_penalty": ("A25", 0.1),
    "diagnostics": ("A27", False),
    "output_fcn": ("A29", []),
    "tol_stable_excpt_frac": ("A31", 0.2),
    "f_vals": ("A33", []),
    "proposal_fcn": ("A35", None),
    "nonlinear_scaling": ("A37", True),
    "search_acq_fcn": ("A39", ["AcqFcnLog()"]),
    "ns_search": ("A41", 2**13),
    "ns_ent": ("A43", lambda K: 100 * K ** (2 / 3)),
    "ns_ent_fast": ("A45", 0),
    "ns_ent_fine": ("A47", lambda K: 2**12 * K),
    "do_final_boost": ("A49", True),
    "ns_ent_boost": ("A51", lambda K: 200 * K ** (2 / 3)),
    "ns_ent_fast_boost": ("A53", []),
    "ns_ent_fine_boost": ("A55", []),
    "ns_ent_active": ("A57", lambda K: 20 * K ** (2 / 3)),
    "ns_ent_fast_active": ("A59", 0),
    "ns_ent_fine_active": ("A61", lambda K: 200 * K),
    "ns_elbo": ("A63", lambda K: 50 * K),
    "ns_elbo_incr": ("A65", 0.1),
    "elbo_starts": ("A67", 2),
    "ns_gp_max": ("A69", 80),
    "ns_gp_max_warmup": ("A71", 8),
    "ns_gp_max_main": ("A73", np.inf),
    "warmup_no_impro_threshold": ("A75", AtD(lambda D: 20 + 5 * D)),
    "warmup_check_max": ("A77", True),
    "stable_gp_sampling": ("A79", AtD(lambda D: 200 + 10 * D)),
    "stable_gp_vp_k": ("A81", np.inf),
    "stable_gp_samples": ("A83", 0),
    "gp_sample_thin": ("A85", 5),
    "gp_train_n_init": ("A87", 1024),
    "gp_train_n_init_final": ("A89", 64),
    "gp_train_init_method": ("A91", "rand"),
    "gp_tol_opt": ("A93", 1e-5),
    "gp_tol_opt_mcmc": ("A95", 1e-2),
    "gp_tol_opt_active": ("A97", 1e-4),
    "gp_tol_opt_mcmc_active": ("A99", 1e-2),
    "tol_gp_var": ("A101", 1e-4),
    "tol_gp_var_mcmc": ("A103", 1e-4),
    "gp_mean_fun": ("A105", "negquad"),
    "gp_int_mean_fun": ("A107", 0),
    "k_fun_max": ("A109", lambda N: N ** (2 / 3)),
    "k_warmup": ("A111", 2),
    "adaptive_k": ("A113", 2),
    "hpd_frac": ("A115", 0.8),
    "elcbo_impro_weight": ("A117", 3),
    "tol_length": ("A119", 1e-6),
    "cache_size": ("A121", 500),
    "cache_frac": ("A123", 0.5),
    "stochastic_optimizer": ("A125", "adam"),
    "tol_fun_stochastic": ("A127", 1e-3),
    "max_iter_stochastic": ("A129", AtD(lambda D: 100 * (2 + D))),
    "gp_stochastic_step_size": ("A131", False),
    "tol_sd": ("A133", 0.1),
    "tol_skl": ("A135", AtD(lambda D: 0.01 * np.sqrt(D))),
    "tol_stable_warmup": ("A137", 15),
    "variational_sampler": ("A139", "malasample"),
    "tol_improvement": ("A141", 0.01),
    "kl_gauss": ("A143", True),
    "true_mean": ("A145", []),
    "true_cov": ("A147", []),
    "min_fun_evals": ("A149", AtD(lambda D: 5 * D)),
    "min_iter": ("A151", AtD(lambda D: D)),
    "heavy_tail_search_frac": ("A153", 0.25),
    "mvn_search_frac": ("A155", 0.25),
    "hpd_search_frac": ("A157", 0),
    "box_search_frac": ("A159", 0.25),
    "search_cache_frac": ("A161", 0),
    "always_refit_vp": ("A163", False),
    "warmup": ("A165", True),
    "warmup_options": ("A167", []),
    "stop_warmup_thresh": ("A169", 0.2),
    "warmup_keep_threshold": ("A171", AtD(lambda D: 10 * D)),
    "warmup_keep_threshold_false_alarm": ("A173", AtD(lambda D: 100 * (D + 2))),
    "stop_warmup_reliability": ("A175", 100),
    "search_optimizer": ("A177", "cmaes"),
    "search_cmaes_vp_init": ("A179", True),
    "search_cmaes_best": ("A181", False),
    "search_max_fun_evals": ("A183", AtD(lambda D: 500 * (D + 2))),
    "moments_run_weight": ("A185", 0.9),
    "gp_retrain_threshold": ("A187", 1),
    "elcbo_midpoint": ("A189", True),
    "gp_sample_widths": ("A191", 5),
    "hyp_run_weight": ("A193", 0.9),
    "weighted_hyp_cov": ("A195", True),
    "tol_cov_weight": ("A197", 0),
    "gp_hyp_sampler": ("A199", "slicesample"),
    "cov_sample_thresh": ("A201", 10),
    "det_entropy_tol_opt": ("A203", 1e-3),
    "entropy_switch": ("A205", False),
    "entropy_force_switch": ("A207", 0.8),
    "det_entropy_alpha": ("A209", 0),
    "update_random_alpha": ("A211", False),
    "adaptive_entropy_alpha": ("A213", False),
    "det_entropy_min_d": ("A215", 5),
    "tol_con_loss": ("A217", 0.01),
    "best_safe_sd": ("A219", 5),
    "best_frac_back": ("A221", 0.25),
    "tol_weight": ("A223", 1e-2),
    "pruning_threshold_multiplier": ("A225", lambda K: 1 / np.sqrt(K)),
    "annealed_gp_mean": ("A227", _zero),
    "constrained_gp_mean": ("A229", False),
    "empirical_gp_prior": ("A231", False),
    "tol_gp_noise": ("A233", np.sqrt(1e-5)),
    "gp_length_prior_mean": ("A235", AtD(lambda D: np.sqrt(D / 6))),
    "gp_length_prior_std": ("A237", 0.5 * np.log(1e3)),
    "upper_gp_length_factor": ("A239", 0),
    "init_design": ("A241", "plausible"),
    "gp_quadratic_mean_bound": ("A243", True),
    "fitness_shaping": ("A245", False),
    "out_warp_thresh_base": ("A247", AtD(lambda D: 10 * D)),
    "out_warp_thresh_mult": ("A249", 1.25),
    "out_warp_thresh_tol": ("A251", 0.8),
    "temperature": ("A253", 1),
    "separate_search_gp": ("A255", False),
    "noise_shaping": ("A257", False),
    "noise_shaping_threshold": ("A259", AtD(lambda D: 10 * D)),
    "noise_shaping_factor": ("A261", 0.05),
    "acq_hedge": ("A263", False),
    "acq_hedge_iter_window": ("A265", 4),
    "acq_hedge_decay": ("A267", 0.9),
    "active_variational_samples": ("A269", 0),
    "scale_lower_bound": ("A271", True),
    "active_sample_vp_update": ("A273", False),
    "active_sample_gp_update": ("A275", False),
    "active_sample_full_update_past_warmup": ("A277", 2),
    "active_sample_full_update_threshold": ("A279", 3),
    "variational_init_repo": ("A281", False),
    "sample_extra_vp_means": ("A283", 0),
    "optimistic_variational_bound": ("A285", 0),
    "active_importance_sampling_vp_samples": ("A287", 100),
    "active_importance_sampling_box_samples": ("A289", 100),
    "active_importance_sampling_mcmc_samples": ("A291", 100),
    "active_importance_sampling_mcmc_thin": ("A293", 1),
    "active_sample_fess_thresh": ("A295", 1),
    "active_importance_sampling_fess_thresh": ("A297", 0.9),
    "active_search_bound": ("A299", 2),
    "integrate_gp_mean": ("A301", False),
    "tol_bound_x": ("A303", 1e-5),
    "recompute_lcb_max": ("A305", True),
    "bounded_transform": ("A307", "probit"),
    "double_gp": ("A309", False),
    "warp_every_iters": ("A311", 5),
    "incremental_warp_delay": ("A313", True),
    "warp_tol_reliability": ("A315", 3),
    "warp_rotoscaling": ("A317", True),
    "warp_cov_reg": ("A319", 0),
    "warp_roto_corr_thresh": ("A321", 0.05),
    "warp_min_k": ("A323", 5),
    "warp_undo_check": ("A325", True),
    "warp_tol_improvement": ("A327", 0.1),
    "warp_tol_sd_multiplier": ("A329", 2),
    "warp_tol_sd_base": ("A331", 1),
}


def _default_of(key, D):
    value = DEFAULTS[key][1]
    return value.f(D) if isinstance(value, AtD) else value


def _import_dill():
    try:
        import dill
    except ImportError:
        return None
    return dill


def _restore_options(D, useroptions, is_initialized, attrs, items):
    """Unpickling: ``items`` are ``(key, how, payload)`` in the dict's order -- ``how`` "default" (the table's callable of
    that key), "value" (the value itself) or "dill" (a callable as ``dill.dumps`` wrote it)."""
    new = Options.__new__(Options)
    new.__dict__.update(attrs)
    new.D, new.useroptions = D, set(useroptions)
    for key, how, payload in items:
        if how == "default":
            payload = _default_of(key, D)
        elif how == "dill":
            dill = _import_dill()
            if dill is None:
                raise TypeError(f"option {key!r} was saved with dill, which is not installed")
            payload = dill.loads(payload)
        dict.__setitem__(new, key, payload)
    new.is_initialized = is_initialized
    return new


class Options(dict):
    """``Options(D, user_options=None)``: the defaults at dimension ``D`` with the user's values over them."""

    def __init__(self, D, user_options=None):
        super().__init__()
        self.is_initialized = False
        self.D = D
        user_options = {} if user_options is None else dict(user_options)
        for key in user_options:
            if key not in DEFAULTS:
                raise ValueError("The option {} does not exist.".format(key))
        for key, (_, value) in DEFAULTS.items():
            self[key] = value.f(D) if isinstance(value, AtD) else copy.copy(value)
        self.update(user_options)
        self.useroptions = set(user_options)
        self.update_defaults()
        self.is_initialized = True

    def update_defaults(self):
        """Defaults that follow from other options (reference ``options.py`` :68-80): a target that reports its noise gets
        half again the budget, full updates inside active sampling and the VIQR acquisition -- unless the user set them."""
        if self.get("specify_target_noise"):
            for key, val in (("max_fun_evals", ceil(self["max_fun_evals"] * 1.5)),
                             ("tol_stable_count", ceil(self["tol_stable_count"] * 1.5)),
                             ("active_sample_gp_update", True), ("active_sample_vp_update", True),
                             ("search_acq_fcn", ["AcqFcnVIQR()"])):
                if key not in self.useroptions:
                    dict.__setitem__(self, key, val)

    def __setitem__(self, key, val, force=False):
        if getattr(self, "is_initialized", False) and not force:
            raise AttributeError("Cannot set options after initialization. Please re-initialize with `options = {...}`")
        dict.__setitem__(self, key, val)

    def eval(self, key, evaluation_parameters):
        """The option's value, called with ``evaluation_parameters`` (by keyword) when it is a callable."""
        v = self.get(key)
        return v(**evaluation_parameters) if callable(v) else v

    def revise(self, new_options):
        """Change items of a finished option set by name, with the constructor's validation (an unknown name raises
        ``ValueError``): what ``VBMC.load(new_options=...)`` does, ``is_initialized`` toggled as in the reference."""
        new_options = dict(new_options)
        for key in new_options:
            if key not in DEFAULTS:
                raise ValueError("The option {} does not exist.".format(key))
        self.is_initialized = False
        try:
            self.update(new_options)
            self.useroptions = set(self.useroptions) | set(new_options)
        finally:
            self.is_initialized = True

    def __reduce__(self):
        """Plain ``pickle`` (module text): the table's own callables by key, everything else as it is."""
        items = []
        for key, v in self.items():
            if callable(v):
                if key in DEFAULTS and v is DEFAULTS[key][1]:
                    items.append((key, "default", None))
                    continue
                try:
                    pickle.dumps(v)
                except Exception as exc:
                    dill = _import_dill()
                    if dill is None:
                        raise TypeError(f"option {key!r}: its value {v!r} cannot be pickled (a lambda or a closure); make it "
                                        "a module-level function, or install dill") from exc
                    items.append((key, "dill", dill.dumps(v)))
                    continue
            items.append((key, "value", v))
        attrs = {k: v for k, v in self.__dict__.items() if k not in ("D", "useroptions", "is_initialized")}
        return _restore_options, (self.D, sorted(self.useroptions), self.is_initialized, attrs, items)

    def __copy__(self):
        new = Options.__new__(Options)
        new.__dict__.update(self.__dict__)
        dict.update(new, self)
        return new

    def __deepcopy__(self, memo):
        new = Options.__new__(Options)
        memo[id(self)] = new
        new.__dict__.update(copy.deepcopy(self.__dict__, memo))
        for k, v in self.items():
            dict.__setitem__(new, k, v if callable(v) else copy.deepcopy(v, memo))
        return new

    def with_overrides(self, **over):
        """A copy with some items replaced (what the final boost and the local updates need)."""
        new = copy.copy(self)
        for k, v in over.items():
            new.__setitem__(k, v, force=True)
        return new


__all__ = ["Options", "DEFAULTS", "AtD"]
