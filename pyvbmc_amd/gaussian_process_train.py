"""GP training for VBMC: the mirror of the reference's ``pyvbmc/vbmc/gaussian_process_train.py`` over this package's
``GP`` and its fused fit (``GP.fit(optimizer="fused")``: vbmc_gp_fit, one device call that leaves the posterior installed).

Names and return values are the reference's; every function cites the reference lines it mirrors.  What the reference
decides is reproduced exactly -- the noise size and prior by ``uncertainty_handling_level``, the length-scale upper
bound, the mean-constant bounds, the squared-exponential lower bounds from the high-posterior-density set, the Student-t
priors, the number of samples, the training options, the hyper-parameter covariance, the ``hyp0`` assembly with its draws
from NumPy's global stream, the running covariance and the noise estimate (tests/golden/train_gp.npz records the
reference's own results).

What is THIS PACKAGE'S OWN, because gpyreg is not part of the reference tree:

* ``get_bounds_info`` of the covariance, mean and noise classes (pyvbmc_amd/gp.py states the rule);
* the box: ``GP.fit`` needs finite bounds and ``_gp_hyp`` leaves several infinite, so a bound that is NaN or infinite after
  the reference's rules is replaced by the matching ``LB`` / ``UB`` entry of the block's ``get_bounds_info(X, y)`` on the
  FULL data (``_close_box``);
* the design box of the drawn candidates: ``get_bounds_info``'s ``[PLB, PUB]`` on the full data, clipped into the final
  box -- the hard box spans twelve orders of magnitude in length scale;
* the fit itself: counter-based uniform design, the package's L-BFGS, S lockstep slice chains with one kept sample each.
  gpyreg's random stream, its Sobol design, its default bounds and its single long thinned chain are not reproduced.

``train_gp`` raises ``_lib.UnsupportedShape`` -- before any side effect on ``hyp_dict`` or on NumPy's global stream, so a
caller can fall back to the reference (``dropin.patch_train_gp``) -- for samplers other than ``slicesample``, covariance
functions other than the squared exponential, and the noise forms the package's ``GP`` does not take
(``noise_provided_log_multiplier``, rectified-linear output-dependent noise, ``uncertainty_handling_level`` 1).
"""
import math

import numpy as np

from . import _lib
from . import gp as _gp
from .sieve import get_hpd

_MEANS = {"zero": _gp.ZeroMean, "const": _gp.ConstantMean, "negquad": _gp.NegativeQuadratic}
_SAMPLERS = ("slicesample", "npv", "mala", "slicelite", "splitsample", "covsample", "laplace")


def _meanfun_name_to_mean_function(name):
    """The package's mean function by the reference's name (:200-228); ``ValueError`` for an unknown one."""
    if name not in _MEANS:
        raise ValueError("Unknown mean function!")
    return _MEANS[name]()


def _cov_identifier_to_covariance_function(identifier):
    """The covariance function by the reference's identifier (:231-262): 1 is the squared exponential; the Matern
    identifiers (3, [3, degree]) are known to the reference but not to this package (``UnsupportedShape``)."""
    if identifier == 1:
        return _gp.SquaredExponential()
    if identifier == 3 or (isinstance(identifier, list) and identifier and identifier[0] == 3):
        raise _lib.UnsupportedShape("train_gp: Matern covariance functions are not supported")
    raise ValueError("Unknown covariance function")


def _get_training_data(function_logger):
    """``(x_train, y_train, s2_train, t_train)`` (:739-772): ``gp.training_data`` plus the evaluation times."""
    X, y, s2 = _gp.training_data(function_logger)
    t = getattr(function_logger, "fun_eval_time", None)
    return X, y, s2, None if t is None else np.asarray(t)[function_logger.X_flag]


def reupdate_gp(function_logger, gp, **kw):
    """``reupdate_gp`` (:817-842): ``gp.reupdate``."""
    return _gp.reupdate(function_logger, gp, **kw)


def _noise_size_and_std(optim_state, options):
    """``(noise_size, noise_std)`` by ``uncertainty_handling_level`` (:325-346); level 1 (a noise multiplier with a prior
    of its own, :333-342) needs a hyper-parameter this package's noise has not."""
    min_noise = options["tol_gp_noise"]
    level = optim_state["uncertainty_handling_level"]
    if level == 1:
        raise _lib.UnsupportedShape("train_gp: uncertainty_handling_level 1 (noise_provided_log_multiplier) is not supported")
    if level == 0 and np.size(options["noise_size"]) > 0:
        return max(float(np.ravel(options["noise_size"])[0]), min_noise), 0.5
    return min_noise, 0.5


def _close_box(gp, X, y):
    """The package's own rule for the box (see the module text): every bound of ``gp`` that is NaN or infinite becomes the
    matching ``LB`` / ``UB`` entry of the block's ``get_bounds_info(X, y)`` on the full data, and the design box is
    ``[PLB, PUB]`` clipped into the result.  Sets the bounds on ``gp``; returns ``(lb, ub, design_lb, design_ub)``."""
    info = [gp.covariance.get_bounds_info(X, y), gp.noise.get_bounds_info(X, y), gp.mean.get_bounds_info(X, y)]
    LB, UB, PLB, PUB = (np.concatenate([np.ravel(i[k]) for i in info]) for k in ("LB", "UB", "PLB", "PUB"))
    b = gp.get_bounds(as_array=True)
    lb = np.where(np.isfinite(b["lb"]), b["lb"], LB)
    ub = np.where(np.isfinite(b["ub"]), b["ub"], UB)
    ub = np.maximum(ub, lb)  # (a reference-decided bound beyond the package's opposite one: the reference's wins)
    gp.set_bounds({"lb": lb, "ub": ub})
    dlb = np.minimum(np.maximum(PLB, lb), ub)
    dub = np.minimum(np.maximum(PUB, dlb), ub)
    return lb, ub, dlb, dub


def _gp_hyp(optim_state, options, plb_tran, pub_tran, gp, X, y):
    """Bounds, priors and the number of samples of the GP's hyper-parameters (:265-477); returns ``(gp, hyp0, gp_s_N)``.

    The reference's decisions, exactly: ``hyp0`` from the blocks' ``x0`` on the high-posterior-density set with the noise
    at ``log noise_size`` (:317-347); the length-scale upper bound ``log(upper_gp_length_factor (pub - plb))`` (:354-359)
    -- which under the squared exponential the reference then replaces, with its lower bound, by "not decided" (:385-388
    assign the same key again), and so does this; the noise lower bound ``log tol_gp_noise`` (:361); the mean constant's
    upper bound (:364-377); the squared exponential's lower bounds from the HPD set's ``get_bounds_info`` (:380-391); the
    Student-t priors on the noise and the length scales (:397-400, :436-443); ``gp_s_N`` and the ``stop_sampling`` rules
    (:451-472).  The name-keyed bounds are kept in ``gp.temporary_data["reference_bounds"]`` as the reference leaves them
    (with their infinities and NaNs); the package's own rule then closes the box (``_close_box`` on the full data) and
    leaves the design box in ``gp.temporary_data["design_box"]``."""
    hpd_X, hpd_y, _, _ = get_hpd(X, y, options["hpd_frac"])
    D = hpd_X.shape[1]
    cov_info = gp.covariance.get_bounds_info(hpd_X, hpd_y)
    mean_info = gp.mean.get_bounds_info(hpd_X, hpd_y)
    noise_info = gp.noise.get_bounds_info(hpd_X, hpd_y)
    min_noise = options["tol_gp_noise"]
    noise_size, noise_std = _noise_size_and_std(optim_state, options)
    noise_x0 = np.array(noise_info["x0"], dtype=np.float64)
    noise_x0[0] = np.log(noise_size)
    hyp0 = np.concatenate([np.ravel(cov_info["x0"]), noise_x0, np.ravel(mean_info["x0"])])

    width = np.ravel(pub_tran) - np.ravel(plb_tran)
    bounds = gp.get_bounds()
    if options["upper_gp_length_factor"] > 0:
        bounds["covariance_log_lengthscale"] = (-np.inf, np.log(options["upper_gp_length_factor"] * width))
    bounds["noise_log_scale"] = (np.log(min_noise), np.inf)
    if isinstance(gp.mean, _gp.ZeroMean):
        pass
    elif isinstance(gp.mean, _gp.ConstantMean):
        bounds["mean_const"] = (-np.inf, np.min(hpd_y))
    elif isinstance(gp.mean, _gp.NegativeQuadratic):
        if options["gp_quadratic_mean_bound"]:
            delta_y = max(options["tol_sd"], min(D, np.max(hpd_y) - np.min(hpd_y)))
            bounds["mean_const"] = (-np.inf, np.max(hpd_y) + delta_y)
    else:
        raise TypeError("The mean function is not supported.")
    if isinstance(gp.covariance, _gp.SquaredExponential):
        # (NaN: not decided here.  The length-scale entry REPLACES the one set above, as it does in the reference, whose
        # dict is set once at the end: under the squared exponential the reference leaves that upper bound to gpyreg)
        bounds["covariance_log_outputscale"] = (cov_info["LB"][D], np.nan)
        bounds["covariance_log_lengthscale"] = (cov_info["LB"][:D], np.nan)

    priors = gp.get_priors()
    priors["noise_log_scale"] = ("student_t", (np.log(noise_size), noise_std, 3))
    priors["covariance_log_lengthscale"] = (
        "student_t", (np.log(options["gp_length_prior_mean"] * width), options["gp_length_prior_std"], 3))
    gp.set_priors(priors)

    stop_sampling = optim_state["stop_sampling"]
    if stop_sampling == 0:
        gp_s_N = options["ns_gp_max"] / np.sqrt(optim_state["N"])
        gp_s_N = np.minimum(gp_s_N, options["ns_gp_max_warmup"] if optim_state["warmup"] else options["ns_gp_max_main"])
        if optim_state["N"] >= options["stable_gp_sampling"] or optim_state["vp_K"] >= options["stable_gp_vp_k"]:
            stop_sampling = optim_state["N"]
    if stop_sampling > 0:
        gp_s_N = options["stable_gp_samples"]

    gp.set_bounds(bounds)  # (a NaN entry leaves the slot as it was: not finite, so ``_close_box`` decides it)
    gp.temporary_data["reference_bounds"] = bounds
    lb, ub, dlb, dub = _close_box(gp, X, y)
    gp.temporary_data["design_box"] = (dlb, dub)
    return gp, hyp0, round(gp_s_N)


def _slice_widths(options, hyp_cov, r_index):
    """``max(sqrt(diag hyp_cov), 1e-3) max(gp_sample_widths, r_index)`` where both are there, else None (:534-537)."""
    if options["gp_sample_widths"] > 0 and hyp_cov is not None:
        return np.maximum(np.sqrt(np.diag(hyp_cov).T), 1e-3) * np.maximum(options["gp_sample_widths"], r_index)
    return None


def _get_gp_training_options(optim_state, iteration_history, options, hyp_dict, gp_s_N):
    """The options of a GP fit (:480-653): ``thin``, ``init_method``, ``tol_opt``, ``tol_opt_mcmc``, ``widths``, ``sampler``,
    ``init_N``, ``opts_N``, ``burn``, ``n_samples`` (and ``step_size`` for mala), for every sampler name the reference
    knows; ``ValueError`` for any other."""
    iteration = optim_state["iter"]
    r_index = iteration_history["r_index"][iteration - 1] if iteration > 0 else np.inf
    gp_train = {"thin": options["gp_sample_thin"], "init_method": options["gp_train_init_method"],
                "tol_opt": options["gp_tol_opt"], "tol_opt_mcmc": options["gp_tol_opt_mcmc"], "widths": None}
    hyp_cov = _get_hyp_cov(optim_state, iteration_history, options, hyp_dict)
    name = options["gp_hyp_sampler"]
    if name not in _SAMPLERS:
        raise ValueError("Unknown MCMC sampler for GP hyperparameters")
    gp_train["sampler"] = name
    if name in ("slicesample", "slicelite", "splitsample"):
        gp_train["widths"] = _slice_widths(options, hyp_cov, r_index)
    elif name == "mala":
        if hyp_cov is not None:
            gp_train["widths"] = np.sqrt(np.diag(hyp_cov).T)
        if "gp_mala_step_size" in optim_state:
            gp_train["step_size"] = optim_state["gp_mala_step_size"]
    elif name == "covsample":  # (:563-580)
        if options["gp_sample_widths"] > 0 and hyp_cov is not None:
            width_mult = np.maximum(options["gp_sample_widths"], r_index)
            if np.all(np.isfinite(width_mult)) and np.all(r_index < options["cov_sample_thresh"]):
                hyp_n = hyp_cov.shape[0]
                gp_train["widths"] = (hyp_cov + 1e-6 * np.eye(hyp_n)) * width_mult**2
                gp_train["thin"] *= math.ceil(np.sqrt(hyp_n))
            else:
                gp_train["widths"] = _slice_widths(options, hyp_cov, r_index)
                gp_train["sampler"] = "slicesample"
    elif name == "laplace" and optim_state["n_eff"] < 30:  # (:582-590)
        gp_train["sampler"] = "slicesample"
        gp_train["widths"] = _slice_widths(options, hyp_cov, r_index)

    # the N-dependent number of initial points: the cubic of :596-604 (its square and linear terms at the same x)
    a = -(options["gp_train_n_init"] - options["gp_train_n_init_final"])
    x = (optim_state["n_eff"] - options["fun_eval_start"]) / (min(options["max_fun_evals"], 1e3) - options["fun_eval_start"])
    init_N = max(round(a * x**3 + (-3 * a) * x**2 + (3 * a) * x + options["gp_train_n_init"]), 9)

    retrain = False
    if optim_state["recompute_var_post"]:
        gp_train["burn"] = gp_train["thin"] * gp_s_N
    else:
        gp_train["burn"] = gp_train["thin"] * 3
        retrain = iteration > 1 and iteration_history["r_index"][iteration - 1] < options["gp_retrain_threshold"]
    if retrain:  # (:616-642)
        gp_train["init_N"] = 0
        if name == "slicelite":
            r_last = iteration_history["r_index"][iteration - 1]
            sweeps = math.ceil(gp_train["thin"] * np.log(r_last / np.log(options["gp_retrain_threshold"])))
            gp_train["burn"] = max(1, sweeps) * gp_s_N
            gp_train["thin"] = 1
        gp_train["opts_N"] = 0 if gp_s_N > 0 else 1
    else:
        gp_train["init_N"] = init_N
        gp_train["opts_N"] = 1 if gp_s_N > 0 else 2
    gp_train["n_samples"] = round(gp_s_N)
    gp_train["burn"] = round(gp_train["burn"])
    return gp_train


def _get_hyp_cov(optim_state, iteration_history, options, hyp_dict):
    """The hyper-parameter posterior covariance of earlier iterations (:656-736): None at iteration 0; the running
    covariance ``hyp_dict["run_cov"]`` without ``weighted_hyp_cov``; else the weighted covariance of the samples in
    ``iteration_history["gp_hyp_full"]``, newest first, the weight of iteration ``iter - 1 - i`` shrinking by
    ``hyp_run_weight ** (fun_evals_per_iter max(1, log(sKL / tol_skl fun_evals_per_iter)))`` per step and the walk ending
    where it falls below ``tol_cov_weight``.  The array handling -- which axis the reference weights, which it sums --
    is the reference's, kept as it is."""
    it = optim_state["iter"]
    if it <= 0:
        return None
    if not options["weighted_hyp_cov"]:
        return hyp_dict["run_cov"]
    w_list, hyp_list, w = [], [], 1
    for i in range(it):
        if i > 0:
            diff_mult = max(1, np.log(iteration_history["sKL"][it - i] / options["tol_skl"] * options["fun_evals_per_iter"]))
            w *= options["hyp_run_weight"] ** (options["fun_evals_per_iter"] * diff_mult)
        if w < options["tol_cov_weight"]:
            break
        hyp = iteration_history["gp_hyp_full"][it - 1 - i]
        hyp_n = hyp.shape[1]
        if len(hyp_list) == 0 or np.shape(hyp_list)[2] == hyp.shape[0]:
            hyp_list.append(hyp.T)
            w_list.append(w * np.ones((hyp_n, 1)) / hyp_n)
    w_list = np.concatenate(w_list)
    hyp_list = np.concatenate(hyp_list)
    w_list /= np.sum(w_list, axis=0)
    mu_star = np.sum(hyp_list * w_list, axis=0)
    hyp_n = np.shape(hyp_list)[1]
    hyp_cov = np.zeros((hyp_n, hyp_n))
    for j in range(np.shape(hyp_list)[0]):
        dev = hyp_list[j] - mu_star
        hyp_cov += np.dot(w_list[j], np.dot(dev.T, dev))
    hyp_cov /= 1 - np.sum(w_list**2)
    return hyp_cov


def _estimate_noise(gp):
    """The GP's observation noise around the top of the posterior (:775-814): over the ``ceil(0.2 N)`` training points of
    largest ``y``, the median over the points of the noise variance averaged over the hyper-parameter samples."""
    N = gp.X.shape[0]
    order = np.argsort(gp.y, axis=None)[::-1][: math.ceil(0.2 * N)]
    hpd_X, hpd_y = gp.X[order], gp.y[order]
    hpd_s2 = None if gp.s2 is None else gp.s2[order]
    cov_N = gp.covariance.hyperparameter_count(gp.D)
    noise_N = gp.noise.hyperparameter_count()
    sn2 = np.zeros((hpd_X.shape[0], np.size(gp.posteriors)))
    for s, post in enumerate(gp.posteriors):
        sn2[:, s : s + 1] = gp.noise.compute(post.hyp[cov_N : cov_N + noise_N], hpd_X, hpd_y, hpd_s2)
    return np.median(np.mean(sn2, axis=1))


def _supported(optim_state, options):
    """Raise ``_lib.UnsupportedShape`` for what the package's ``GP`` and its fit do not take (nothing is touched yet)."""
    nf = optim_state["gp_noise_fun"]
    if nf[1] == 2 or nf[2] == 1:
        raise _lib.UnsupportedShape("train_gp: scaled user noise and rectified-linear output-dependent noise are not supported")
    if optim_state["uncertainty_handling_level"] == 1:
        raise _lib.UnsupportedShape("train_gp: uncertainty_handling_level 1 (noise_provided_log_multiplier) is not supported")


def train_gp(hyp_dict, optim_state, function_logger, iteration_history, options, plb_tran, pub_tran, *, device=True,
             seed=None, ctx=None):
    """Train the GP surrogate (:13-197): returns ``(gp, gp_s_N, sn2_hpd, hyp_dict)`` as the reference does, with ``gp`` this
    package's ``GP``, fitted by ``GP.fit(optimizer="fused")`` -- on the device (``device=True``) one call that scores the
    candidates, optimises, samples and leaves the posterior installed in ``ctx`` (default: the GP's context).

    ``hyp_dict`` keeps the reference's keys (``hyp``, ``warp``, ``logp``, ``full``, ``run_cov``; :56-66, :164-189).  The
    starting points are the reference's (:119-146): with ``init_N > 0`` past iteration 0, the samples of the second half of
    ``iteration_history["gp"]``, sub-sampled to ``ceil(init_N / 2)`` rows by ``np.random.choice`` on NumPy's GLOBAL stream
    where there are more than ``init_N / 2``, then ``hyp_dict["hyp"]``, made unique.  ``seed`` seeds the fit's own
    counter-based draws (None: a fresh one).  The fit's options are ``_get_gp_training_options``' ``tol_opt``, ``init_N``,
    ``opts_N``, ``n_samples``, ``thin``, ``burn`` and ``widths``, plus the design box of ``_gp_hyp``.
    ``_lib.UnsupportedShape`` (see the module text) is raised before ``hyp_dict`` or the global stream is touched."""
    _supported(optim_state, options)
    x_train, y_train, s2_train, _ = _get_training_data(function_logger)
    D = x_train.shape[1]
    mean_f = _meanfun_name_to_mean_function(optim_state["gp_mean_fun"])
    cov_f = _cov_identifier_to_covariance_function(optim_state["gp_cov_fun"])
    nf = optim_state["gp_noise_fun"]
    noise_f = _gp.GaussianNoise(constant_add=nf[0] == 1, user_provided_add=nf[1] == 1)
    if not noise_f.constant_add:
        raise _lib.UnsupportedShape("train_gp: noise without a constant term is not supported by the fused fit")
    gp = _gp.GP(D, cov_f, mean_f, noise_f)
    if ctx is not None:
        gp.ctx = ctx
    gp, hyp0, gp_s_N = _gp_hyp(optim_state, options, plb_tran, pub_tran, gp, x_train, y_train)
    trial = dict(hyp_dict)
    trial.setdefault("run_cov", None)
    gp_train = _get_gp_training_options(optim_state, iteration_history, options, trial, gp_s_N)
    if gp_train["sampler"] != "slicesample":
        raise _lib.UnsupportedShape(f"train_gp: sampler '{gp_train['sampler']}' is not supported (slicesample only)")

    # ---- from here on the call has side effects (:56-66)
    for k in ("hyp", "warp", "logp", "full", "run_cov"):
        hyp_dict.setdefault(k, None)
    if hyp_dict["hyp"] is None:
        hyp_dict["hyp"] = hyp0.copy()
    if gp_train["widths"] is not None and np.size(gp_train["widths"]) != np.size(hyp0):
        gp_train["widths"] = None  # (the model can change between iterations, :113-117)

    starts = np.empty((0, np.asarray(hyp_dict["hyp"]).T.shape[0]))
    if gp_train["init_N"] > 0 and optim_state["iter"] > 0:
        n_gp = np.size(iteration_history["gp"])
        for i in range(math.ceil((n_gp + 1) / 2) - 1, n_gp):
            starts = np.concatenate((starts, iteration_history["gp"][i].get_hyperparameters(as_array=True)))
        N0 = starts.shape[0]
        if N0 > gp_train["init_N"] / 2:
            starts = starts[np.random.choice(N0, math.ceil(gp_train["init_N"] / 2), replace=False), :]
    starts = np.unique(np.concatenate((starts, np.atleast_2d(hyp_dict["hyp"]))), axis=0)
    if starts.shape[1] != np.size(gp.hyper_priors["mu"]):
        starts = None  # (:148-150; ``fit`` then starts from the middle of the box)

    fit_opts = {k: gp_train[k] for k in ("tol_opt", "init_N", "opts_N", "n_samples", "thin", "burn", "widths")}
    fit_opts["design_lb"], fit_opts["design_ub"] = gp.temporary_data["design_box"]
    hyp_dict["hyp"], _, res = gp.fit(x_train, y_train, s2_train, hyp0=starts, options=fit_opts, device=device, seed=seed,
                                     optimizer="fused")
    if res is not None:
        hyp_dict["full"] = res["samples"]
        hyp_dict["logp"] = res["log_priors"]

    # the running average of the hyper-parameter covariance (:180-189)
    if hyp_dict["full"] is not None and hyp_dict["full"].shape[1] > 1:
        hyp_cov = np.cov(hyp_dict["full"].T)
        if hyp_dict["run_cov"] is None or options["hyp_run_weight"] == 0:
            hyp_dict["run_cov"] = hyp_cov
        else:
            w = options["hyp_run_weight"] ** options["fun_evals_per_iter"]
            hyp_dict["run_cov"] = (1 - w) * hyp_cov + w * hyp_dict["run_cov"]
    else:
        hyp_dict["run_cov"] = None
    return gp, gp_s_N, _estimate_noise(gp), hyp_dict
