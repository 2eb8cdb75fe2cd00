"""The active-sampling loop: mirror of the reference's ``active_sample`` (``pyvbmc/vbmc/active_sample.py`` :27-644; line
numbers below cite that file) driving this package's device calls in sequence.

Per acquired point: the pre-computations (:246-303) on the host, the ranked search (``active_search.search``: one fused
device call), the local optimisation (``active_search.refine``: lockstep CMA-ES on the device), the target evaluation
through the function logger (:473-499), and the GP update -- a one-point append on the device in O(S N^2)
(``gp.append_point`` / ``gp.reupdate``: vbmc_gp_append, under per-point noise vbmc_gp_append_noisy) where the reference
calls ``gp.update(xnew, ynew)`` or ``reupdate_gp``.  With full updates (:203-242, :506-571) the GP is trained and the
posterior optimised after every point by the callables passed in (default: the reference's own).

The module adds no kernel: its hot path is the launches behind those calls.  What it decides itself is the order, the
seeds (with a Philox seed ``s`` point ``i`` searches under ``s + 2 i`` and refines under ``s + 2 i + 1``) and that a shape
the device route does not cover is refused BEFORE the first side effect (``_lib.UnsupportedShape`` /
``_lib.NoDeviceError`` with ``np.random``, the logger and ``optim_state`` untouched), so a caller can hand the same
arguments to the reference's function instead (``dropin.patch_active_sample_loop``).

The optimiser of the refinement is this package's own CMA-ES, not ``cma``: a refined run is not the reference's
trajectory.  With ``rng="numpy"`` and ``search_optimizer="none"`` the loop consumes ``np.random`` call for call as the
reference's and acquires the reference's points.
"""
import copy
import logging
import math

import numpy as np

from . import _lib
from . import active_search as _as
from . import gp as gp_mod
from . import transformer as _xf
from .acquisition import as_package_acq
from .variational_optimization import _neg_elcbo
from .variational_posterior import IdentityTransformer, _rng_mode, _seed_or_draw


def _set_option(options, key, value):
    """``options.__setitem__(key, value, force=True)`` where the options object takes ``force`` (the reference's
    ``Options``), a plain item assignment otherwise."""
    try:
        options.__setitem__(key, value, force=True)
    except TypeError:
        options[key] = value


def _options_copy(options):
    return dict(options) if isinstance(options, dict) else copy.deepcopy(options)


def _device_runs(pt, D):
    """Whether ``active_search`` accepts the transformer: the identity, or one the device runs (transformer.py)."""
    if pt is None or isinstance(pt, IdentityTransformer):
        return True
    return _xf.candidate(pt) and _xf.transformer_fields(pt, D) is not None


def _reference_callables(train_gp, optimize_vp, need_train, need_vp):
    """The full update's callables: the ones passed in, else the reference's, imported on first need.  (The default stays
    the reference's ``train_gp``; the package's own -- one device call per fit that leaves the posterior installed -- is
    ``pyvbmc_amd.gaussian_process_train.train_gp``: pass it as ``active_sample(..., train_gp=...)``, or bind it under the
    drop-in with ``pyvbmc_amd.patch_train_gp()``.)"""
    if need_train and train_gp is None:
        try:
            from pyvbmc.vbmc.gaussian_process_train import train_gp
        except ImportError as e:
            raise ImportError("active_sample: full updates with active_sample_gp_update need train_gp: pass it, or install "
                              "PyVBMC (pyvbmc.vbmc.gaussian_process_train.train_gp)") from e
    if need_vp and optimize_vp is None:
        try:
            from pyvbmc.vbmc.variational_optimization import optimize_vp
        except ImportError as e:
            raise ImportError("active_sample: full updates with active_sample_vp_update need optimize_vp: pass it, or install "
                              "PyVBMC (pyvbmc.vbmc.variational_optimization.optimize_vp)") from e
    return train_gp, optimize_vp


def _initial_design(sample_count, optim_state, function_logger, options, logger):
    """:82-168 -- no GP yet: the provided points, topped up from the plausible box."""
    parameter_transformer = function_logger.parameter_transformer
    x0 = optim_state["cache"]["x_orig"]
    provided_sample_count, D = x0.shape
    if provided_sample_count <= sample_count:
        Xs = np.copy(x0)
        ys = np.copy(optim_state["cache"]["y_orig"])
        if provided_sample_count < sample_count:
            pub_tran = optim_state.get("pub_tran")
            plb_tran = optim_state.get("plb_tran")
            if options.get("init_design") == "plausible":
                # uniform random samples in the plausible box (in transformed space)
                random_Xs = np.random.rand(sample_count - provided_sample_count, D) * (pub_tran - plb_tran) + plb_tran
            elif options.get("init_design") == "narrow":
                start_Xs = parameter_transformer(Xs[0])
                random_Xs = (np.random.rand(sample_count - provided_sample_count, D) - 0.5) * 0.1 * (pub_tran - plb_tran) + start_Xs
                random_Xs = np.minimum((np.maximum(random_Xs, plb_tran)), pub_tran)
            else:
                raise ValueError("Unknown initial design for VBMC. "
                                 "The option 'init_design' must be 'plausible' or "
                                 "'narrow' but was {}.".format(options.get("init_design")))
            random_Xs = parameter_transformer.inverse(random_Xs)  # back to original space
            Xs = np.append(Xs, random_Xs, axis=0)
            ys = np.append(ys, np.full(sample_count - provided_sample_count, np.nan), axis=0)
        idx_remove = np.full(provided_sample_count, True)
    else:
        Xs = np.copy(x0[:sample_count])
        ys = np.copy(optim_state["cache"]["y_orig"][:sample_count])
        idx_remove = np.full(provided_sample_count, True)
        logger.info("More than sample_count=%s initial points have been provided, using only the first %s points.",
                    sample_count, sample_count)
    # remove points from the starting cache
    optim_state["cache"]["x_orig"] = np.delete(optim_state["cache"]["x_orig"], np.where(idx_remove), 0)
    optim_state["cache"]["y_orig"] = np.delete(optim_state["cache"]["y_orig"], np.where(idx_remove), 0)
    Xs = parameter_transformer(Xs)
    for idx in range(sample_count):
        if np.isnan(ys[idx]):  # function value is not available
            function_logger(Xs[idx])
        else:
            function_logger.add(Xs[idx], ys[idx])


def _precompute(gp, optim_state, function_logger):
    """:265-303 -- the noise at every training point (mean over the samples), the GP's length scale (geometric mean) and
    the training inputs in units of it."""
    posts = gp.posteriors
    Ns_gp = np.size(posts)
    D = gp.D
    cov = getattr(gp, "covariance", None)
    cov_N = cov.hyperparameter_count(D) if cov is not None and hasattr(cov, "hyperparameter_count") else D + 1
    noise = getattr(gp, "noise", None)
    noise_N = noise.hyperparameter_count() if noise is not None and hasattr(noise, "hyperparameter_count") else 1
    if hasattr(function_logger, "S"):
        s2 = (function_logger.S[function_logger.X_flag] ** 2) * function_logger.n_evals[function_logger.X_flag]
    else:
        s2 = None
    sn2new = np.zeros((gp.X.shape[0], Ns_gp))
    for s in range(Ns_gp):
        hyp_noise = np.ravel(posts[s].hyp)[cov_N : cov_N + noise_N]
        if noise is not None and hasattr(noise, "compute"):
            sn2new[:, s] = np.reshape(noise.compute(hyp_noise, gp.X, gp.y, s2), -1)
        else:  # a stand-in without a noise function: the rule of gp._noise_var
            sn2new[:, s] = np.exp(2 * hyp_noise[0]) + (0.0 if s2 is None else np.reshape(s2, -1))
    gp.temporary_data["sn2_new"] = sn2new.mean(1)
    ln_ell = np.zeros((D, Ns_gp))
    for s in range(Ns_gp):
        ln_ell[:, s] = np.ravel(posts[s].hyp)[:D]
    optim_state["gp_length_scale"] = np.exp(ln_ell.mean(1))
    gp.temporary_data["X_rescaled"] = gp.X / optim_state["gp_length_scale"]


def _check_support(gp, function_logger, vp, options, device, injected):
    """Obligation of the drop-in: every reason to refuse, found before anything is drawn, logged or written.  Returns
    the acquisition objects of ``options["search_acq_fcn"]`` as this package's."""
    D = int(gp.D)
    if D > 32:
        raise _lib.UnsupportedShape(f"active_sample: D={D} > 32 not supported")
    acqs = [as_package_acq(a) for a in options["search_acq_fcn"]]
    optimizer = options["search_optimizer"]
    if optimizer not in ("none", "cmaes") and not (D == 1 and optimizer == "Nelder-Mead"):
        raise _lib.UnsupportedShape(f"active_sample: search_optimizer {optimizer!r} (none, cmaes and, for D = 1, Nelder-Mead)")
    if not injected:
        if not (_device_runs(function_logger.parameter_transformer, D) and _device_runs(vp.parameter_transformer, D)):
            raise _lib.UnsupportedShape("active_sample: the parameter transformer is not one the device runs "
                                        "(pyvbmc_amd/transformer.py)")
        if not device or _lib.device_count() <= 0:
            raise _lib.NoDeviceError(_lib.E_NODEV, "active_sample needs a gfx950 device (pyvbmc_amd has no CPU fallback)")
    return acqs


def active_sample(gp, sample_count, optim_state, function_logger, iteration_history, vp, options, *, rng=None, seed=None,
                  device=True, n_starts=1, fetch=None, ctx=None, timer=None, train_gp=None, optimize_vp=None, trace=None,
                  _search=None, _refine=None):
    """Acquire ``sample_count`` points one after the other: the reference's ``active_sample`` with its arguments and its
    return tuple ``(function_logger, optim_state, vp, gp)``.

    Accepted are the reference's own objects (``FunctionLogger``, ``Options``, ``VariationalPosterior``, a gpyreg-shaped
    GP), this package's classes and plain ducks; ``options`` is anything with ``.get`` and ``[]``.  An entry of
    ``options["search_acq_fcn"]`` is a constructor string, one of this package's acquisition classes or the reference's
    object of the same class name (``acquisition.as_package_acq``).

    ``gp is None``: the initial design (:82-168), host code with the reference's statements and draws.

    Keyword-only:
      rng, seed   "numpy": every draw is the reference's statement on NumPy's global stream, in its order -- with
                  ``search_optimizer="none"`` the acquired points are the reference's after the same ``np.random.seed``.
                  "philox": the search set is drawn on the device; point i searches under ``seed + 2 i`` and refines under
                  ``seed + 2 i + 1`` (``seed=None``: one fresh seed).  ``np.random.randint`` for the choice among several
                  acquisition functions is drawn in both modes.  Default as everywhere in the package (``VBMC_HIP_RNG``).
      device      False: only with injected ``_search`` / ``_refine``; the GP updates then run on the host.
      n_starts    handed to ``refine``: CMA-ES runs side by side from the best ranked rows.
      fetch       whether the GP updates inside the loop copy the factor ``L`` back.  None (default): they do not --
                  nothing on the host reads it there -- and the GP is fetched once on return (``fetch_posteriors``).
                  False: as None, but a GP of this package's class is returned with ``L = None`` records.
      timer       the reference's ``main_timer`` (anything with ``start_timer`` / ``stop_timer``); None: no timing.
      train_gp, optimize_vp   the full update's callables; default the reference's, imported when first needed
                  (``ImportError`` when PyVBMC is absent).
      trace       ``trace(i, res, ref, gp, vp, optim_state)`` after the refinement of point i, before the target
                  evaluation; a read-only hook.
      _search, _refine   test hooks with the signatures and return fields of ``active_search.search`` / ``refine``.

    Raises ``_lib.UnsupportedShape`` (D > 32, a transformer the device does not run, an unknown acquisition class, a
    ``search_optimizer`` other than none / cmaes / Nelder-Mead at D = 1) or ``_lib.NoDeviceError`` before the first
    ``np.random`` draw, logger call or change of ``optim_state``."""
    logger = logging.getLogger("ActiveSample")
    logger.setLevel(logging.INFO)
    if options.get("display") == "off":
        logger.setLevel(logging.WARN)
    elif options.get("display") == "iter":
        logger.setLevel(logging.INFO)
    elif options.get("display") == "full":
        logger.setLevel(logging.DEBUG)

    if gp is None:
        _initial_design(sample_count, optim_state, function_logger, options, logger)
        return function_logger, optim_state, vp, gp

    # ---- support, decided before the first side effect
    injected = _search is not None
    acqs = _check_support(gp, function_logger, vp, options, device, injected)
    mode = _rng_mode(rng)
    search_fn = _as.search if _search is None else _search
    refine_fn = _as.refine if _refine is None else _refine
    if device:
        from ._duck import ctx_of

        ctx = ctx_of(vp, ctx) if (not injected or _lib.device_count() > 0) else None
        if not injected and ctx.device < 0:
            raise _lib.NoDeviceError(_lib.E_NODEV, "active_sample needs a gfx950 device (pyvbmc_amd has no CPU fallback)")
    else:
        ctx = None
    on_device = bool(device) and ctx is not None and ctx.device >= 0
    loop_fetch = bool(fetch)

    # :203-214
    active_sample_full_update = (options["active_sample_vp_update"] or options["active_sample_gp_update"]) and (
        (optim_state["iter"] - options["active_sample_full_update_past_warmup"] <= optim_state["last_warmup"])
        or iteration_history["r_index"][-1] > options["active_sample_full_update_threshold"])
    full = bool(active_sample_full_update) and sample_count > 1
    if full:
        train_gp, optimize_vp = _reference_callables(train_gp, optimize_vp, bool(options["active_sample_gp_update"]),
                                                     bool(options["active_sample_vp_update"]))
    if mode == "philox":
        seed = _seed_or_draw(seed)

    if full:  # :216-242: temporarily changed options for the local updates, on a copy
        recompute_var_post_old = optim_state["recompute_var_post"]
        entropy_alpha_old = optim_state["entropy_alpha"]
        options_update = _options_copy(options)
        _set_option(options_update, "gp_tol_opt", options["gp_tol_opt_active"])
        _set_option(options_update, "gp_tol_opt_mcmc", options["gp_tol_opt_mcmc_active"])
        _set_option(options_update, "tol_weight", 0)
        _set_option(options_update, "ns_ent", options["ns_ent_active"])
        _set_option(options_update, "ns_ent_fast", options["ns_ent_fast_active"])
        _set_option(options_update, "ns_ent_fine", options["ns_ent_fine_active"])
        hyp_dict = None
        vp0 = copy.deepcopy(vp)

    def start(name):
        if timer is not None:
            timer.start_timer(name)

    def stop(name):
        if timer is not None:
            timer.stop_timer(name)

    idx_acq = 0
    for i in range(sample_count):
        optim_state["N"] = function_logger.Xn + 1  # :246-251
        optim_state["N_eff"] = sum(function_logger.n_evals[function_logger.X_flag])
        if not options["acq_hedge"]:  # :260-263: drawn whatever the mode, so NumPy's stream stays aligned
            idx_acq = np.random.randint(len(acqs))
        _precompute(gp, optim_state, function_logger)  # :265-303
        acq_eval = acqs[idx_acq]

        # :310-349 the ranked search, :355-423 the local optimisation
        kw = {"rng": mode, "ctx": ctx}
        if mode == "philox":
            kw["seed"] = (seed + 2 * i) % 2**64
        res = search_fn(acq_eval, gp, vp, function_logger, optim_state, options, **kw)
        if options["search_optimizer"] != "none" and gp.D == 1:  # :357-361
            _set_option(options, "search_optimizer", "Nelder-Mead")
        ref = refine_fn(res, acq_eval, gp, vp, function_logger, optim_state, options, n_starts=n_starts,
                        seed=(seed + 2 * i + 1) % 2**64 if mode == "philox" else None, device=on_device, ctx=ctx)
        if trace is not None:
            trace(i, res, ref, gp, vp, optim_state)

        # :473-499 the target
        xnew = np.array(ref.X_acq, dtype=np.float64).reshape(1, -1)
        idx = ref.idx_cache_acq
        if np.isnan(idx):
            y_orig = np.nan
        else:
            idx = int(idx)
            y_orig = optim_state["cache"]["y_orig"][idx]
        start("fun_time")
        if np.isnan(y_orig):  # function value is not available, evaluate
            ynew, _, idx_new = function_logger(xnew)
        else:
            ynew, _, idx_new = function_logger.add(xnew, y_orig)
            optim_state["cache"]["x_orig"] = np.delete(optim_state["cache"]["x_orig"], idx, 0)
            optim_state["cache"]["y_orig"] = np.delete(optim_state["cache"]["y_orig"], idx, 0)
        stop("fun_time")
        s2new = function_logger.S[idx_new] ** 2 if hasattr(function_logger, "S") else None

        if i + 1 < sample_count:  # :503-588 (no update after the last point)
            if active_sample_full_update:
                if hyp_dict is None:
                    hyp_dict = optim_state["hyp_dict"]
                start("gp_train")
                if options["active_sample_gp_update"]:
                    gp, __, optim_state["sn2_hpd"], optim_state["hyp_dict"] = train_gp(
                        hyp_dict, optim_state, function_logger, iteration_history, options_update, optim_state["plb_tran"],
                        optim_state["pub_tran"])
                    stop("gp_train")
                else:
                    gp = gp_mod.reupdate(function_logger, gp, ctx=ctx, device=on_device, fetch=loop_fetch)
                if options["active_sample_vp_update"]:  # quick variational optimisation
                    start("variational_fit")
                    N_fastopts = math.ceil(options_update["ns_elbo_incr"] * options_update["ns_elbo"](vp.K))
                    if options["update_random_alpha"]:
                        optim_state["entropy_alpha"] = 1 - np.sqrt(np.random.rand())
                    vp, _, _ = optimize_vp(options_update, optim_state, vp, gp, N_fastopts, slow_opts_N=1)
                    if optim_state.get("vp_repo") is not None:
                        np.append(optim_state["vp_repo"], vp.get_parameters())  # (as there: the result is dropped)
                    else:
                        optim_state["vp_repo"] = [vp.get_parameters()]
                    stop("variational_fit")
            else:
                # only the posterior follows, at the present hyper-parameter samples: a one-point append where there is
                # no observation noise and the point is new, else the logger's data again (the noisy append inside)
                start("gp_train")
                update1 = (s2new is None and function_logger.n_evals[idx_new] == 1) and not options["noise_shaping"]
                if update1:
                    gp = gp_mod.append_point(gp, xnew, ynew, ctx=ctx, device=on_device, fetch=loop_fetch)
                else:
                    gp = gp_mod.reupdate(function_logger, gp, ctx=ctx, device=on_device, fetch=loop_fetch)
                stop("gp_train")

        # :590-605 search bounds that the new point comes close to are moved out
        delta_search = 0.05 * (optim_state["ub_search"] - optim_state["lb_search"])
        idx = np.abs(xnew - optim_state["lb_search"]) < delta_search
        optim_state["lb_search"][idx] = np.maximum(optim_state["lb_tran"][idx], optim_state["lb_search"][idx] - delta_search[idx])
        idx = np.abs(xnew - optim_state["ub_search"]) < delta_search
        optim_state["ub_search"][idx] = np.minimum(optim_state["ub_tran"][idx], optim_state["ub_search"][idx] + delta_search[idx])

    if full:  # :620-642
        optim_state["recompute_var_post"] = recompute_var_post_old
        optim_state["entropy_alpha"] = entropy_alpha_old
        optim_state["hyp_dict"] = hyp_dict
        # if the variational posterior has changed, the old one is kept when it is the better of the two
        theta0 = vp0.get_parameters()
        theta = vp.get_parameters()
        if (np.size(theta0) != np.size(theta)) or np.any(theta0 != theta):
            NSentFineK = math.ceil(options["ns_ent_fine_active"](vp0.K) / vp0.K)
            elbo0 = -_neg_elcbo(theta0, gp, vp0, 0.0, NSentFineK, False, True)[0]
            if elbo0 > vp.stats["elbo"]:
                vp = vp0

    if not (fetch is False and isinstance(gp, gp_mod.GP)) and any(p.L is None for p in gp.posteriors):
        gp_mod.fetch_posteriors(gp, ctx)
    return function_logger, optim_state, vp, gp


__all__ = ["active_sample"]
