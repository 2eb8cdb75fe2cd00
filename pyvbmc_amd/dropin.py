"""``pyvbmc_amd.patch(vo)`` (this module: pyvbmc_amd/dropin.py) -- the whole drop-in in one call.

Rebinds, on the reference's ``pyvbmc.vbmc.variational_optimization`` module object (or any module
with the same names):

* the four leaf names the ELBO path binds by value at import:
  ``entmc_vbmc``, ``entlb_vbmc``, ``_gp_log_joint``, ``_neg_elcbo``;
* ``_sieve`` (reference vbmc/variational_optimization.py:660-810): the reference's own function
  still runs -- candidate generation, ``np.random`` consumption, return tuple are its own -- but
  its per-candidate ``_neg_elcbo(theta, gp, vp0, 0, 0, 0, compute_var, theta_bnd)`` loop (:775-787)
  only *records* the candidates (and applies the side effects the real call has on ``vp0``); they
  are then evaluated in ONE device call (``_neg_elcbo_batch``) and the returned
  candidate arrays are sorted by the true values, as the reference sorts them (:789-792);
* ``minimize_adam`` (vbmc/minimize_adam.py:84-137): when it is handed ``optimize_vp``'s stochastic
  objective -- the closure ``vb_train_mc_fun`` over ``gp, vp0, elcbo_beta, ns_ent_K, compute_var,
  theta_bnd`` (:238-249) -- the whole loop runs on the device (``minimize_adam_elbo``, SURVEY 8f row
  2: Philox draws, iteration i uses seed + i); any other objective goes to the host loop with the
  reference's signature.

Everything falls back to the per-call path when a precondition of the batched / device-resident
form does not hold (Monte-Carlo entropy in the sieve, a variance term, candidates that differ in a
block that is not optimised, an objective that is not that closure).  A shape the kernels do not cover
at all (``_lib.UnsupportedShape``: D > 32 -- the reference's loops take any D,
entropy/entmc_vbmc.py:64-112 -- or a GP beyond the LDS plans) goes back to the REFERENCE callable
``patch`` replaced, with the reference's own arguments: the drop-in never turns a run the reference could do
into an error, and never routes anywhere but to the reference's own code.  ``unpatch(vo)`` restores the
module.  Nothing here imports the reference: ``vo`` is passed in (or imported on request).

``patch_active_sampling(mod)`` is a separate, explicit step (``patch`` does not take it): it rebinds
``active_importance_sampling`` on ``pyvbmc.vbmc.active_sample`` -- the name that module binds by value at import
(active_sample.py:15) -- to this package's mirror, with the same fallback to the reference's function for shapes the
kernels do not cover; ``unpatch_active_sampling(mod)`` puts the reference's function back.  The reference calls it
without the mirror's keyword-only extras, so under the drop-in they are chosen by the environment: ``VBMC_HIP_RNG=philox``
(the proposals drawn on the device) and ``VBMC_HIP_AIS_SAMPLER=device`` (the MCMC chains of step 2 as one launch, on the
mirror's own slice sampler and stream).  ``patch_active_sampling(mod, search=True)`` also rebinds ``_get_search_points``
(active_sample.py:647-837) to ``pyvbmc_amd.active_search.get_search_points`` -- with ``VBMC_HIP_RNG=philox`` the search
points are then drawn on the device -- again with the reference's function behind it; the reference's ``active_sample``
keeps its own evaluate / argsort lines (:334-349): only callers of ``pyvbmc_amd.search`` get the fused stage.

``patch_sieve(vo)`` is another explicit step: it replaces ``_sieve`` by ``pyvbmc_amd.sieve.sieve`` -- the candidates
drawn, scored and ranked on the device -- with the binding it finds (``make_sieve``'s wrapper after ``patch``, else the
reference's function) behind it for shapes the mirror refuses; ``patch`` and ``make_sieve`` are unchanged by it.
"""
import numpy as np

from . import _lib
from . import entropy as _entropy
from . import minimize_adam as _adam
from . import variational_optimization as _avo
from .active_importance_sampling import active_importance_sampling as _ais_mirror
from .active_search import get_search_points as _gsp_mirror
from . import whitening as _whitening

_SAVED = "_pyvbmc_amd_saved"
_LEAVES = ("entmc_vbmc", "entlb_vbmc", "_gp_log_joint", "_neg_elcbo")


_MIRROR_ONLY_KW = ("rng", "seed", "eps_half", "ctx", "rows", "return_raw", "sampler", "products", "device",
                   "n_plausible", "n_search")  # keyword-only extras of the mirrors


def _with_reference_fallback(fast, ref):
    """``fast`` with ``ref`` -- the reference callable of the same name -- behind it for shapes the device path
    does not cover.  The mirrors raise before they have touched ``vp`` (the C call fails while planning; the reference's
    in-place max-shift of theta's eta tail is idempotent), so the reference simply starts over."""

    def call(*a, **kw):
        try:
            return fast(*a, **kw)
        except _lib.UnsupportedShape:
            for k in _MIRROR_ONLY_KW:
                kw.pop(k, None)
            return ref(*a, **kw)

    call.__name__ = getattr(fast, "__name__", "call")
    call.__doc__ = getattr(fast, "__doc__", None)
    call.__wrapped__ = fast
    return call


def _apply_vp_side_effects(vp0, theta):
    """What the reference's ``_neg_elcbo`` does to the ``vp`` it is given before any arithmetic
    (:1080-1085): ``set_parameters(theta)`` and, with optimised weights, eta = theta's tail
    max-shifted (the tail of the caller's theta is shifted in place too: view arithmetic)."""
    vp0.set_parameters(theta)
    if vp0.optimize_weights:
        K = vp0.K
        tail = theta[-K:]
        tail -= np.amax(tail)
        vp0.eta = np.reshape(tail, (1, -1))


def _same_fixed_blocks(vps):
    """True when every candidate agrees with the first in the blocks that are NOT optimised (the
    batched call takes those from one ``vp``)."""
    a = vps[0]
    for b in vps[1:]:
        if not a.optimize_mu and not np.array_equal(a.mu, b.mu):
            return False
        if not a.optimize_sigma and not np.array_equal(a.sigma, b.sigma):
            return False
        if not a.optimize_lambd and not np.array_equal(a.lambd, b.lambd):
            return False
        if not a.optimize_weights and not (np.array_equal(a.w, b.w) and np.array_equal(a.eta, b.eta)):
            return False
    return True


def make_sieve(vo, ref_sieve, batch_eval=None):
    """The reference's ``_sieve`` with its candidate loop evaluated in one batched call.
    ``batch_eval(thetas, gp, vp, theta_bnd) -> F[B]`` defaults to the device call; the build
    container's check (tools/check_integration_patch.py) passes the oracle instead."""
    batch_eval = _avo._neg_elcbo_batch if batch_eval is None else batch_eval

    def _sieve(options, optim_state, vp, gp, init_N=None, best_N=1, K=None):
        rec = []          # (theta, vp0) of every deferred candidate, in call order
        state = {"bnd": None, "gp": None, "direct": False}
        real = vo._neg_elcbo

        def recorder(theta, gp_, vp0, beta=0.0, Ns=0, compute_grad=True, compute_var=None, theta_bnd=None,
                     *a, **kw):
            batchable = (Ns == 0 and not compute_grad and not compute_var and not beta and not a and not kw
                         and not state["direct"])
            if not batchable:
                state["direct"] = True  # (one form for the whole sieve: the values must be comparable)
                return real(theta, gp_, vp0, beta, Ns, compute_grad, compute_var, theta_bnd, *a, **kw)
            _apply_vp_side_effects(vp0, theta)
            rec.append((np.array(theta, dtype=np.float64), vp0))
            state["bnd"], state["gp"] = theta_bnd, gp_
            # a placeholder that keeps the reference's argsort an identity: the call index
            return float(len(rec) - 1), None, 0.0, 0.0, 0.0

        vo._neg_elcbo = recorder
        try:
            out = ref_sieve(options, optim_state, vp, gp, init_N, best_N, K)
        finally:
            vo._neg_elcbo = real
        if not rec:
            return out
        vp0_vec, vp0_type = out[0], out[1]
        vps = [v for _, v in rec]
        # the reference sorted by the placeholders: its arrays are still in candidate order
        if len(vp0_vec) != len(rec) or not all(a is b for a, b in zip(vp0_vec, vps)):
            # not the loop this wrapper was written for (another version of the caller): evaluate what it
            # returned, in the order it returned it
            F = np.array([real(v.get_parameters(), state["gp"], v, 0, 0, 0, False, state["bnd"])[0] for v in vp0_vec])
            order = np.argsort(F)
            return (vp0_vec[order], vp0_type[order]) + tuple(out[2:])
        thetas = np.stack([t for t, _ in rec])
        F = None
        if _same_fixed_blocks(vps):
            try:
                F = np.asarray(batch_eval(thetas, state["gp"], vps[0], state["bnd"]), dtype=np.float64)
            except _lib.UnsupportedShape:
                F = None  # a shape the batch kernels do not cover: one call each (which routes on to the reference)
        if F is None:  # candidates differ in a block the batched call would take from one vp: one call each
            F = np.array([real(t.copy(), state["gp"], v, 0, 0, 0, False, state["bnd"])[0] for t, v in rec])
        order = np.argsort(F)  # (:789-792)
        return (vp0_vec[order], vp0_type[order]) + tuple(out[2:])

    _sieve.__wrapped__ = ref_sieve
    return _sieve


_CLOSURE_VARS = ("gp", "vp0", "elcbo_beta", "ns_ent_K", "compute_var", "theta_bnd")


def _objective_parts(f):
    """(gp, vp0, beta, ns_ent_K, compute_var, theta_bnd) if ``f`` is ``optimize_vp``'s stochastic
    objective (:238-249: a closure named ``vb_train_mc_fun`` over exactly those names), else None."""
    code = getattr(f, "__code__", None)
    cells = getattr(f, "__closure__", None)
    if code is None or cells is None or code.co_name != "vb_train_mc_fun":
        return None
    env = dict(zip(code.co_freevars, cells))
    if not all(n in env for n in _CLOSURE_VARS):
        return None
    try:
        return tuple(env[n].cell_contents for n in _CLOSURE_VARS)
    except ValueError:  # an empty cell
        return None


def make_minimize_adam(vo, loop=None):
    """``minimize_adam`` that runs ``optimize_vp``'s stochastic objective on the device.
    ``loop(theta0, gp, vp0, ns, theta_bnd, beta, **kw)`` defaults to ``minimize_adam_elbo``."""
    loop = _adam.minimize_adam_elbo if loop is None else loop

    def minimize_adam(f, x0, lb=None, ub=None, tol_fun=0.001, max_iter=10000, master_min=0.001, master_max=0.1,
                      master_decay=200, use_early_stopping=True):
        parts = _objective_parts(f)
        # the device loop evaluates the MIRROR's objective: only when the module still routes there
        if parts is not None and getattr(vo._neg_elcbo, "__wrapped__", vo._neg_elcbo) is _avo._neg_elcbo:
            gp, vp0, beta, ns, compute_var, theta_bnd = parts
            if ns > 0 and not compute_var and (not beta or not np.isfinite(beta)):
                try:
                    return loop(np.array(x0, dtype=np.float64), gp, vp0, ns, theta_bnd, 0.0, lb, ub, tol_fun, max_iter,
                                master_min, master_max, master_decay, use_early_stopping)
                except _lib.UnsupportedShape:
                    pass  # the host loop below around f, whose _neg_elcbo routes on to the reference
        return _adam.minimize_adam(f, x0, lb, ub, tol_fun, max_iter, master_min, master_max, master_decay,
                                   use_early_stopping)

    return minimize_adam


def patch(vo=None, sieve=True, adam=True, _batch_eval=None, _loop=None):
    """Route ``vo`` (default: ``pyvbmc.vbmc.variational_optimization``) through the MI355X path.
    Idempotent; returns ``vo``.  ``sieve`` / ``adam`` switch the two caller-side rebinding steps
     off individually; the ``_``-prefixed arguments are the build-container
    check's injection points."""
    if vo is None:
        import importlib

        vo = importlib.import_module("pyvbmc.vbmc.variational_optimization")
    if hasattr(vo, _SAVED):
        unpatch(vo)
    saved = {n: getattr(vo, n) for n in _LEAVES + ("_sieve", "minimize_adam") if hasattr(vo, n)}
    setattr(vo, _SAVED, saved)
    mirrors = {"entmc_vbmc": _entropy.entmc_vbmc, "entlb_vbmc": _entropy.entlb_vbmc,
               "_gp_log_joint": _avo._gp_log_joint, "_neg_elcbo": _avo._neg_elcbo}
    for n, fast in mirrors.items():
        setattr(vo, n, _with_reference_fallback(fast, saved[n]) if callable(saved.get(n)) else fast)
    if sieve and "_sieve" in saved:
        vo._sieve = make_sieve(vo, saved["_sieve"], _batch_eval)
    if adam and "minimize_adam" in saved:
        vo.minimize_adam = make_minimize_adam(vo, _loop)
    return vo


def unpatch(vo):
    """Put back what ``patch`` replaced."""
    saved = getattr(vo, _SAVED, None)
    if saved is None:
        return vo
    for n, v in saved.items():
        setattr(vo, n, v)
    delattr(vo, _SAVED)
    _avo.clear_fast_path()  # (the repeat record holds the last call's vp, gp and context)
    return vo


_SAVED_AIS = "_pyvbmc_amd_saved_ais"
_SAVED_GSP = "_pyvbmc_amd_saved_gsp"


def patch_active_sampling(mod=None, search=False):
    """Rebind ``active_importance_sampling`` on ``mod`` (default: ``pyvbmc.vbmc.active_sample``, which binds the name by
    value, active_sample.py:15) to the device mirror, with the reference's function behind it for
    ``_lib.UnsupportedShape``; with ``search`` also ``_get_search_points`` (:647-837), in the same way.  Idempotent;
    returns ``mod``."""
    if mod is None:
        import importlib

        mod = importlib.import_module("pyvbmc.vbmc.active_sample")
    if hasattr(mod, _SAVED_AIS):
        unpatch_active_sampling(mod)
    ref = getattr(mod, "active_importance_sampling", None)
    setattr(mod, _SAVED_AIS, ref)
    fast = _ais_mirror
    mod.active_importance_sampling = _with_reference_fallback(fast, ref) if callable(ref) else fast
    if search:
        ref = getattr(mod, "_get_search_points", None)
        setattr(mod, _SAVED_GSP, ref)
        mod._get_search_points = _with_reference_fallback(_gsp_mirror, ref) if callable(ref) else _gsp_mirror
    return mod


def unpatch_active_sampling(mod):
    """Put back what ``patch_active_sampling`` replaced."""
    for saved, name in ((_SAVED_AIS, "active_importance_sampling"), (_SAVED_GSP, "_get_search_points")):
        if not hasattr(mod, saved):
            continue
        ref = getattr(mod, saved)
        if ref is None:
            delattr(mod, name)
        else:
            setattr(mod, name, ref)
        delattr(mod, saved)
    return mod


_SAVED_WARP = "_pyvbmc_amd_saved_whitening"
_WARP_NAMES = ("warp_input", "warp_gp_and_vp")


def patch_whitening(mod=None):
    """Rebind ``warp_input`` and ``warp_gp_and_vp`` on ``mod`` (default: ``pyvbmc.vbmc.vbmc``, which binds both names by
    value, vbmc.py:24) to the device mirrors of pyvbmc_amd/whitening.py, with the reference's functions behind them for
    ``_lib.UnsupportedShape`` (an unrecognised transformer, D > 32).  Opt-in: ``patch()`` does not call it.  Idempotent;
    returns ``mod``."""
    if mod is None:
        import importlib

        mod = importlib.import_module("pyvbmc.vbmc.vbmc")
    if hasattr(mod, _SAVED_WARP):
        unpatch_whitening(mod)
    saved = {n: getattr(mod, n, None) for n in _WARP_NAMES}
    setattr(mod, _SAVED_WARP, saved)
    for n in _WARP_NAMES:
        fast = getattr(_whitening, n)
        setattr(mod, n, _with_reference_fallback(fast, saved[n]) if callable(saved[n]) else fast)
    return mod


def unpatch_whitening(mod):
    """Put back what ``patch_whitening`` replaced."""
    if not hasattr(mod, _SAVED_WARP):
        return mod
    for n, ref in getattr(mod, _SAVED_WARP).items():
        if ref is None:
            delattr(mod, n)
        else:
            setattr(mod, n, ref)
    delattr(mod, _SAVED_WARP)
    return mod


_SAVED_SIEVE = "_pyvbmc_amd_saved_sieve"


def patch_sieve(vo=None):
    """Rebind ``_sieve`` on ``vo`` (default: ``pyvbmc.vbmc.variational_optimization``; ``optimize_vp`` looks the name up
    at call time, :146) to ``pyvbmc_amd.sieve.sieve``: the candidates drawn, scored and ranked on the device.  The binding
    it replaces -- ``make_sieve``'s wrapper if ``patch()`` ran before, else the reference's function -- stays behind it
    for ``_lib.UnsupportedShape`` / ``_lib.NoDeviceError``: the mirror refuses before its first draw and before it touches
    ``vp``, so the previous binding starts from untouched state.  The draws follow ``VBMC_HIP_RNG``.  Opt-in (``patch()``
    does not call it; call it after ``patch()``, which saves and restores ``_sieve`` itself) and idempotent; returns ``vo``."""
    from .sieve import sieve as _sieve_mirror

    if vo is None:
        import importlib

        vo = importlib.import_module("pyvbmc.vbmc.variational_optimization")
    if hasattr(vo, _SAVED_SIEVE):
        unpatch_sieve(vo)
    prev = getattr(vo, "_sieve", None)
    setattr(vo, _SAVED_SIEVE, prev)

    def _sieve(options, optim_state, vp, gp, init_N=None, best_N=1, K=None):
        try:
            return _sieve_mirror(options, optim_state, vp, gp, init_N, best_N, K)
        except (_lib.UnsupportedShape, _lib.NoDeviceError):
            if not callable(prev):
                raise
            return prev(options, optim_state, vp, gp, init_N, best_N, K)

    _sieve.__doc__ = _sieve_mirror.__doc__
    _sieve.__wrapped__ = _sieve_mirror
    vo._sieve = _sieve
    return vo


def unpatch_sieve(vo):
    """Put back what ``patch_sieve`` replaced."""
    if not hasattr(vo, _SAVED_SIEVE):
        return vo
    prev = getattr(vo, _SAVED_SIEVE)
    if prev is None:
        delattr(vo, "_sieve")
    else:
        vo._sieve = prev
    delattr(vo, _SAVED_SIEVE)
    return vo


_SAVED_OPTIMIZE_VP = "_pyvbmc_amd_saved_optimize_vp"


def patch_optimize_vp(vo=None):
    """Rebind ``optimize_vp`` on ``vo`` (default: ``pyvbmc.vbmc.variational_optimization``) to
    ``pyvbmc_amd.optimize_vp.optimize_vp``: the sieve, Adam, the full ELCBO and the pruning trials on the device.  The
    binding it replaces stays behind it for ``_lib.UnsupportedShape`` / ``_lib.NoDeviceError``: the mirror refuses what it
    can see (D, K, N, the optimise flags, the options, a communicator, no device) before its first draw and before it
    touches ``vp``, so the previous binding starts from untouched state.  One refusal is made later, by the sieve's
    generator (``pyvbmc_amd/optimize_vp.py``, "Refusals"): the previous binding is still called, but
    ``vp.optimize_weights`` may then already be off (warm-up).  The draws follow
    ``VBMC_HIP_RNG``.  A module that bound the name by value (``from ... import optimize_vp``) keeps what it bound: rebind
    it there as well, or pass ``pyvbmc_amd.optimize_vp`` to the caller (``active_sample(..., optimize_vp=...)``).  Opt-in
    (``patch()`` does not call it) and idempotent; returns ``vo``."""
    from .optimize_vp import optimize_vp as _mirror

    if vo is None:
        import importlib

        vo = importlib.import_module("pyvbmc.vbmc.variational_optimization")
    if hasattr(vo, _SAVED_OPTIMIZE_VP):
        unpatch_optimize_vp(vo)
    prev = getattr(vo, "optimize_vp", None)
    setattr(vo, _SAVED_OPTIMIZE_VP, prev)

    def optimize_vp(options, optim_state, vp, gp, fast_opts_N, slow_opts_N, K=None):
        try:
            return _mirror(options, optim_state, vp, gp, fast_opts_N, slow_opts_N, K)
        except (_lib.UnsupportedShape, _lib.NoDeviceError):
            if not callable(prev):
                raise
            return prev(options, optim_state, vp, gp, fast_opts_N, slow_opts_N, K)

    optimize_vp.__doc__ = _mirror.__doc__
    optimize_vp.__wrapped__ = _mirror
    vo.optimize_vp = optimize_vp
    return vo


def unpatch_optimize_vp(vo):
    """Put back what ``patch_optimize_vp`` replaced."""
    if not hasattr(vo, _SAVED_OPTIMIZE_VP):
        return vo
    prev = getattr(vo, _SAVED_OPTIMIZE_VP)
    if prev is None:
        delattr(vo, "optimize_vp")
    else:
        vo.optimize_vp = prev
    delattr(vo, _SAVED_OPTIMIZE_VP)
    return vo


_SAVED_TRAIN_GP = "_pyvbmc_amd_saved_train_gp"
_TRAIN_GP_MODULES = ("pyvbmc.vbmc.gaussian_process_train", "pyvbmc.vbmc.vbmc", "pyvbmc.vbmc.active_sample")


def patch_train_gp(mods=None, **defaults):
    """Rebind ``train_gp`` to ``pyvbmc_amd.gaussian_process_train.train_gp`` -- the hyper-parameter fit as one device call
    that leaves the posterior installed -- on every module of ``mods`` that carries the name (default: the reference's
    ``gaussian_process_train`` and the two modules that bind the name by value, ``vbmc.py`` and ``active_sample.py``).
    Each module's previous binding stays behind the mirror for ``_lib.UnsupportedShape`` / ``_lib.NoDeviceError``: the
    mirror refuses (samplers other than slice sampling, noise forms and covariance functions the package's ``GP`` does not
    take) before it touches ``hyp_dict`` or NumPy's global stream, so the previous binding starts from untouched state.
    ``defaults``: the mirror's ``device``, ``seed``, ``ctx``.  The GP it returns is this package's ``GP``, which the
    package's other mirrors and patches accept.  Opt-in (``patch()`` does not call it) and idempotent; returns the list
    of modules it rebound."""
    from .gaussian_process_train import train_gp as _mirror

    unknown = set(defaults) - {"device", "seed", "ctx"}
    if unknown:
        raise TypeError(f"patch_train_gp: unknown defaults {sorted(unknown)} (device, seed, ctx)")
    if mods is None:
        import importlib

        mods = [importlib.import_module(m) for m in _TRAIN_GP_MODULES]
    done = []
    for mod in mods:
        if hasattr(mod, _SAVED_TRAIN_GP):
            unpatch_train_gp([mod])
        prev = getattr(mod, "train_gp", None)
        if prev is None:
            continue
        setattr(mod, _SAVED_TRAIN_GP, prev)

        def train_gp(hyp_dict, optim_state, function_logger, iteration_history, options, plb_tran, pub_tran, _prev=prev):
            try:
                return _mirror(hyp_dict, optim_state, function_logger, iteration_history, options, plb_tran, pub_tran, **defaults)
            except (_lib.UnsupportedShape, _lib.NoDeviceError):
                if not callable(_prev):
                    raise
                return _prev(hyp_dict, optim_state, function_logger, iteration_history, options, plb_tran, pub_tran)

        train_gp.__doc__ = _mirror.__doc__
        train_gp.__wrapped__ = _mirror
        mod.train_gp = train_gp
        done.append(mod)
    return done


def unpatch_train_gp(mods=None):
    """Put back what ``patch_train_gp`` replaced."""
    if mods is None:
        import importlib

        mods = [importlib.import_module(m) for m in _TRAIN_GP_MODULES]
    for mod in mods:
        if hasattr(mod, _SAVED_TRAIN_GP):
            mod.train_gp = getattr(mod, _SAVED_TRAIN_GP)
            delattr(mod, _SAVED_TRAIN_GP)
    return mods


_SAVED_LOOP = "_pyvbmc_amd_saved_active_sample"
_LOOP_DEFAULTS = ("rng", "seed", "n_starts")


def patch_active_sample_loop(mod=None, **defaults):
    """Rebind ``active_sample`` on ``mod`` (default: ``pyvbmc.vbmc.vbmc``, which binds the name by value, vbmc.py:26) to
    ``pyvbmc_amd.active_sample.active_sample``, the driver of the device calls, with the reference's function behind it
    for ``_lib.UnsupportedShape`` / ``_lib.NoDeviceError``: the driver refuses before its first side effect, so the
    reference starts from untouched state.  ``timer``, ``train_gp`` and ``optimize_vp`` are the reference's own
    (``pyvbmc.timer.main_timer``, ``gaussian_process_train.train_gp``, ``variational_optimization.optimize_vp`` -- the
    last looked up at call time, so ``patch()`` applies to it), taken from ``mod`` where it carries them.  ``defaults``:
    the driver's ``rng``, ``seed``, ``n_starts``.  Opt-in (neither ``patch()`` nor ``patch_active_sampling()`` calls it)
    and idempotent; returns ``mod``."""
    from .active_sample import active_sample as _loop

    unknown = set(defaults) - set(_LOOP_DEFAULTS)
    if unknown:
        raise TypeError(f"patch_active_sample_loop: unknown defaults {sorted(unknown)} (rng, seed, n_starts)")
    if mod is None:
        import importlib

        mod = importlib.import_module("pyvbmc.vbmc.vbmc")
    if hasattr(mod, _SAVED_LOOP):
        unpatch_active_sample_loop(mod)
    ref = getattr(mod, "active_sample", None)
    setattr(mod, _SAVED_LOOP, ref)

    def _from_reference(name, module, attr):
        if getattr(mod, name, None) is not None:
            return getattr(mod, name)
        try:
            import importlib

            return getattr(importlib.import_module(module), attr)
        except ImportError:
            return None

    def active_sample(gp, sample_count, optim_state, function_logger, iteration_history, vp, options):
        kw = dict(defaults)
        kw["timer"] = _from_reference("timer", "pyvbmc.timer", "main_timer")
        kw["train_gp"] = _from_reference("train_gp", "pyvbmc.vbmc.gaussian_process_train", "train_gp")
        kw["optimize_vp"] = _from_reference("optimize_vp", "pyvbmc.vbmc.variational_optimization", "optimize_vp")
        try:
            return _loop(gp, sample_count, optim_state, function_logger, iteration_history, vp, options, **kw)
        except (_lib.UnsupportedShape, _lib.NoDeviceError):
            if not callable(ref):
                raise
            return ref(gp, sample_count, optim_state, function_logger, iteration_history, vp, options)

    active_sample.__doc__ = _loop.__doc__
    active_sample.__wrapped__ = _loop
    mod.active_sample = active_sample
    return mod


def unpatch_active_sample_loop(mod):
    """Put back what ``patch_active_sample_loop`` replaced."""
    if not hasattr(mod, _SAVED_LOOP):
        return mod
    ref = getattr(mod, _SAVED_LOOP)
    if ref is None:
        delattr(mod, "active_sample")
    else:
        mod.active_sample = ref
    delattr(mod, _SAVED_LOOP)
    return mod
