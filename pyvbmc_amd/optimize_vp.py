"""``optimize_vp`` (reference ``pyvbmc/vbmc/variational_optimization.py:90-391``): the sieve, the stochastic optimiser, the
full ELCBO and the pruning trials, joined, with every stage on the device.  Line numbers below cite
``variational_optimization.py``.

The stages and what runs them:

sieve (:146-154)            ``pyvbmc_amd.sieve.sieve``: candidates drawn, scored, ranked in two device calls.
optimiser (:181-295)        Adam with the reference's step arithmetic (:255-269): ``adam="device"`` (default) is
                            ``minimize_adam_elbo``, the whole loop on the device with Philox draws; ``adam="host"`` is the
                            package's ``minimize_adam`` around ``_neg_elcbo`` with the call's ``rng``.  With ``ns_ent_K == 0``
                            (K = 1 or ``entropy_switch``) SciPy's ``minimize`` around ``_neg_elcbo(Ns=0)`` (:202-235).
full ELCBO (:428-499)       ``vbmc_elcbo_full``: theta -> mixture, the GP sums and variance, the value-only entropy and the
                            statistics over the GP samples as one call with one wait.  It leaves a RECORD of ``I_sk`` /
                            ``J_sjk`` on the device (include/vbmc_hip.h).
selection (:307-320)        by ``nelcbo``, on the host.  Only the winner's record needs to be resident when pruning starts:
                            unless it is the evaluation made last it is re-installed from the arrays already downloaded
                            (``vbmc_elcbo_put``); nothing is evaluated again.
pruning (:322-378)          ``vbmc_elcbo_prune_trial`` / ``_accept``: removing a component leaves ``mu``, ``sigma``, ``lambd`` of
                            the others unchanged and rescales their weights, so a trial's ``G``, ``varG``, ``var_ss`` are a
                            re-weighting of the record (csrc/elcbo_full.hip) and only the Monte-Carlo entropy is new --
                            no GP kernel is launched.  ``ns_ent_fine_K`` is recomputed at K' as ``_eval_full_elcbo`` does.

Draw modes (``rng`` keyword, else ``VBMC_HIP_RNG``, else "numpy"):

``rng="numpy"``   the sieve's draws, the candidate of every trial (``np.random.randint``) and the entropy draws of every full
                  evaluation and trial come from NumPy's global stream in the reference's order; from Adam's ``theta_opt``
                  onwards the stream's state after the call is the reference's for the same accepted and rejected sequence.
                  (``adam="device"`` draws from Philox inside the loop, so the whole call is then not stream-identical.)
``rng="philox"``  the trial candidates come from ``np.random.default_rng(seed)``, every other draw from the device, under
                  seeds derived from ``seed`` (``seed=None``: one draw of NumPy's global stream).

``vp.stats`` has the reference's keys (:380-389).  ``stats["I_sk"]`` is the winning evaluation's columns with the pruned
ones deleted.  ``stats["J_sjk"]`` has the reference's shape after pruning, ``(S, K0, K')``: the reference deletes along
axis 2 only (:376), and so does this function.  The square block of the final posterior is ``J_sjk[:, alive, :]`` with
``alive`` the surviving columns -- ``np.delete`` along axis 1 of the indices that were pruned, in the order they were.

``device=False`` is the same function over the composed calls (``_neg_elcbo`` with ``compute_var`` and ``separate_K``,
``entmc_vbmc``) with the re-weighting in NumPy (``reweight``), following ``sieve.py``'s convention: the kernels still run on
the device, this package has no host ELBO.

Refusals: everything the sieve refuses (``sieve.check_supported``: D <= 32, K <= 128, ...) and a context with a
communicator raise ``_lib.UnsupportedShape`` (no device: ``_lib.NoDeviceError``) before the first draw and before
``vp.optimize_weights`` or ``vp.bounds`` change; ``dropin.patch_optimize_vp`` then goes back to the binding it replaced.
A training set beyond the GP sums' LDS plan (2 D + N + 5 doubles over 150 KiB: N above about 19 000) is refused with the
others.  NOT covered by that promise: a refusal only the sieve's generator can make (``rng="philox"`` with more
high-density points than its LDS holds, about 3 700 at K D = 4 096) is raised inside the sieve, after the warm-up switch.  An unknown ``stochastic_optimizer`` raises the
reference's ``ValueError`` (:295).
"""
import copy
import ctypes as C
import math

import numpy as np
import scipy as sp
import scipy.optimize  # noqa: F401

from . import _lib
from . import sieve as _sieve_mod
from . import variational_optimization as _avo
from ._duck import ctx_of, optimize_mask, upload_vp
from .entropy import _even_ns, entmc_vbmc, entlb_vbmc, upload_reference_eps
from .gp import upload_gp
from .minimize_adam import minimize_adam, minimize_adam_elbo
from .variational_posterior import _rng_mode, _seed_or_draw

_opt = _sieve_mod._opt
TINY = np.spacing(1)
_SEED_MASK = 0x3FFFFFFFFFFFFFFF
_GLJ_LDS_MAX = 150 * 1024  # bytes of dynamic LDS a block of the GP sums may take (csrc/prep.hip)


def reweight(I_sk, J_sjk, alive, w):
    """``(G, varG, var_ss)`` of the posterior whose components are the columns ``alive`` of a recorded ``I_sk`` (S, K0) /
    ``J_sjk`` (S, K0, K0) with weights ``w``: ``_gp_log_joint``'s tail (:1505-1596) in NumPy, upper triangle, both clamps
    at ``np.spacing(1)``.  ``J_sjk`` None (``skip_elbo_variance``): the variances are 0."""
    alive = np.asarray(alive, dtype=np.int64)
    w = np.asarray(w, dtype=np.float64).ravel()
    I = np.asarray(I_sk)[:, alive]
    S = I.shape[0]
    G = I @ w
    if J_sjk is None:
        return (np.sum(G) / S if S > 1 else G[0]), 0.0, 0.0
    J = np.asarray(J_sjk)[:, alive][:, :, alive]
    ww = np.triu(2.0 * np.outer(w, w), 1)
    d = np.arange(alive.size)
    varG = np.sum(J * ww, axis=(1, 2)) + np.sum(w**2 * np.maximum(TINY, J[:, d, d]), axis=1)
    varG = np.maximum(varG, TINY)
    if S == 1:
        return G[0], varG[0], 0.0
    G_bar = np.sum(G) / S
    varG_ss = np.sum((G - G_bar) ** 2) / (S - 1)
    return G_bar, np.sum(varG) / S + varG_ss, varG_ss + np.std(varG, ddof=1)


def _initialize_full_elcbo(max_idx, D, K, Ns):
    """:394-425."""
    s = {k: np.full((max_idx,), np.nan) for k in ("G", "H", "varF", "varG", "varH", "var_ss")}
    s["nelbo"] = np.full((max_idx,), np.inf)
    s["nelcbo"] = np.full((max_idx,), np.inf)
    s["theta"] = np.full((max_idx, D), np.nan)
    s["I_sk"] = np.full((max_idx, Ns, K), np.nan)
    s["J_sjk"] = np.full((max_idx, Ns, K, K), np.nan)
    return s


def _skip_variance(options):
    return bool("skip_elbo_variance" in options and options["skip_elbo_variance"])


def _dup(vp):
    """``copy.deepcopy(vp)`` that stays on ``vp``'s device context (the package's posterior does not copy it)."""
    v = copy.deepcopy(vp)
    if getattr(vp, "_ctx", None) is not None:
        v._ctx = vp._ctx
    return v


def _prune_vp(vp, idx):
    """The posterior without component ``idx`` as the pruning loop forms it (:328-340) and ``_neg_elcbo`` leaves it
    (``set_parameters``, then eta = the max-shifted tail, :1080-1085)."""
    v = _dup(vp)
    v.w = np.delete(v.w, idx)
    v.eta = np.delete(v.eta, idx)
    v.sigma = np.delete(v.sigma, idx)
    v.mu = np.delete(v.mu, idx, axis=1)
    v.K -= 1
    theta = v.get_parameters()
    v.set_parameters(theta)
    if v.optimize_weights:
        tail = theta[-v.K:]
        tail -= np.amax(tail)
        v.eta = np.reshape(tail, (1, -1)).copy()
    return v, theta


class _Seeds:
    """The seeds of one call's device draws: ``base`` for the sieve, then one per stage and use."""

    def __init__(self, base):
        self.base, self.n = base, 0

    def adam(self, i):
        return None if self.base is None else (self.base + ((i + 1) << 24)) & _SEED_MASK

    def next(self):
        self.n += 1
        return 0 if self.base is None else (self.base + (1 << 44) + self.n) & _SEED_MASK


class _Stage:
    """The full evaluations and trials of one call, on one of the two routes."""

    def __init__(self, ctx, gp, options, mode, seeds, device):
        self.ctx, self.gp, self.options, self.mode, self.seeds, self.device = ctx, gp, options, mode, seeds, device
        self.compute_var = not _skip_variance(options)
        self.resident = None  # the slot whose record the device holds
        self.rec = None       # device=False: (I_sk, J_sjk) of the winner

    def ns(self, K):
        return math.ceil(_opt(self.options, "ns_ent_fine", K) / K)

    def _draws(self, K, D, ns):
        """(eps mode, seed) of an entropy of ``ns`` samples per component, the reference's draws made resident first."""
        if ns <= 0:
            return _lib.EPS_PHILOX, 0
        if self.mode == "numpy":
            upload_reference_eps(self.ctx, K, D, ns)
            return _lib.EPS_RESIDENT, 0
        return _lib.EPS_PHILOX, self.seeds.next()

    def full(self, slot, theta, vp0):
        """One ``_eval_full_elcbo`` (:465-485): the 11 outputs' seven scalars, I_sk, J_sjk; ``theta``'s tail is shifted."""
        ctx, D, K = self.ctx, vp0.D, vp0.K
        S = len(self.gp.posteriors)
        ns = _even_ns(self.ns(K))
        if not self.device:
            seed = self.seeds.next() if self.mode == "philox" else None
            r = _avo._neg_elcbo(theta, self.gp, vp0, 0, ns, False, self.compute_var, None, 0.0, True, rng=self.mode, seed=seed,
                                ctx=ctx)
            out = np.array([float(np.ravel(v)[0]) for v in (r[0], r[2], r[3], r[4], r[7], r[8], r[6])])  # (S = 1: varG is (1,))
            return out, r[9], r[10]
        # theta overwrites every optimised block: the attributes only need to be on the device when some block is NOT
        # optimised or the context holds another (D, K) -- as in _neg_elcbo's fused path
        mask = optimize_mask(vp0)
        if mask != 15 or getattr(ctx, "D", None) != D or getattr(ctx, "K", None) != K:
            upload_vp(vp0, ctx)
        upload_gp(self.gp, ctx)
        eps_mode, seed = self._draws(K, D, ns)
        out = np.empty(7)
        I = np.empty((S, K))
        J = np.empty((S, K, K)) if self.compute_var else None
        assert theta.dtype == np.float64 and theta.flags["C_CONTIGUOUS"]
        try:
            ctx.check(ctx._lib.vbmc_elcbo_full(ctx._h, _lib.ptr(theta), theta.size, mask, ns, eps_mode,
                                               C.c_uint64(seed), int(self.compute_var), _lib.ptr(out), _lib.ptr(I), _lib.ptr(J)))
        finally:
            ctx.mixture_changed(D, K)
        self.resident = slot
        return out, I, J

    def install(self, slot, vp, I, J):
        """The winner's record for the trials."""
        if not self.device:
            self.rec = (I, J)
            return
        if self.resident == slot:
            return
        ctx = self.ctx
        upload_vp(vp, ctx)
        S, K = I.shape
        ctx.check(ctx._lib.vbmc_elcbo_put(ctx._h, S, K, _lib.ptr(_lib.f64(I)), _lib.ptr(None if J is None else _lib.f64(J))))
        self.resident = slot

    def trial(self, vp_pruned, alive, pos):
        """The evaluation of a pruning trial (:342-352): the seven scalars.  On the device route the pruned mixture exists
        twice: the library forms its own from the record's (csrc/api_elcbo_full.hip ``prune_mixture``) and THAT one is what
        the trial's entropy and weights are evaluated on; ``vp_pruned`` (``_prune_vp``, the reference's NumPy statements) is
        what the caller keeps -- the weights the next candidates are chosen by and the posterior that is returned.  The two
        are the same statements in C++ and NumPy and agree to the rounding of ``log`` / ``exp``."""
        ctx, D, K = self.ctx, vp_pruned.D, vp_pruned.K
        ns = _even_ns(self.ns(K))
        if not self.device:
            if ns > 0:
                seed = self.seeds.next() if self.mode == "philox" else None
                H, _ = entmc_vbmc(vp_pruned, ns, (False,) * 4, 1, rng=self.mode, seed=seed, ctx=ctx)
            else:
                H, _ = entlb_vbmc(vp_pruned, (False,) * 4, 1, ctx=ctx)
            G, varG, var_ss = reweight(self.rec[0], self.rec[1], alive, vp_pruned.w)
            return np.array([-G - H, G, H, varG, varG, 0.0, var_ss])
        eps_mode, seed = self._draws(K, D, ns)
        out = np.empty(7)
        try:
            ctx.check(ctx._lib.vbmc_elcbo_prune_trial(ctx._h, int(pos), ns, eps_mode, C.c_uint64(seed), _lib.ptr(out)))
        finally:
            ctx.mixture_changed(D, K)
        return out

    def accept(self):
        if self.device:
            self.ctx.check(self.ctx._lib.vbmc_elcbo_prune_accept(self.ctx._h))

    def record_info(self):
        """``vbmc_elcbo_record_info``: S, K0, K_alive, the alive list, GP launches and stream waits since the record was made."""
        info = (C.c_int64 * 5)()
        alive = np.zeros(_sieve_mod.MAX_K, dtype=np.int32)
        self.ctx.check(self.ctx._lib.vbmc_elcbo_record_info(self.ctx._h, info, alive.ctypes.data_as(C.POINTER(C.c_int32))))
        return {"S": int(info[0]), "K0": int(info[1]), "K_alive": int(info[2]), "alive": alive[: int(info[2])].copy(),
                "gp_launches": int(info[3]), "waits": int(info[4])}


def _adam_steps(options, optim_state, vp):
    """The reference's step arithmetic (:255-269)."""
    master_min = min(options["sgd_step_size"], 0.001)
    if optim_state["warmup"] or not vp.optimize_weights:
        scaling_factor = min(0.1, options["sgd_step_size"] * 10)
    else:
        scaling_factor = min(0.1, options["sgd_step_size"])
    master_max = max(master_min, scaling_factor)
    return master_min, master_max, 200, int(min(10000, options["max_iter_stochastic"]))


def optimize_one(options, optim_state, vp, gp, vp0, ns_ent_K, theta_bnd, elbo_stats, i, stage, *, adam="device", adam_seed=None,
                 theta_opt=None, theta_mid=None, slots=None):
    """One slow start (:200-303) from ``vp0``: the optimiser, then the full evaluations of the midpoint (slot ``2 i``, with
    ``elcbo_midpoint``) and of the endpoint (slot ``2 i + 1``) into ``elbo_stats``.  ``theta_opt`` / ``theta_mid`` given (tests:
    the reference's recorded iterates): the optimiser is skipped."""
    ctx, mode = stage.ctx, stage.mode
    i_mid, i_end = 2 * i, 2 * i + 1
    theta0 = vp0.get_parameters()
    if theta_opt is None:
        if ns_ent_K == 0:
            def vb_train_fun(theta_):
                res = _avo._neg_elcbo(theta_, gp, vp0, 0, 0, compute_grad=True, compute_var=0, theta_bnd=theta_bnd, ctx=ctx)
                return res[0], res[1]

            res = sp.optimize.minimize(vb_train_fun, theta0, jac=True, tol=options["det_entropy_tol_opt"])
            if not res.success:
                raise RuntimeError("Cannot optimize variational parameters with", "scipy.optimize.minimize.")
            theta_opt = res.x
        else:
            master_min, master_max, master_decay, max_iter = _adam_steps(options, optim_state, vp)
            kw = dict(tol_fun=options["tol_fun_stochastic"], max_iter=max_iter, master_min=master_min, master_max=master_max,
                      master_decay=master_decay)
            if adam == "device":
                theta_opt, _, theta_lst, f_val_lst, _ = minimize_adam_elbo(theta0, gp, vp0, ns_ent_K, theta_bnd, rng="philox",
                                                                            seed=adam_seed, ctx=ctx, **kw)
            else:
                def vb_train_mc_fun(theta_):
                    res = _avo._neg_elcbo(theta_, gp, vp0, 0, ns_ent_K, compute_grad=True, compute_var=0, theta_bnd=theta_bnd,
                                          rng=mode, ctx=ctx)
                    return res[0], res[1]

                theta_opt, _, theta_lst, f_val_lst, _ = minimize_adam(vb_train_mc_fun, theta0, **kw)
            if options["elcbo_midpoint"]:
                theta_mid = theta_lst[:, np.argmin(f_val_lst)]
    evals = []
    if ns_ent_K != 0 and options["elcbo_midpoint"] and theta_mid is not None:
        evals.append((i_mid, theta_mid))
    evals.append((i_end, theta_opt))
    for slot, theta in evals:
        theta = np.array(theta, dtype=np.float64)
        out, I, J = stage.full(slot, theta, vp0)
        K = vp0.K
        if stage.device:
            # _neg_elcbo's side effects on vp0 (:1080-1085), which the reference's final posterior inherits: eta stays
            # that of the start's LAST evaluation, whichever slot wins (set_parameters does not touch it)
            vp0.set_parameters(theta)
            if vp0.optimize_weights:
                vp0.eta = theta[-K:].reshape(1, -1).copy()
        for k, v in zip(("nelbo", "G", "H", "varF", "varG", "varH", "var_ss"), out):
            elbo_stats[k][slot] = v
        elbo_stats["nelcbo"][slot] = out[0]  # (:486 with beta = 0)
        elbo_stats["theta"][slot, : theta.size] = theta
        elbo_stats["I_sk"][slot, :, :K] = I
        if J is not None:
            elbo_stats["J_sjk"][slot, :, :K, :K] = J
        if slots is not None:
            slots[slot] = vp0
    return elbo_stats


def finish(options, vp0_by_slot, elbo_stats, K, stage, *, choose=None, on_trial=None):
    """Selection (:307-320), the pruning loop (:322-378) and the stats (:380-389).  ``choose(n)``: the trial candidate's
    position among the ``n`` below the threshold (default by the draw mode: module docstring).  ``on_trial(info)`` (tests):
    called after every trial with its candidate set, index, delta, threshold and decision."""
    if choose is None:
        choose = _chooser(stage.mode, stage.seeds.base)
    idx = int(np.argmin(elbo_stats["nelcbo"]))
    elbo = -elbo_stats["nelbo"][idx]
    elbo_sd = np.sqrt(elbo_stats["varF"][idx])
    G, H = elbo_stats["G"][idx], elbo_stats["H"][idx]
    var_ss, varG, varH = elbo_stats["var_ss"][idx], elbo_stats["varG"][idx], elbo_stats["varH"][idx]
    I_sk = elbo_stats["I_sk"][idx].copy()
    J_sjk = elbo_stats["J_sjk"][idx].copy()
    vp = _dup(vp0_by_slot[idx])
    vp.set_parameters(elbo_stats["theta"][idx, :])
    pruned = 0
    if vp.optimize_weights:
        already_checked = np.full((vp.K,), False)
        alive = list(range(vp.K))
        installed = False
        while np.any((vp.w < options["tol_weight"]) & ~already_checked):
            if not installed:
                stage.install(idx, vp, I_sk, None if not stage.compute_var else J_sjk)
                installed = True
            cand = np.argwhere((vp.w < options["tol_weight"]).ravel() & ~already_checked).ravel()
            r = choose(np.size(cand))
            i_c = int(cand[r])
            vp_pruned, _ = _prune_vp(vp, i_c)
            alive_pruned = alive[:i_c] + alive[i_c + 1 :]
            out = stage.trial(vp_pruned, alive_pruned, i_c)
            elbo_pruned, elbo_pruned_sd = -out[0], np.sqrt(out[3])
            w_imp = options["elcbo_impro_weight"]
            delta_elcbo = np.abs((elbo_pruned - w_imp * elbo_pruned_sd) - (elbo - w_imp * elbo_sd))
            pruning_threshold = options["tol_improvement"] * _opt(options, "pruning_threshold_multiplier", K)
            accept = bool(delta_elcbo < pruning_threshold)
            if on_trial is not None:
                on_trial({"cand": cand, "r": r, "idx": i_c, "delta": float(delta_elcbo), "threshold": float(pruning_threshold),
                          "accept": accept, "out": out})
            if accept:
                stage.accept()
                vp, alive = vp_pruned, alive_pruned
                elbo, elbo_sd = elbo_pruned, elbo_pruned_sd
                G, H, var_ss, varG, varH = out[1], out[2], out[6], out[4], out[5]
                pruned += 1
                already_checked = np.delete(already_checked, i_c)
                I_sk = np.delete(I_sk, i_c, axis=1)
                J_sjk = np.delete(J_sjk, i_c, axis=2)
            else:
                already_checked[i_c] = True
    vp.stats = {"elbo": elbo, "elbo_sd": elbo_sd, "e_log_joint": G, "e_log_joint_sd": np.sqrt(varG), "entropy": H,
                "entropy_sd": np.sqrt(varH), "stable": False, "I_sk": I_sk, "J_sjk": J_sjk}
    return vp, var_ss, pruned


def _chooser(mode, seed):
    if mode == "numpy":
        return lambda n: int(np.random.randint(0, n))
    gen = np.random.default_rng(seed)
    return lambda n: int(gen.integers(0, n))


def optimize_vp(options, optim_state, vp, gp, fast_opts_N, slow_opts_N, K=None, *, rng=None, seed=None, device=True,
                adam="device", ctx=None):
    """The reference's ``optimize_vp`` (:90-391) with its arguments and its return value ``(vp, var_ss, pruned)``: the
    optimised posterior (a new object; ``vp.stats`` as there), the variance of the ELBO due to the GP hyper-parameter
    samples, the number of pruned components.  Module docstring: the stages, the draw modes, ``stats["J_sjk"]``'s shape
    ``(S, K0, K')`` after pruning, ``device=False``, the refusals."""
    if K is None:
        K = vp.K
    # ---- everything that can refuse, before the first draw and before vp changes
    mode = _rng_mode(rng)
    if adam not in ("device", "host"):
        raise ValueError(f"unknown adam {adam!r} (device, host)")
    ns_ent_K = math.ceil(_opt(options, "ns_ent", K) / K)
    ns_ent_K_fast = math.ceil(_opt(options, "ns_ent_fast", K) / K)
    if optim_state["entropy_switch"] or K == 1:
        ns_ent_K = ns_ent_K_fast = 0
    if ns_ent_K > 0 and options["stochastic_optimizer"] != "adam":
        raise ValueError("Unknown stochastic optimizer!")
    _sieve_mod.check_supported(vp, K, ns_ent_K_fast, 0)
    N = int(np.shape(gp.X)[0])
    if 8 * (2 * int(vp.D) + N + 5) > _GLJ_LDS_MAX:  # (csrc/prep.hip launch_prep_on, csrc/glj_block.h glj_own)
        raise _lib.UnsupportedShape(f"optimize_vp: N={N} too large for the GP sums' LDS plan")
    ctx = ctx_of(vp, ctx)
    _sieve_mod._need_device(ctx)
    if ctx.world != 1:
        raise _lib.UnsupportedShape("optimize_vp: not covered with a communicator")

    if optim_state["warmup"]:  # (:142-143)
        vp.optimize_weights = False
    base = _seed_or_draw(seed) if mode == "philox" else seed
    seeds = _Seeds(base)
    vp0_vec, vp0_type, elcbo_beta, compute_var, ns_ent_K, _ = _sieve_mod.sieve(
        options, optim_state, vp, gp, fast_opts_N, slow_opts_N, K, rng=mode, seed=base, device=device, ctx=ctx)
    vp0_vec, vp0_type = np.atleast_1d(vp0_vec), np.atleast_1d(vp0_type)
    theta_bnd = vp.get_bounds(gp.X, options, K)

    theta_N = np.size(vp0_vec[0].get_parameters())
    Ns = len(gp.posteriors)
    elbo_stats = _initialize_full_elcbo(slow_opts_N * 2, theta_N, K, Ns)
    stage = _Stage(ctx, gp, options, mode, seeds, device)
    slots = {}
    for i in range(0, slow_opts_N):
        if slow_opts_N == 1:  # (:187-199)
            idx = 0
        elif slow_opts_N == 2:
            idx = np.where(vp0_type == 1)[0][0] if i == 0 else np.where((vp0_type == 2) | (vp0_type == 3))[0][0]
        else:
            idx = np.where(vp0_type == (i % 3) + 1)[0][0]
        vp0 = vp0_vec[idx]
        vp0_vec = np.delete(vp0_vec, idx)
        vp0_type = np.delete(vp0_type, idx)
        optimize_one(options, optim_state, vp, gp, vp0, ns_ent_K, theta_bnd, elbo_stats, i, stage, adam=adam,
                     adam_seed=seeds.adam(i), slots=slots)
    return finish(options, slots, elbo_stats, K, stage, choose=_chooser(mode, base))
