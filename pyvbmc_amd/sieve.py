"""The sieve that opens every ``optimize_vp`` (reference ``pyvbmc/vbmc/variational_optimization.py``): ``_sieve``
(:660-810), ``_vb_init`` (:813-988) and ``get_hpd`` (``stats/get_hpd.py``), with the candidates drawn, scored and ranked
on the device.  Line numbers below cite ``variational_optimization.py``.

The host keeps what is small and happens once per call -- ``get_hpd``, ``vp.get_bounds``, the option arithmetic, type 2's
ordering of ``y_star`` and its single ``sigma0`` draw, the ``std(X_star)`` form of ``lambd`` -- and, with ``rng="numpy"``,
the draws themselves.  Everything that is done once per candidate is one launch with a workgroup per candidate
(``vbmc_sieve_fill``, csrc/sieve.hip) that writes the raw theta rows where the batch evaluator's launches read them;
``vbmc_sieve_eval`` scores and ranks them and hands everything back in one copy.

Draw modes, chosen like everywhere in this package (``rng`` keyword, else ``VBMC_HIP_RNG``, else "numpy"):

``rng="numpy"``
    Every draw is the reference's statement on NumPy's global stream, in the reference's order; the stream's state after
    the call is the reference's.  Consecutive ``np.random.randn`` calls continue one sequence, so where no other kind of
    draw sits between them (type 1 with ``K_new == K``, type 2) the jitter of all candidates of a type is one vectorised
    draw; where ``randint`` / ``rand`` (spawned components) or ``permutation`` (type 3) interleave, a short loop makes the
    reference's calls in its order and does nothing else.  The draws go up as one (B, n_slot) matrix and one (B, K_new)
    index matrix (slot layout: csrc/sieve.hip).

``rng="philox"``
    Every draw that scales with the number of candidates is made on the device: counter (seed, candidate, slot) through
    the sampler's 53-bit draws.  Type 3 takes the ``min(K_new, N_star)`` training points of smallest Philox key, ties by
    index; a spawned component's parent is ``floor(u K)``.  Type 2's ``sigma0`` draw, one per call, comes from
    ``np.random.default_rng(seed)``.  ``seed=None`` takes one draw of NumPy's global stream (``_seed_or_draw``).

``device=False`` generates the candidates on the host (the same algorithm in NumPy, ``_assemble_host``; Philox restated
in NumPy for ``rng="philox"``) and brings them to the device with ``vbmc_sieve_put``; they are still SCORED on the device
(``vbmc_sieve_eval``): this package has no host ``_neg_elcbo``.  ``vb_init(device=False)`` alone touches no GPU.

What the route covers: D <= 32, K_new <= 128, ``optimize_sigma`` on (``optimize_mu``, ``optimize_lambd``,
``optimize_weights`` in any combination: every block that is not optimised is then the same for all candidates of all
three types, :969-985, and the whole sieve is one batch), ``K_new >= vp.K`` (``K_new > vp.K`` only with ``optimize_mu``),
``ns_ent_K_fast == 0`` and ``elcbo_beta == 0``.  Anything else raises ``_lib.UnsupportedShape`` (no device:
``_lib.NoDeviceError``) before the first ``np.random`` draw and before any attribute of ``vp`` changes;
``dropin.patch_sieve`` then goes back to the binding it replaced.
"""
import copy
import ctypes as C
import math

import numpy as np

from . import _lib
from . import variational_optimization as _avo
from ._duck import ctx_of
from .gp import upload_gp
from .variational_posterior import _rng_mode, _seed_or_draw

MAX_D, MAX_K = 32, 128
_STREAM_NORMAL, _STREAM_UNIFORM, _STREAM_KEY = 10, 11, 12  # counter word 3 (csrc/sieve.hip)


def get_hpd(X, y, hpd_frac=0.8):
    """High-posterior-density subset of the training set (reference stats/get_hpd.py:30-45): the ``round(hpd_frac * N)``
    points of largest ``y``, in descending order (the reversed ``argsort``), their range per dimension (NaN when the
    set is empty) and their indices."""
    N, D = X.shape
    order = np.argsort(y, axis=None)[::-1]
    hpd_N = round(hpd_frac * N)
    indices = order[0:hpd_N]
    hpd_X = X[indices]
    hpd_y = y[indices]
    if hpd_N > 0:
        hpd_range = np.max(hpd_X, axis=0) - np.min(hpd_X, axis=0)
    else:
        hpd_range = np.full((D), np.nan)
    return hpd_X, hpd_y, hpd_range, indices


class _Shape:
    """The sizes, the optimise flags and the slot layout of one call (csrc/sieve.hip)."""

    def __init__(self, vp, K_new, N_star):
        self.D, self.K, self.Kn, self.Ns = int(vp.D), int(vp.K), int(K_new), int(N_star)
        self.o_mu, self.o_sg = bool(vp.optimize_mu), bool(vp.optimize_sigma)
        self.o_lm, self.o_w = bool(vp.optimize_lambd), bool(vp.optimize_weights)
        self.mask = self.o_mu | (self.o_sg << 1) | (self.o_lm << 2) | (self.o_w << 3)
        D, K, Kn = self.D, self.K, self.Kn
        self.n_sp = Kn - K
        self.s_s3 = self.n_sp * (D + 1)
        self.s_mu = self.s_s3 + Kn
        self.s_sg = self.s_mu + D * Kn
        self.s_lm = self.s_sg + Kn
        self.s_w = self.s_lm + D
        self.s_u = self.s_w + Kn
        self.n_slot = self.s_u + self.n_sp
        self.m = min(Kn, self.Ns)
        # the jitter's slots in the order the reference draws them (:956-967), the blocks that are optimised only
        cols = []
        if self.o_mu:
            cols.append(np.arange(self.s_mu, self.s_sg))
        cols.append(np.arange(self.s_sg, self.s_lm))
        if self.o_lm:
            cols.append(np.arange(self.s_lm, self.s_w))
        if self.o_w:
            cols.append(np.arange(self.s_w, self.s_u))
        self.jcols = np.concatenate(cols)
        self.p_sg = D * Kn if self.o_mu else 0
        self.p_lm = self.p_sg + Kn
        self.n_theta = self.p_lm + (D if self.o_lm else 0) + (Kn if self.o_w else 0)


def check_supported(vp, K_new, ns_ent_K_fast=0, elcbo_beta=0):
    """Raise ``_lib.UnsupportedShape`` unless the device route covers this call (module docstring).  Reads ``vp`` only."""
    D, K = int(vp.D), int(vp.K)
    if D > MAX_D or K_new > MAX_K:
        raise _lib.UnsupportedShape(f"sieve: D={D}, K_new={K_new} beyond D <= {MAX_D}, K_new <= {MAX_K}")
    if not vp.optimize_sigma:
        raise _lib.UnsupportedShape("sieve: optimize_sigma off is not covered")
    if K_new < K:
        raise _lib.UnsupportedShape(f"sieve: K_new={K_new} < K={K} is not covered")
    if K_new > K and not vp.optimize_mu:
        raise _lib.UnsupportedShape("sieve: K_new > K needs optimize_mu")
    if ns_ent_K_fast != 0:
        raise _lib.UnsupportedShape("sieve: Monte-Carlo entropy in the sieve (ns_ent_fast > 0) is not covered")
    if elcbo_beta != 0:
        raise _lib.UnsupportedShape("sieve: elcbo_beta != 0 is not covered")


def _need_device(ctx):
    if getattr(ctx, "device", 0) < 0:
        raise _lib.NoDeviceError(_lib.E_NODEV, "sieve: host-only context (this route needs a gfx950 device)")


# ---- the per-call constants (host) -------------------------------------------------------------------------------------

def _constants(vp, sh, X_star, y_star, counts, z2):
    """What ``_vb_init`` computes once per call.  ``z2``: type 2's ``randn(1, K_new)`` (:873-875), or None."""
    D, K, Kn = sh.D, sh.K, sh.Kn
    c = {"lambd0": np.array(vp.lambd, dtype=np.float64).reshape(D, 1), "mu0": np.array(vp.mu, dtype=np.float64).reshape(D, K),
         "w0": np.array(vp.w, dtype=np.float64).reshape(1, K), "sigma0": np.array(vp.sigma, dtype=np.float64).reshape(1, K)}
    N_star = X_star.shape[0]
    if counts[1] > 0:
        mu2 = c["mu0"]
        if sh.o_mu:  # (:863-868)
            order = np.argsort(y_star, axis=None)[::-1]
            idx_order = np.tile(range(0, min(Kn, N_star)), (math.ceil(Kn / N_star),))
            mu2 = X_star[order[idx_order[0:Kn]], :].T
        V = np.var(mu2, axis=1, ddof=1) if K > 1 else np.var(X_star, axis=0, ddof=1)
        c["mu2"] = mu2
        c["sigma2"] = np.sqrt(np.mean(V / c["lambd0"] ** 2) / Kn) * np.exp(0.2 * z2)
    if (counts[1] > 0 or counts[2] > 0) and sh.o_lm:  # (:920-921, :946-947)
        lambd_s = np.reshape(np.std(X_star, axis=0, ddof=1), (-1, 1))
        lambd_s *= np.sqrt(D / np.sum(lambd_s**2))
        c["lambd_s"] = lambd_s
    c["v3"] = float(np.mean(np.var(X_star, axis=0, ddof=1))) if (counts[2] > 0 and K == 1) else 0.0
    return c


# ---- the draws -----------------------------------------------------------------------------------------------------------

def _draws_numpy(sh, counts):
    """(Z, I, z2): the reference's draws on NumPy's global stream, in the reference's order, laid out by slot."""
    D, K, Kn = sh.D, sh.K, sh.Kn
    n1, n2, n3 = counts
    B = n1 + n2 + n3
    Z = np.zeros((B, sh.n_slot))
    I = np.zeros((B, Kn), dtype=np.int32)
    nj = sh.jcols.size
    z2 = None
    if n1 > 0:
        if sh.n_sp == 0:
            if n1 > 1:
                Z[1:n1, sh.jcols] = np.random.randn((n1 - 1) * nj).reshape(n1 - 1, nj)
        else:
            for i in range(n1):
                for j in range(sh.n_sp):  # (:900-914)
                    I[i, j] = np.random.randint(0, K)
                    Z[i, j * (D + 1) : j * (D + 1) + D + 1] = np.random.randn(D + 1)
                    if sh.o_w:
                        Z[i, sh.s_u + j] = np.random.rand()
                if i > 0:
                    Z[i, sh.jcols] = np.random.randn(nj)
    if n2 > 0:
        z2 = np.random.randn(1, Kn)
        if n2 > 1:
            Z[n1 + 1 : n1 + n2, sh.jcols] = np.random.randn((n2 - 1) * nj).reshape(n2 - 1, nj)
    cols3 = np.concatenate((np.arange(sh.s_s3, sh.s_mu), sh.jcols))
    for b in range(n1 + n2, B):
        if sh.o_mu:
            I[b, : sh.m] = np.random.permutation(sh.Ns)[: sh.m]
        Z[b, cols3] = np.random.randn(cols3.size)
    return Z, I, z2


_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_LO = np.uint64(0xFFFFFFFF)


def _philox(c0, c1, c2, c3, seed):
    """Philox4x32-10 (Salmon et al., SC'11) over uint32 arrays, key = the 64-bit seed: csrc/philox.h in NumPy."""
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    c = [np.asarray(x, dtype=np.uint32).astype(np.uint64) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def _u53(hi, lo):
    return ((hi << np.uint64(32)) | lo) >> np.uint64(11)


def _draws_philox_host(sh, counts, seed):
    """(Z, I) of ``rng="philox"`` on the host: what the device draws under the same seed (csrc/sieve.hip)."""
    n1, n2, n3 = counts
    B = n1 + n2 + n3
    b = np.arange(B, dtype=np.uint64)[:, None]
    lo, hi = (b & _LO), (b >> np.uint64(32))
    n_pair = (sh.s_u + 1) // 2
    x = _philox(lo, hi, np.arange(n_pair)[None, :], _STREAM_NORMAL, seed)
    u1 = (_u53(x[0], x[1]) + np.uint64(1)).astype(np.float64) * 2.0**-53
    u2 = _u53(x[2], x[3]).astype(np.float64) * 2.0**-53
    rad = np.sqrt(-2.0 * np.log(u1))
    Zn = np.stack((rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)), axis=2).reshape(B, 2 * n_pair)
    Z = np.zeros((B, sh.n_slot))
    Z[:, : sh.s_u] = Zn[:, : sh.s_u]
    I = np.zeros((B, sh.Kn), dtype=np.int32)
    if sh.n_sp > 0 and n1 > 0:
        x = _philox(lo[:n1], hi[:n1], np.arange(2 * sh.n_sp)[None, :], _STREAM_UNIFORM, seed)
        u = _u53(x[0], x[1]).astype(np.float64) * 2.0**-53
        I[:n1, : sh.n_sp] = np.floor(u[:, 0::2] * sh.K).astype(np.int32)
        Z[:n1, sh.s_u :] = u[:, 1::2]
    if n3 > 0 and sh.o_mu:
        x = _philox(lo[n1 + n2 :], hi[n1 + n2 :], np.arange(sh.Ns)[None, :], _STREAM_KEY, seed)
        I[n1 + n2 :, : sh.m] = np.argsort(_u53(x[0], x[1]), axis=1, kind="stable")[:, : sh.m]
    return Z, I


# ---- the candidates from the draws, in NumPy (device=False) ------------------------------------------------------------------

def _assemble_host(sh, counts, c, Z, I):
    """The thetas of all candidates from the draws: csrc/sieve.hip's arithmetic, vectorised over the candidates."""
    D, K, Kn = sh.D, sh.K, sh.Kn
    n1, n2, n3 = counts
    B = n1 + n2 + n3
    mu = np.empty((B, D, Kn))
    sg = np.empty((B, Kn))
    lm = np.empty((B, D))
    w = np.full((B, Kn), 1.0 / Kn)
    lam0 = c["lambd0"][:, 0]
    lam23 = c["lambd_s"][:, 0] if sh.o_lm and "lambd_s" in c else lam0
    t1, t2, t3 = slice(0, n1), slice(n1, n1 + n2), slice(n1 + n2, B)
    if n1 > 0:
        mu[t1, :, :K], sg[t1, :K], lm[t1] = c["mu0"], c["sigma0"][0], lam0
        if sh.o_w:
            w[t1, :K] = c["w0"][0]
        rows = np.arange(n1)
        for j in range(sh.n_sp):
            p = I[t1, j]
            zs = Z[t1, j * (D + 1) : j * (D + 1) + D + 1]
            mu[t1, :, K + j] = c["mu0"][:, p].T + 0.5 * c["sigma0"][0, p][:, None] * lam0[None, :] * zs[:, :D]
            sg[t1, K + j] = c["sigma0"][0, p] * np.exp(0.2 * zs[:, D])
            if sh.o_w:
                xi = 0.25 + 0.25 * Z[t1, sh.s_u + j]
                w[t1, K + j] = xi * w[rows, p]
                w[rows, p] *= 1.0 - xi
    if n2 > 0:
        mu[t2], sg[t2], lm[t2] = c["mu2"], c["sigma2"][0], lam23
    if n3 > 0:
        if sh.o_mu:
            sel = I[t3][:, np.arange(Kn) % sh.m]
            mu[t3] = np.transpose(c["X_star"][sel], (0, 2, 1))
        else:
            mu[t3] = c["mu0"]
        v3 = np.mean(np.var(mu[t3], axis=2, ddof=1), axis=1) if K > 1 else np.full(n3, c["v3"])
        sg[t3] = np.sqrt(v3 / Kn)[:, None] * np.exp(0.2 * Z[t3, sh.s_s3 : sh.s_mu])
        lm[t3] = lam23
    jit = np.ones(B, dtype=bool)
    if n1 > 0:
        jit[0] = False
    if n2 > 0:
        jit[n1] = False
    if sh.o_mu:
        zm = Z[:, sh.s_mu : sh.s_sg].reshape(B, D, Kn)
        mu[jit] += (sg[:, None, :] * lm[:, :, None] * zm)[jit]
    sg[jit] *= np.exp(0.2 * Z[jit, sh.s_sg : sh.s_lm])
    if sh.o_lm:
        lm[jit] *= np.exp(0.2 * Z[jit, sh.s_lm : sh.s_w])
    if sh.o_w:
        w[jit] *= np.exp(0.2 * Z[jit, sh.s_w : sh.s_u])
    nl = np.sqrt(np.sum(lm**2, axis=1) / D)[:, None]
    th = np.empty((B, sh.n_theta))
    if sh.o_mu:
        th[:, : D * Kn] = np.transpose(mu, (0, 2, 1)).reshape(B, D * Kn)
    th[:, sh.p_sg : sh.p_sg + Kn] = np.log(sg * nl)
    if sh.o_lm:
        th[:, sh.p_lm : sh.p_lm + D] = np.log(lm / nl)
    if sh.o_w:
        eta = np.log(w / np.sum(w, axis=1, keepdims=True))
        th[:, sh.n_theta - Kn :] = eta - np.max(eta, axis=1, keepdims=True)
    return th


# ---- the candidates --------------------------------------------------------------------------------------------------------

class Candidates:
    """The candidates of one ``vb_init`` / ``sieve`` call.

    ``thetas`` (B, n_theta): the raw parameters the reference's ``get_parameters`` returns for a candidate -- ``lambd``
    renormalised so that ``sum(lambd**2) == D``, ``sigma`` scaled by the same factor, ``w`` normalised -- with the weight
    tail max-shifted as ``_neg_elcbo`` leaves it (:1082-1085).  ``types`` (B,).  ``fixed``: the values of the blocks that
    are not optimised, one set for all rows (``mu`` (D, K), ``lambd`` (D, 1), ``w`` (1, K); ``eta`` (1, K) without optimised
    weights).  ``F``, ``G``, ``H``: the scores in row order once the candidates have been scored (``sieve``), else None.
    """

    def __init__(self, vp, sh, thetas, types, fixed):
        self.vp, self._sh, self.thetas, self.types, self.fixed = vp, sh, thetas, types, fixed
        self.K = sh.Kn
        self.F = self.G = self.H = None

    def __len__(self):
        return self.thetas.shape[0]

    def to_vps(self):
        """The reference's object array of posteriors (:969-988 followed by ``set_parameters`` and the eta assignment of
        ``_neg_elcbo``, :1080-1085): each a shallow copy of ``vp`` with its own ``mu``, ``sigma``, ``lambd``, ``w``,
        ``eta``, ``K = K_new``, ``bounds = None``, ``stats = None``.  The ``parameter_transformer`` is SHARED with ``vp``,
        not deep-copied as the reference does: nothing downstream of the sieve (``optimize_vp``, ``_neg_elcbo``,
        ``update_K``, the pruning loop) mutates it, and copying it was most of the reference's cost per candidate."""
        sh, th = self._sh, self.thetas
        D, Kn, B = sh.D, sh.Kn, th.shape[0]
        sigma = np.exp(th[:, sh.p_sg : sh.p_sg + Kn])
        lambd = np.exp(th[:, sh.p_lm : sh.p_lm + D]) if sh.o_lm else np.tile(self.fixed["lambd"][:, 0], (B, 1))
        nl = np.sqrt(np.sum(lambd**2, axis=1) / D)[:, None]
        lambd, sigma = lambd / nl, sigma * nl
        if sh.o_w:
            eta = th[:, sh.n_theta - Kn :]
            w = np.exp(eta)
            w = w / np.sum(w, axis=1, keepdims=True)
        out = np.empty(B, dtype=object)
        for b in range(B):
            v = copy.copy(self.vp)
            v.K = Kn
            v.mu = np.reshape(th[b, : D * Kn], (D, Kn), order="F").copy() if sh.o_mu else self.fixed["mu"].copy()
            v.sigma = sigma[b].reshape(1, -1).copy()
            v.lambd = lambd[b].reshape(-1, 1).copy()
            v.w = w[b].reshape(1, -1).copy() if sh.o_w else self.fixed["w"].copy()
            v.eta = eta[b].reshape(1, -1).copy() if sh.o_w else self.fixed["eta"].copy()
            v.bounds = None
            v.stats = None
            if hasattr(v, "_mode"):
                v._mode = None
            out[b] = v
        return out


def _fixed_blocks(sh, c):
    Kn = sh.Kn
    fixed = {}
    if not sh.o_mu:
        fixed["mu"] = c["mu0"].copy()
    if not sh.o_lm:
        fixed["lambd"] = c["lambd0"] / np.sqrt(np.sum(c["lambd0"] ** 2) / sh.D)
    if not sh.o_w:
        fixed["w"] = np.ones((1, Kn)) / Kn
        fixed["eta"] = np.ones((1, Kn)) / Kn
    return fixed


def _fill_device(ctx, sh, counts, c, Z, I, seed):
    """``vbmc_sieve_fill``: the resident set from the constants and the draws (``Z`` None: Philox under ``seed``)."""
    a = _lib.SieveFillArgs()
    a.D, a.K, a.K_new, a.optimize_mask = sh.D, sh.K, sh.Kn, sh.mask
    a.n1, a.n2, a.n3 = counts
    keep = [_lib.f64(c["mu0"].T), _lib.f64(c["sigma0"].ravel()), _lib.f64(c["lambd0"].ravel()), _lib.f64(c["w0"].ravel())]
    a.mu0_KxD, a.sigma0_K, a.lambd0_D, a.w0_K = (_lib.ptr(k) for k in keep)
    if counts[1] > 0:
        keep += [_lib.f64(c["mu2"].T), _lib.f64(c["sigma2"].ravel())]
        a.mu2_KnxD, a.sigma2_Kn = _lib.ptr(keep[-2]), _lib.ptr(keep[-1])
    if "lambd_s" in c:
        keep.append(_lib.f64(c["lambd_s"].ravel()))
        a.lambd_s_D = _lib.ptr(keep[-1])
    keep.append(_lib.f64(c["X_star"]))
    a.N_star, a.X_star_NxD, a.v3 = sh.Ns, _lib.ptr(keep[-1]), c["v3"]
    if Z is not None:
        keep += [_lib.f64(Z), np.ascontiguousarray(I, dtype=np.int32)]
        a.Z_BxS, a.n_slot = _lib.ptr(keep[-2]), sh.n_slot
        a.I_BxKn = keep[-1].ctypes.data_as(C.POINTER(C.c_int32))
    a.seed = int(seed or 0)
    return a, keep


def _generate(vp, counts, K_new, X_star, y_star, rng, seed, device, ctx, want_thetas=True):
    """The candidates of ``counts`` = (type 1, type 2, type 3), in that order.  With ``device`` the set is resident
    afterwards (and downloaded only if ``want_thetas``)."""
    check_supported(vp, K_new)
    mode = _rng_mode(rng)
    if device:
        ctx = ctx_of(vp, ctx)
        _need_device(ctx)
    X_star = np.ascontiguousarray(X_star, dtype=np.float64)
    sh = _Shape(vp, K_new, X_star.shape[0])
    counts = tuple(int(max(0, n)) for n in counts)
    B = sum(counts)
    if sh.Ns < 1 and (counts[1] > 0 or counts[2] > 0):
        raise _lib.UnsupportedShape("sieve: an empty X_star")
    Z = I = z2 = None
    if mode == "numpy":
        Z, I, z2 = _draws_numpy(sh, counts)
    else:
        seed = _seed_or_draw(seed)
        if counts[1] > 0:
            z2 = np.random.default_rng(seed).standard_normal((1, sh.Kn))
        if not device:
            Z, I = _draws_philox_host(sh, counts, seed)
    c = _constants(vp, sh, X_star, y_star, counts, z2)
    c["X_star"] = X_star
    types = np.concatenate([t * np.ones(n) for t, n in zip((1, 2, 3), counts)])
    thetas = None
    if device:
        a, keep = _fill_device(ctx, sh, counts, c, Z, I, seed)
        thetas = np.empty((B, sh.n_theta)) if want_thetas else None
        ctx.check(ctx._lib.vbmc_sieve_fill(ctx._h, C.byref(a), _lib.ptr(thetas)))
    else:
        thetas = _assemble_host(sh, counts, c, Z, I)
    return Candidates(vp, sh, thetas, types, _fixed_blocks(sh, c))


def vb_init(vp, vb_type, opts_N, K_new, X_star, y_star, *, rng=None, seed=None, device=True, ctx=None):
    """``opts_N`` starting points of type ``vb_type`` (1: the old parameters, 2: the best training points, 3: random
    training points) for a posterior of ``K_new`` components: the reference's ``_vb_init`` (:813-988), returned as
    ``Candidates`` (``to_vps()`` gives the reference's object array, ``types`` its second value)."""
    if vb_type not in (1, 2, 3):
        raise ValueError("Unknown type for initialization of variational posteriors.")
    counts = [0, 0, 0]
    counts[vb_type - 1] = opts_N
    return _generate(vp, counts, K_new, X_star, y_star, rng, seed, device, ctx)


def _opt(options, name, K):
    if hasattr(options, "eval"):
        return options.eval(name, {"K": K})
    v = options[name]
    return v(K) if callable(v) else v


def _template_mixture(ctx, cand):
    """The context's mixture for the scoring: D, K_new and the blocks that are not optimised (the others are read from
    the theta rows)."""
    sh, fx = cand._sh, cand.fixed
    D, Kn = sh.D, sh.Kn
    ctx.set_mixture(fx.get("mu", np.zeros((D, Kn))), np.ones(Kn), fx.get("lambd", np.ones((D, 1))),
                    fx.get("w", np.ones((1, Kn)) / Kn), fx.get("eta", np.zeros((1, Kn))))
    ctx.__dict__["_vp_args"] = None  # (upload_vp's record of what it sent last no longer describes the device)
    _avo.clear_fast_path()


def score(cand, gp, theta_bnd, *, ctx=None, put=False):
    """Score and rank the resident set (``put``: ``cand.thetas`` first becomes it): ``vbmc_sieve_eval``.  Fills
    ``cand.F / G / H`` (row order) and returns ``(order, thetas in rank order)``; ``cand.thetas`` is replaced by the
    downloaded rows put back in row order."""
    ctx = ctx_of(cand.vp, ctx)
    sh = cand._sh
    B = len(cand.types)
    if put:
        th = _lib.f64(cand.thetas)
        ctx.check(ctx._lib.vbmc_sieve_put(ctx._h, B, sh.n_theta, _lib.ptr(th)))
    _template_mixture(ctx, cand)
    upload_gp(gp, ctx)
    opts = _lib.ElboOpts()
    opts.ns_per_comp, opts.compute_grad, opts.optimize_mask = 0, 0, sh.mask
    keep = []
    if theta_bnd is not None:
        lb, ub = _lib.f64(theta_bnd["lb"].ravel()), _lib.f64(theta_bnd["ub"].ravel())
        keep += [lb, ub]
        opts.bnd_lb, opts.bnd_ub, opts.n_bnd = _lib.ptr(lb), _lib.ptr(ub), lb.size
        opts.tol_con = float(theta_bnd["tol_con"])
        opts.weight_threshold = float(theta_bnd.get("weight_threshold", 0.0))
        opts.weight_penalty = float(theta_bnd.get("weight_penalty", 0.0))
    F, G, H = np.empty(B), np.empty(B), np.empty(B)
    order = np.empty(B, dtype=np.int64)
    ranked = np.empty((B, sh.n_theta))
    ctx.check(ctx._lib.vbmc_sieve_eval(ctx._h, C.byref(opts), _lib.ptr(F), _lib.ptr(G), _lib.ptr(H),
                                       order.ctypes.data_as(C.POINTER(C.c_int64)), _lib.ptr(ranked)))
    cand.F, cand.G, cand.H = F, G, H
    th = np.empty_like(ranked)
    th[order] = ranked
    cand.thetas = th
    return order, ranked


def sieve(options, optim_state, vp, gp, init_N=None, best_N=1, K=None, *, rng=None, seed=None, device=True, ctx=None,
          return_candidates=False):
    """The reference's ``_sieve`` (:660-810) with its arguments and its 6-tuple ``(vp0_vec, vp0_type, elcbo_beta,
    compute_var, ns_ent_K, ns_ent_K_fast)``: ``vp0_vec`` an object ``ndarray`` of posteriors sorted by ascending negative
    ELCBO (``Candidates.to_vps``: the transformer is shared), ``vp0_type`` their types.  ``options``: anything with
    ``[]``; a value is a number or a callable of ``K`` (an object with the reference's ``Options.eval`` is asked through
    it).  ``return_candidates`` appends the scored ``Candidates`` (row order) and the order to the tuple."""
    if K is None:
        K = vp.K
    if init_N is None:
        init_N = math.ceil(_opt(options, "ns_elbo", K))
    ns_ent_K = math.ceil(_opt(options, "ns_ent", K) / K)
    ns_ent_K_fast = math.ceil(_opt(options, "ns_ent_fast", K) / K)
    if optim_state["entropy_switch"] or K == 1:  # (:735-737)
        ns_ent_K = 0
        ns_ent_K_fast = 0
    elcbo_beta = 0  # (:743: the reference has no elcbo weight option)
    compute_var = elcbo_beta != 0
    if init_N > 0:  # every refusal comes before vp.get_bounds touches vp.bounds and before the first draw
        check_supported(vp, K, ns_ent_K_fast, elcbo_beta)
        _rng_mode(rng)
        ctx = ctx_of(vp, ctx)
        _need_device(ctx)
    theta_bnd = vp.get_bounds(gp.X, options, K)
    if init_N > 0:
        X_star, y_star, _, _ = get_hpd(gp.X, gp.y, options["hpd_frac"])
        if best_N == 1:
            counts = (init_N, 0, 0)
        else:
            n = math.ceil(init_N / 3)
            counts = (n, n, init_N - 2 * n)
        cand = _generate(vp, counts, K, X_star, y_star, rng, seed, device, ctx, want_thetas=False)
        order, _ = score(cand, gp, theta_bnd, ctx=ctx, put=not device)
        out = (cand.to_vps()[order], cand.types[order], elcbo_beta, compute_var, ns_ent_K, ns_ent_K_fast)
        return out + (cand, order) if return_candidates else out
    return (copy.deepcopy(vp), 1, elcbo_beta, compute_var, ns_ent_K, ns_ent_K_fast)
