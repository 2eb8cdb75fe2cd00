"""The CMA-ES of the acquisition search's refinement in NumPy: the algorithm csrc/cmaes.hip runs on the device, with the
same Philox draws (stream 8 of csrc/sample.hip).  ``fmin`` is the ``device=False`` route of
``pyvbmc_amd.active_search.refine`` and works for any batched objective.

The optimiser is this package's own -- ``cma`` (the reference's ``cma.fmin``, vbmc/active_sample.py:398-404) is a
third-party package with a stream of its own, and there is nothing to be bit-compatible with.  It is a
(mu/mu_w, lambda)-CMA-ES for minimisation in a box: the covariance C is kept explicitly and its lower Cholesky factor
recomputed every generation; candidates are clipped to the box and the update uses the repaired steps
``y = (x - m) / sigma`` and ``z' = L^-1 y`` (no penalty term, no resampling).  The reference wraps its call in
``cma.NoiseHandler``; the acquisition functions are deterministic, so there is no noise handling here.

Every sum is taken in rank order, then ``d`` ascending, one multiply and one add per term: NumPy's elementwise operations
round as the kernel's do, so a run here and a run on the device differ only by the last bits of ``exp``, ``1 / sqrt``,
``1 / sigma`` and the normals (fastmath.h there, libm here).

Stop reasons (``stats[2]``), checked after the update, the first that holds: 1 ``tolfun``, 2 ``tolx``, 3 ``maxfevals``,
4 ``condition``, 5 ``invalid`` (a generation, or the start, without a finite value).
"""
import math
from types import SimpleNamespace

import numpy as np

STREAM = 8
_GOLDEN = 0x9E3779B97F4A7C15
STOP_REASONS = {0: "running", 1: "tolfun", 2: "tolx", 3: "maxfevals", 4: "condition", 5: "invalid"}
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def sub_seed(seed, r):
    """The key of run ``r``: ``seed + (r + 1) * 0x9E3779B97F4A7C15`` modulo 2^64 (``active_search.sub_seed``)."""
    return (int(seed) + (r + 1) * _GOLDEN) % 2**64


def default_lambda(D):
    return 4 + int(math.floor(3.0 * math.log(D)))


def constants(D, lam):
    """The strategy constants in float64, operation for operation what csrc/api_cmaes.hip computes."""
    d = float(D)
    mu = lam // 2
    w = [math.log((lam + 1) / 2.0) - math.log(float(i + 1)) for i in range(mu)]
    sw = 0.0
    for v in w:
        sw = sw + v
    w = [v / sw for v in w]
    s2 = 0.0
    for v in w:
        s2 = s2 + v * v
    mueff = 1.0 / s2
    cs = (mueff + 2.0) / (d + mueff + 5.0)
    ds = 1.0 + 2.0 * max(0.0, math.sqrt((mueff - 1.0) / (d + 1.0)) - 1.0) + cs
    cc = (4.0 + mueff / d) / (d + 4.0 + 2.0 * mueff / d)
    c1 = 2.0 / ((d + 1.3) * (d + 1.3) + mueff)
    cmu = min(1.0 - c1, 2.0 * (mueff - 2.0 + 1.0 / mueff) / ((d + 2.0) * (d + 2.0) + mueff))
    chi = math.sqrt(d) * (1.0 - 1.0 / (4.0 * d) + 1.0 / (21.0 * d * d))
    one_cs, one_cc = 1.0 - cs, 1.0 - cc
    return SimpleNamespace(mu=mu, w=np.array(w), mueff=mueff, cs=cs, ds=ds, cc=cc, c1=c1, cmu=cmu, chi=chi,
                           hist=10 + (30 * D + lam - 1) // lam, one_cs=one_cs, a_ps=math.sqrt(cs * (2.0 - cs) * mueff),
                           q_cs=one_cs * one_cs, hs_thresh=(1.4 + 2.0 / (d + 1.0)) * chi, one_cc=one_cc,
                           a_pc=math.sqrt(cc * (2.0 - cc) * mueff), c_old=1.0 - c1 - cmu, cc2=cc * (2.0 - cc), cs_ds=cs / ds,
                           inv_chi=1.0 / chi)


def _philox(c0, c1, c2, c3, key):
    """Philox4x32-10 (Salmon et al., SC'11) on equal-shaped uint32 arrays."""
    k0, k1 = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LOW, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LOW
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def normals(n0, count, D, key):
    """``count x D`` standard normals: row i from the blocks ``(n_lo, n_hi, pair, 8)``, ``n = n0 + i``, under ``key``
    (csrc/mixture_dev.h philox_normal_pair: Box-Muller on 53-bit uniforms)."""
    n = np.arange(count, dtype=np.uint64) + np.uint64(n0)
    out = np.empty((count, D))
    for p in range((D + 1) // 2):
        x0, x1, x2, x3 = _philox(n & _LOW, n >> _S32, np.full(count, p), np.full(count, STREAM), key)
        u1 = ((((x0 << _S32) | x1) >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0**-53
        u2 = (((x2 << _S32) | x3) >> np.uint64(11)).astype(np.float64) * 2.0**-53
        rad = np.sqrt(-2.0 * np.log(u1))
        out[:, 2 * p] = rad * np.cos(2.0 * np.pi * u2)
        if 2 * p + 1 < D:
            out[:, 2 * p + 1] = rad * np.sin(2.0 * np.pi * u2)
    return out


def rank(values):
    """Ascending order of the values, the index breaks ties, NaN behind +inf (-0 equals +0)."""
    v = np.asarray(values, dtype=np.float64)
    return np.array(sorted(range(v.size), key=lambda i: (1, 0.0, i) if v[i] != v[i] else (0, float(v[i]), i)), dtype=np.int64)


def _cholesky(C):
    """Column-by-column lower factor with L_jj = s / sqrt(s) formed as s * (1 / sqrt(s)); ``(L, 1 / diag L, ok)``."""
    D = C.shape[0]
    L, rd = np.zeros((D, D)), np.ones(D)
    for j in range(D):
        s = float(C[j, j])
        for k in range(j):
            s = s - float(L[j, k]) * float(L[j, k])
        if not (s > 0.0 and s < math.inf):
            return L, rd, False
        r = 1.0 / math.sqrt(s)
        L[j, j], rd[j] = s * r, r
        t = C[j + 1:, j].copy()
        for k in range(j):
            t = t - L[j + 1:, k] * L[j, k]
        L[j + 1:, j] = t * r
    return L, rd, True


def fmin(f_batch, x0, sigma0, lb, ub, *, lam=None, max_fevals, tol_fun, tol_x=None, seed, run=0, evaluated=None):
    """Minimise ``f_batch`` in the box ``[lb, ub]`` from ``x0`` with initial step ``sigma0``.

    ``f_batch(X)``: the values of the rows of ``X`` (n x D), one call per generation.  ``evaluated(X)`` (optional): the
    points that are evaluated in place of the optimiser's -- the rounding of integer variables; the optimiser goes on
    with its own point, the evaluated one is what becomes the best.  ``run``: the index r whose key ``sub_seed(seed, r)``
    draws the normals.  Returns the fields of ``vbmc_search_cmaes``: ``x_best``, ``f_best``, ``f0``, ``mean``, ``sigma``,
    ``C``, ``stats`` = [generations, evaluations, stop reason, generation of the best (0: the start)]."""
    x0, lb, ub = (np.array(np.ravel(a), dtype=np.float64) for a in (x0, lb, ub))
    D = x0.size
    lam = default_lambda(D) if lam is None else int(lam)
    if D < 2 or D > 32 or lam < 4 or lam > 64:
        raise ValueError(f"cmaes.fmin: D={D}, lambda={lam} outside 2 <= D <= 32, 4 <= lambda <= 64")
    if not sigma0 > 0 or np.any(lb > ub) or np.any(x0 < lb) or np.any(x0 > ub) or max_fevals < 1 + lam:
        raise ValueError("cmaes.fmin: needs sigma0 > 0, lb <= x0 <= ub and max_fevals >= 1 + lambda")
    c = constants(D, lam)
    key = sub_seed(seed, run)
    sigma0 = float(sigma0)
    tol_x = float(tol_x) if tol_x is not None and tol_x > 0 else 1e-11 * sigma0
    evaluated = evaluated if evaluated is not None else (lambda X: X)

    def evaluate(X):
        Xe = np.array(evaluated(X.copy()), dtype=np.float64).reshape(X.shape)
        return Xe, np.asarray(f_batch(Xe.copy()), dtype=np.float64).ravel()

    m, sigma = x0.copy(), sigma0
    C, L, rd = np.eye(D), np.eye(D), np.ones(D)
    ps, pc = np.zeros(D), np.zeros(D)
    decay = 1.0
    ring = []
    Xe, f = evaluate(x0[None, :])
    x_best, f_best, f0 = Xe[0].copy(), float(f[0]), float(f[0])
    gen, evals, best_gen, reason = 0, 1, 0, 0
    if not math.isfinite(f0):
        reason = 5
    while not reason:
        # the generation: x = clip(m + sigma L z), y = (x - m) / sigma, z' = L^-1 y
        Z = normals(gen * lam, lam, D, key)
        LZ = np.zeros((lam, D))
        for k in range(D):
            LZ[:, k:] = LZ[:, k:] + L[k:, k][None, :] * Z[:, k:k + 1]
        X = m[None, :] + sigma * LZ
        X = np.where(X < lb, lb, X)
        X = np.where(X > ub, ub, X)
        Y = (X - m[None, :]) * (1.0 / sigma)
        acc, Zp = Y.copy(), np.empty((lam, D))
        for d in range(D):
            Zp[:, d] = acc[:, d] * rd[d]
            acc[:, d + 1:] = acc[:, d + 1:] - L[d + 1:, d][None, :] * Zp[:, d:d + 1]
        Xe, f = evaluate(X)
        order = rank(f)
        evals += lam
        gen += 1
        vbest = float(f[order[0]])
        if not math.isfinite(vbest):
            reason = 5
            break
        if vbest < f_best:
            x_best, f_best, best_gen = Xe[order[0]].copy(), vbest, gen
        # the update
        yw, zw = np.zeros(D), np.zeros(D)
        for i in range(c.mu):
            yw = yw + c.w[i] * Y[order[i]]
            zw = zw + c.w[i] * Zp[order[i]]
        m = m + sigma * yw
        ps = c.one_cs * ps + c.a_ps * zw
        n2 = 0.0
        for d in range(D):
            n2 = n2 + float(ps[d]) * float(ps[d])
        nps = math.sqrt(n2)
        decay = decay * c.q_cs
        hs = 1.0 if nps * (1.0 / math.sqrt(1.0 - decay)) < c.hs_thresh else 0.0
        pc = c.one_cc * pc + (hs * c.a_pc) * yw
        keep = (1.0 - hs) * c.cc2
        Cn = c.c_old * C + c.c1 * (pc[:, None] * pc[None, :] + keep * C)
        for k in range(c.mu):
            y = Y[order[k]]
            Cn = Cn + (c.cmu * c.w[k]) * (y[:, None] * y[None, :])
        C = Cn
        sigma = sigma * math.exp(c.cs_ds * (nps * c.inv_chi - 1.0))
        L, rd, ok = _cholesky(C)
        # the stop rules
        ring.append(vbest)
        ring = ring[-c.hist:]
        fin = f[np.isfinite(f)]
        if len(ring) >= c.hist and max(ring) - min(ring) < tol_fun and float(fin.max()) - vbest < tol_fun:
            reason = 1
        elif sigma * max(max(math.sqrt(C[d, d]) if C[d, d] > 0 else 0.0, abs(float(pc[d]))) for d in range(D)) < tol_x:
            reason = 2
        elif evals + lam > max_fevals:
            reason = 3
        elif not ok:
            reason = 4
        else:
            dl = np.diag(L)
            if float(dl.max()) * float(dl.max()) > 1e14 * (float(dl.min()) * float(dl.min())):
                reason = 4
    return SimpleNamespace(x_best=x_best, f_best=f_best, f0=f0, mean=m, sigma=sigma, C=C,
                           stats=np.array([gen, evals, reason, best_gen], dtype=np.int64))


__all__ = ["fmin", "constants", "default_lambda", "normals", "rank", "sub_seed", "STOP_REASONS", "STREAM"]
