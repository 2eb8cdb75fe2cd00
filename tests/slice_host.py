"""The slice sampler of ``vbmc_is_mcmc`` (pyvbmc_amd/csrc/acq_is_mcmc.hip), stated once in NumPy.  TEST INFRASTRUCTURE:
the device chains are replayed against it (tests/test_ais_mcmc_gpu.py), and its law is checked on a target with known
moments (tests/test_slice_host.py).

This is NOT a restatement of ``gpyreg.slice_sample.SliceSampler`` (gpyreg is not part of the reference tree): it is
Neal's (2003, Ann. Statist. 31) coordinate-wise slice sampler with stepping out and shrinkage, defined here.  Its draws
are its own counter-based stream, not ``np.random``'s.

Chain ``s`` from ``x`` (clipped into ``[lb, ub]``) runs ``burn_in + n thin`` sweeps; a sweep updates the coordinates
d = 0 .. D-1 in order.  One coordinate update:

1. level   ``ly = f(x) + log(u)``, u in (0, 1];
2. interval ``L = x_d - widths_d u'``, ``R = L + widths_d``, both clipped to ``[lb_d, ub_d]``;
3. step out left, at most 32 evaluations: stop when ``L <= lb_d`` or ``f(x | x_d = L) <= ly``, otherwise
   ``L = max(L - widths_d, lb_d)``;
4. step out right the same way against ``ub_d``;
5. shrink, at most 64 proposals ``x' = L + u'' (R - L)``: accept when ``f(x') > ly``, otherwise ``L = x'`` if
   ``x' < x_d`` else ``R = x'``; when the cap is reached ``x_d`` stays (and the event is counted);
6. after sweep t, when ``t >= burn_in`` and ``(t - burn_in + 1) % thin == 0``, ``x`` and the ``f(x)`` in hand are kept.

Draw i of chain s (i counts up from 0 in the order the draws are consumed above) is the 53-bit uniform of the words 0
and 1 of Philox block ``(i_lo, i_hi, s, 6)`` with key ``seed`` (oracle/philox_ref.philox4x32_10): the level's in the
(0, 1] form ``(a + 1) 2^-53``, every other one in the [0, 1) form ``a 2^-53``.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import philox_ref  # noqa: E402

OUT_CAP, SHRINK_CAP, STREAM = 32, 64, 6


class Draws:
    """The uniforms of chain ``s`` under ``seed``, in order."""

    CHUNK = 1024  # draws generated per call of the (vectorised) block function

    def __init__(self, seed, s):
        self.seed, self.s, self.i = int(seed), int(s), 0
        self._base, self._buf = -1, None

    def _bits(self):
        i = self.i
        self.i += 1
        base = i - i % self.CHUNK
        if base != self._base:
            idx = np.arange(base, base + self.CHUNK, dtype=np.uint64)
            lo, hi = (idx & philox_ref.MASK).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32)
            x0, x1, _, _ = philox_ref.philox4x32_10(lo, hi, np.full_like(lo, self.s), np.full_like(lo, STREAM),
                                                    self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF)
            self._buf = ((x0.astype(np.uint64) << np.uint64(32)) | x1.astype(np.uint64)) >> np.uint64(11)
            self._base = base
        return int(self._buf[i - base])

    def u(self):
        """[0, 1)"""
        return self._bits() * 2.0**-53

    def u_pos(self):
        """(0, 1]"""
        return (self._bits() + 1) * 2.0**-53


def chain(log_p, x0, widths, lb, ub, n, thin=1, burn_in=0, seed=0, s=0):
    """One chain.  ``log_p(x)`` is called with a (D,) array and may return a scalar or any array of one element.
    Returns a dict: ``samples`` (n, D), ``f_vals`` (n,), ``stats`` = [evaluations, draws, step-out caps hit, shrink caps
    hit] and ``margin``, the smallest ``|f - ly|`` over all the comparisons made (inf when none was)."""
    widths, lb, ub = (np.asarray(a, dtype=np.float64).ravel() for a in (widths, lb, ub))
    x = np.maximum(np.minimum(np.array(x0, dtype=np.float64).ravel(), ub), lb)
    D = x.size
    rng = Draws(seed, s)
    st = {"evals": 0, "caps_out": 0, "caps_shrink": 0, "margin": np.inf}

    def f(pt):
        st["evals"] += 1
        return float(np.ravel(log_p(pt))[0])

    def at(d, v):
        y = x.copy()
        y[d] = v
        return f(y)

    def seen(fv, ly):
        if np.isfinite(fv) and np.isfinite(ly):
            st["margin"] = min(st["margin"], abs(fv - ly))

    fx = f(x)
    if not np.isfinite(fx):
        raise ValueError("Invalid value.")
    samples, f_vals = [], []
    for t in range(burn_in + n * thin):
        for d in range(D):
            xd, w, lo, hi = x[d], widths[d], lb[d], ub[d]
            ly = fx + np.log(rng.u_pos())
            L = xd - w * rng.u()
            R = L + w
            L, R = max(L, lo), min(R, hi)
            j = 0
            while True:
                if L <= lo:
                    break
                if j == OUT_CAP:
                    st["caps_out"] += 1
                    break
                fl = at(d, L)
                seen(fl, ly)
                if fl <= ly:
                    break
                L, j = max(L - w, lo), j + 1
            j = 0
            while True:
                if R >= hi:
                    break
                if j == OUT_CAP:
                    st["caps_out"] += 1
                    break
                fr = at(d, R)
                seen(fr, ly)
                if fr <= ly:
                    break
                R, j = min(R + w, hi), j + 1
            for j in range(SHRINK_CAP):
                xp = L + rng.u() * (R - L)
                fp = at(d, xp)
                seen(fp, ly)
                if fp > ly:
                    x[d], fx = xp, fp
                    break
                if xp < xd:
                    L = xp
                else:
                    R = xp
            else:
                st["caps_shrink"] += 1
        if t >= burn_in and (t - burn_in + 1) % thin == 0:
            samples.append(x.copy())
            f_vals.append(fx)
    return {"samples": np.array(samples).reshape(n, D), "f_vals": np.array(f_vals),
            "stats": np.array([st["evals"], rng.i, st["caps_out"], st["caps_shrink"]], dtype=np.int64),
            "margin": st["margin"]}


def sampler_class(seed):
    """A class with ``gpyreg.slice_sample.SliceSampler``'s interface, ``cls(log_p, x0, widths, lb, ub, opts)
    .sample(N, thin, burn_in) -> {"samples", "f_vals"}``, over ``chain`` under ``seed``: its instances take the chain
    indices 0, 1, ... in construction order, as the chains of step 2 are built.  ``cls.results`` collects what every
    ``sample`` call returned (stats and margin included)."""

    class SliceHost:
        results = []
        _next = [0]

        def __init__(self, log_p, x0, widths, lb, ub, opts=None):
            x0 = np.asarray(x0, dtype=np.float64)
            if x0.ndim > 1 and x0.shape[0] != 1:
                raise NotImplementedError("slice_host: one walker per chain (a matrix of walkers is step 0's)")
            self.args = (log_p, x0.ravel(), widths, lb, ub)
            self.s = self._next[0]
            self._next[0] += 1

        def sample(self, N, thin=1, burn_in=0):
            res = chain(*self.args, int(N), int(thin), int(burn_in), seed=seed, s=self.s)
            self.results.append(res)
            return {"samples": res["samples"], "f_vals": res["f_vals"]}

    return SliceHost
