"""``kde_1d`` -- the reference's one-dimensional kernel density estimator (pyvbmc/stats/kde_1d.py:144),
evaluated on the MI355X (csrc/kde.hip, ``vbmc_kde_1d``).

Same signature, return triple ``(density, xmesh, bandwidth)``, shapes and argument errors as the reference.
The bandwidth has the reference's type: ``sqrt(t_star) * (upper_bound - lower_bound)`` on Botev's branch --
a length-1 array when a bound was derived from the samples, the type of the given bounds otherwise -- and
a float from Scott's rule when the fixed-point search fails.

Deviations, each where the reference computes garbage or never returns: a non-finite sample raises
``ValueError``; a mesh of more than 2^14 points raises ``UnsupportedShape``; where the reference's ``_root``
would repeat the same brentq call forever, Scott's rule is used.
"""
import numpy as np

from . import _lib

MAX_MESH = 2**14


def _call_checked(ctx, rc, who):
    """ctx.check, with VBMC_E_NONFINITE (a non-finite input, named in the library's message) as ValueError."""
    if rc == _lib.E_NONFINITE:
        msg = (ctx._lib.vbmc_last_error(ctx._h) or b"").decode()
        raise ValueError(f"{who}: non-finite input ({msg})")
    ctx.check(rc)


def _raise_degenerate(who):
    # the reference indexes its bin counts with NaN / out-of-range bins there (_linear_binning)
    raise IndexError(f"{who}: the mesh is degenerate (its spacing is 0 or not finite)")


def kde_1d(samples, n=2**14, lower_bound=None, upper_bound=None, *, ctx=None):
    """Reference signature (stats/kde_1d.py:144); keyword-only ``ctx``: the device context (default: the
    process-wide one).  Argument errors are raised before a device is touched."""
    return _kde_1d(samples, n, lower_bound, upper_bound, ctx)[:3]


def _kde_1d(samples, n, lower_bound, upper_bound, ctx):
    """kde_1d's ``(density, xmesh, bandwidth)`` and, from the same call, ``len(np.unique(samples))`` and whether
    Scott's rule gave the bandwidth."""
    samples = np.asarray(samples, dtype=np.float64).ravel()
    if n <= 0:
        raise ValueError("n cannot be <= 0")
    if lower_bound is not None and upper_bound is not None:
        if lower_bound > upper_bound:
            raise ValueError("lower_bound cannot be > upper_bound")
    n = int(2 ** np.ceil(np.log2(n)))
    if samples.size == 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    if n == 1:
        raise IndexError("index 1 is out of bounds for axis 0 with size 1")  # xmesh[1] (_linear_binning)
    lb = None if lower_bound is None else np.array([np.asarray(lower_bound, dtype=np.float64).reshape(-1)[0]])
    ub = None if upper_bound is None else np.array([np.asarray(upper_bound, dtype=np.float64).reshape(-1)[0]])
    ctx = _lib.default_context() if ctx is None else ctx
    dens = np.empty(n)
    xmesh = np.empty(n)
    bw = np.empty(1)
    info = np.empty(2, dtype=np.int64)
    x = np.ascontiguousarray(samples)
    rc = ctx._lib.vbmc_kde_1d(ctx._h, 1, x.size, _lib.ptr(x), n, _lib.ptr(lb), _lib.ptr(ub), _lib.ptr(dens),
                              _lib.ptr(xmesh), _lib.ptr(bw), info.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int64)))
    _call_checked(ctx, rc, "kde_1d")
    if info[1] & _lib.KDE_DEGENERATE:
        _raise_degenerate("kde_1d")
    scott = bool(info[1] & _lib.KDE_SCOTT)
    if scott:
        bandwidth = np.float64(bw[0])
    else:
        # np.sqrt(t_star) * delta, delta = upper_bound - lower_bound with the bounds' own types (:218-226, :243)
        lo = np.array([0.0]) if lower_bound is None else lower_bound
        hi = np.array([0.0]) if upper_bound is None else upper_bound
        shape = np.shape(np.subtract(hi, lo))
        bandwidth = np.full(shape, bw[0]) if shape else np.float64(bw[0])
    return dens, xmesh, bandwidth, int(info[0]), scott


__all__ = ["kde_1d"]
