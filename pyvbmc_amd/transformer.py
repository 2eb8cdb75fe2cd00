"""The reference's ``ParameterTransformer`` on the device (csrc/transform.hip, csrc/transform.h).

``device_transformer(pt)`` recognises a transformer by the reference's fields
(parameter_transformer/parameter_transformer.py:50-133): ``type`` (per
dimension 0 unbounded, 3 logit, 12 probit, 13 student4), ``lb_orig``, ``ub_orig``, ``mu``, ``delta``,
``R_mat`` and ``scale`` (either may be ``None``).  Anything else -- ``IdentityTransformer``, a duck
with only ``__call__`` / ``inverse`` / ``log_abs_det_jacobian``, unknown type codes -- is not
recognised (``None``), and ``VariationalPosterior`` keeps calling its own methods on the host.

The descriptor goes to the device through ``vbmc_set_transformer``: the argument tuple is built
when a field is rebound and reused while the same arrays are edited in place or left alone (the
library compares the values with what the device holds, as ``_duck.upload_vp`` does for the
mixture).  ``VBMC_HIP_TRANSFORM=0`` switches recognition off everywhere.
"""
import os

import numpy as np

from . import _lib

TYPES = (0.0, 3.0, 12.0, 13.0)
FORWARD, INVERSE, LOG_ABS_DET = 0, 1, 2
_FIELDS = ("type", "lb_orig", "ub_orig", "mu", "delta", "R_mat", "scale")


def enabled():
    """False under ``VBMC_HIP_TRANSFORM=0``: every transformer stays on the host."""
    return os.environ.get("VBMC_HIP_TRANSFORM", "1") != "0"


def candidate(pt):
    """Cheap first test, no device touched: recognition is on and ``pt`` has the reference's field names."""
    return enabled() and pt is not None and all(hasattr(pt, f) for f in _FIELDS)


def _vec(a, n):
    """``a`` as a C-contiguous float64 vector of n values (a view where it can be), or None."""
    v = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    return v if v.size == n else None


def transformer_fields(pt, D=None):
    """The transformer's fields as float64 vectors ``(type, lb, ub, mu, delta, R or None, scale or None)``,
    or ``None`` when ``pt`` is not reference-shaped.  ``D``: the posterior's dimension; a transformer of
    another dimension is an error, not a fallback."""
    if pt is None or not all(hasattr(pt, f) for f in _FIELDS):
        return None
    try:
        typ = np.ascontiguousarray(pt.type, dtype=np.float64).reshape(-1)
        n = typ.size
        if n < 1 or not np.all(np.isin(typ, TYPES)):
            return None
        out = [typ, _vec(pt.lb_orig, n), _vec(pt.ub_orig, n), _vec(pt.mu, n), _vec(pt.delta, n),
               None if pt.R_mat is None else _vec(pt.R_mat, n * n), None if pt.scale is None else _vec(pt.scale, n)]
    except (TypeError, ValueError, AttributeError):
        return None
    if D is not None and n != D:
        raise ValueError(f"parameter transformer has D={n}, the posterior D={D}")
    if any(o is None for o in out[:5]) or (pt.R_mat is not None and out[5] is None) or (
            pt.scale is not None and out[6] is None):
        return None
    b = typ != 0
    lb, ub = out[1], out[2]
    if not np.all(np.isfinite(lb[b]) & np.isfinite(ub[b]) & (lb[b] < ub[b])):
        return None  # (the reference never gives such a dimension a bounded type)
    return tuple(out)


class _XfArgs:
    """The ctypes argument tuple of vbmc_set_transformer for one set of field ARRAYS (held, so their ids stay
    theirs), reused while they are the same objects and their float64 vectors are views of them."""

    __slots__ = ("ids", "held", "args", "D")


def _ids(pt):
    return tuple(id(getattr(pt, f)) for f in _FIELDS)


def _views(held, vecs):
    return all((h is None and v is None) or (v is not None and np.shares_memory(np.asarray(h), v))
               for h, v in zip(held, vecs))


def upload(pt, ctx, slot=0, D=None):
    """Put ``pt``'s descriptor in ``ctx``'s slot; returns its dimension, or None when ``pt`` is not
    recognised (nothing is uploaded then)."""
    if not candidate(pt):
        return None
    cache = ctx.__dict__.setdefault("_xf_args", [None, None])
    st = cache[slot]
    ids = _ids(pt)
    if st is None or st.ids != ids:
        f = transformer_fields(pt, D)
        if f is None:
            cache[slot] = None
            return None
        held = tuple(getattr(pt, k) for k in _FIELDS)
        st = _XfArgs()
        st.ids, st.held, st.D = ids, (held, f), f[0].size
        st.args = (ctx._h, slot, st.D) + tuple(_lib.ptr(a) for a in f)
        cache[slot] = st if _views(held, f) else None  # (converted copies: rebuilt on every call)
    elif D is not None and st.D != D:
        raise ValueError(f"parameter transformer has D={st.D}, the posterior D={D}")
    ctx.check(ctx._lib.vbmc_set_transformer(*st.args))
    return st.D


def device_transformer(pt, ctx=None):
    """A ``DeviceTransformer`` for ``pt`` when it is reference-shaped, else ``None``."""
    if not enabled() or transformer_fields(pt) is None:
        return None
    return DeviceTransformer(pt, ctx)


def same_by_value(a, b):
    """Two recognised transformers with equal fields (the reference's ``__eq__`` compares the same ones)."""
    fa, fb = transformer_fields(a), transformer_fields(b)
    if fa is None or fb is None:
        return False
    return all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y))
               for x, y in zip(fa, fb))


def _lift(x):
    """handle_0D_1D_input: 0-D and 1-D inputs as one row (reference decorators/handle_0D_1D_input.py)."""
    return np.ndim(x), np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)


class DeviceTransformer:
    """The reference transformer's three calls, evaluated on the device with ``pt``'s fields (re-read on
    every call, so edits of ``pt`` are seen)."""

    def __init__(self, pt, ctx=None):
        self.pt = pt
        self._ctx = ctx

    @property
    def ctx(self):
        return self._ctx if self._ctx is not None else _lib.default_context()

    def __getattr__(self, name):  # lb_orig, ub_orig, type, ... of the wrapped transformer
        if name in ("pt", "_ctx"):
            raise AttributeError(name)
        return getattr(self.pt, name)

    def _run(self, x, direction):
        ctx = self.ctx
        D = upload(self.pt, ctx, 0)
        if D is None:
            raise ValueError("not a reference-shaped parameter transformer (or VBMC_HIP_TRANSFORM=0)")
        return transform_points(ctx, x, direction, D)

    def __call__(self, x):
        dims, x = _lift(x)
        u = self._run(x, FORWARD)
        return u.ravel() if dims == 1 else u

    def inverse(self, u):
        dims, u = _lift(u)
        x = self._run(u, INVERSE)
        return x.ravel() if dims == 1 else x

    def log_abs_det_jacobian(self, u):
        dims, u = _lift(u)
        p = self._run(u, LOG_ABS_DET)
        return p.ravel()[0] if dims == 1 else p


def transform_points(ctx, x, direction, D):
    """Slot 0's transformer (uploaded, dimension D) on the rows of ``x`` (n x D)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] != D:
        raise ValueError(f"points of shape {x.shape}, the transformer D={D}")
    n = x.shape[0]
    out = np.empty(n) if direction == LOG_ABS_DET else np.empty((n, D))
    ctx.check(ctx._lib.vbmc_transform(ctx._h, n, direction, _lib.ptr(x), _lib.ptr(out)))
    return out


__all__ = ["DeviceTransformer", "device_transformer", "transformer_fields", "same_by_value", "upload", "enabled",
           "FORWARD", "INVERSE", "LOG_ABS_DET"]
