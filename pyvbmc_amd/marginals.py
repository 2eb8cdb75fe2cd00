"""``VariationalPosterior.marginals`` and ``plot``: the numbers of a corner plot, and the plot.

The reference's ``plot`` (variational_posterior/variational_posterior.py:1129-1285) draws 1e5 samples and hands them to
``corner.corner`` (:1191-1206), which histograms every dimension and every pair.  Here that is ``marginals``: one device
call (csrc/marginals.hip, ``vbmc_marginals``) on a million samples that never leave the device, returning a ``Marginals``
object; ``plot`` draws it with matplotlib alone.

The rules (the package's own; ``device=False`` states them in NumPy and is what the device route is tested against):

Samples.  ``samples``, an ``(n, D)`` array in the space ``orig_flag`` names, is used when given (``N`` is ignored).
Otherwise the posterior's own draws are: the draws of ``vp.sample(N, orig_flag, rng=..., seed=...)``.  With
``rng="philox"`` they are made on the device and never come to the host (as ``mtv``'s); with ``rng="numpy"`` they come
from ``vp.sample`` on the host and are uploaded once.  A non-finite sample raises ``ValueError``.  Every output is
invariant under a permutation of the samples.

Ranges.  ``ranges=None``: each dimension uses ``[min, max]`` of its column, ``(min - 0.5, max + 0.5)`` when they are
equal (``np.histogram``'s rule).  Or a ``(D, 2)`` array, or a length-D list of ``None`` / ``(lo, hi)``.

Binning is ``np.histogram(x, bins, range=(lo, hi))`` and ``np.histogram2d`` exactly: edges from ``linspace``, the
index from the scaled position corrected against the two neighbouring edges, ``x == hi`` in the last bin.  A sample
outside a dimension's range is left out of that dimension's histogram and of every pair that contains the dimension.

Quantiles.  ``np.quantile``'s default (linear) rule on the sorted column.

Levels.  For pair p and level l: the cells sorted by count, descending; the shortest non-empty prefix whose sum is
``>= l * inside2[p]``; ``level_counts`` is the count of the last cell taken and ``level_mass`` the mass of all cells with
at least that count, over ``inside2[p]`` (NaN for an empty pair) -- so ties never matter, and ``level_mass >= l``.  A
contour at density ``level_counts / (n * cell area)`` is what a plot draws.

Limits.  1 <= D <= 32, 1 <= bins <= 128, 1 <= n <= ``MAX_SAMPLES`` = 2^22: ``UnsupportedShape`` beyond, before a
draw or a launch.  The cap is the exact sort's: its whole-column stage is one workgroup per column (csrc/colsort.h),
measured at 26 ms for 1e6 samples and 146-197 ms for 2^22 on an MI355X (profiles/marginals.md), and with the kde the
columns are sorted twice: a call at the cap stays under half a second.  A wrong ``samples`` shape, a level or quantile outside
[0, 1], ``lo >= hi`` and ``bins < 1`` are ``ValueError``, raised before a device is touched.

``device=False`` is the same function in NumPy (``np.histogram``, a loop of ``np.histogram2d`` over the pairs,
``np.quantile``, a sort of the cells) and needs no device: with ``samples=None`` it draws through ``vp.sample`` on the
host (``rng="numpy"``).  The package's ``kde_1d`` is left out there unless a context is given.
"""
import ctypes as C
import logging

import numpy as np

from . import _lib

MAX_D = 32
MAX_BINS = 128
MAX_SAMPLES = 2**22
KDE_MESH = 2**10

_log = logging.getLogger(__name__)


class Marginals:
    """The result of ``VariationalPosterior.marginals``: plain attributes (see the module docstring).

    ``n`` samples used; ``pairs`` (P, 2), i < j in row-major order; ``edges`` (D, bins + 1); ``counts1`` (D, bins);
    ``counts2`` (P, bins, bins), ``counts2[p, a, b]``: dimension i in bin a and j in bin b; ``inside1`` (D,), ``inside2``
    (P,); ``quantile_levels`` and ``quantiles`` (len, D); ``levels``, ``level_counts`` and ``level_mass`` (P, len);
    ``kde_x``, ``kde_density`` (D, 2^10) and ``kde_bandwidth`` (D,), or None without the kde."""

    _FIELDS = ("n", "pairs", "edges", "counts1", "counts2", "inside1", "inside2", "quantile_levels", "quantiles", "levels",
               "level_counts", "level_mass", "kde_x", "kde_density", "kde_bandwidth")

    def __init__(self, **fields):
        for name in self._FIELDS:
            setattr(self, name, fields.get(name))

    def density1(self, d):
        """The 1-D histogram of dimension ``d`` as a density: counts over ``n`` and the bin width."""
        return self.counts1[d] / (self.n * np.diff(self.edges[d]))

    def density2(self, p):
        """The histogram of pair ``p`` as a density: counts over ``n`` and the cell area."""
        i, j = self.pairs[p]
        return self.counts2[p] / (self.n * np.outer(np.diff(self.edges[i]), np.diff(self.edges[j])))

    def __eq__(self, other):
        if not isinstance(other, Marginals):
            return NotImplemented

        def same(a, b):
            if a is None or b is None:
                return a is None and b is None
            return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=np.asarray(a).dtype.kind == "f")

        return all(same(getattr(self, f), getattr(other, f)) for f in self._FIELDS)

    __hash__ = None

    def __repr__(self):
        q = np.asarray(self.quantile_levels, dtype=np.float64)
        head = f"Marginals(n={self.n}, D={self.edges.shape[0]}, bins={self.edges.shape[1] - 1})"
        if q.size == 0:
            return head
        mid = int(np.argmin(np.abs(q - 0.5)))
        lo, hi = int(np.argmin(q)), int(np.argmax(q))
        rows = [f"{head}: quantile {q[mid]:g} [{q[lo]:g}, {q[hi]:g}]"]
        for d in range(self.edges.shape[0]):
            v = self.quantiles[:, d]
            rows.append(f"  x[{d}] = {v[mid]: .6g}  [{v[lo]: .6g}, {v[hi]: .6g}]")
        return "\n".join(rows)


def pair_table(D):
    """``(P, 2)``: the pairs i < j in row-major order."""
    return np.array([(i, j) for i in range(D) for j in range(i + 1, D)], dtype=np.int64).reshape(-1, 2)


def _ranges_arg(ranges, D):
    """``ranges`` as a (D, 2) float64 array, NaN rows for None; ValueError for a wrong shape or lo >= hi."""
    out = np.full((D, 2), np.nan)
    if ranges is None:
        return out
    if isinstance(ranges, np.ndarray) and ranges.dtype != object:
        if ranges.shape != (D, 2):
            raise ValueError(f"ranges of shape {ranges.shape}, expected ({D}, 2)")
        rows = list(ranges)
    else:
        rows = list(ranges)
        if len(rows) != D:
            raise ValueError(f"ranges of length {len(rows)}, the posterior D={D}")
    for d, r in enumerate(rows):
        if r is None:
            continue
        r = np.asarray(r, dtype=np.float64).reshape(-1)
        if r.size != 2:
            raise ValueError(f"ranges[{d}] is not (lo, hi)")
        if not (np.isfinite(r[0]) and np.isfinite(r[1]) and r[0] < r[1]):
            raise ValueError(f"ranges[{d}] = ({r[0]}, {r[1]}): lo < hi, both finite, is required")
        out[d] = r
    return out


def _unit_levels(values, what):
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    if not np.all((v >= 0.0) & (v <= 1.0)):
        raise ValueError(f"{what} outside [0, 1]: {values}")
    return np.ascontiguousarray(v)


def _check_shape(D, bins, n):
    if not 1 <= D <= MAX_D:
        raise _lib.UnsupportedShape(f"marginals: D={D} outside 1..{MAX_D}")
    if bins > MAX_BINS:
        raise _lib.UnsupportedShape(f"marginals: bins={bins} > {MAX_BINS}")
    if n > MAX_SAMPLES:
        raise _lib.UnsupportedShape(f"marginals: {n} samples > {MAX_SAMPLES}")


def levels_of(counts, levels):
    """``(level_counts, level_mass)`` of one table of cell counts (the Levels rule of the module docstring)."""
    c = np.sort(np.asarray(counts, dtype=np.int64).ravel())[::-1]
    cum = np.cumsum(c)
    inside = int(cum[-1])
    lc = np.zeros(len(levels), dtype=np.int64)
    lm = np.full(len(levels), np.nan)
    for k, lev in enumerate(levels):
        first = int(np.argmax(cum >= lev * float(inside)))
        lc[k] = c[first]
        if inside:
            lm[k] = int(c[c >= c[first]].sum()) / inside
    return lc, lm


def marginals_host(x, bins, ranges, quantiles, levels):
    """The NumPy statement of ``marginals`` on the samples ``x`` (n, D); ``ranges``: (D, 2) with NaN rows for None."""
    n, D = x.shape
    if not np.all(np.isfinite(x)):
        raise ValueError("marginals: non-finite input (a sample is NaN or infinite)")
    pairs = pair_table(D)
    rng = []
    for d in range(D):
        lo, hi = ranges[d]
        if np.isnan(lo):
            lo, hi = float(x[:, d].min()), float(x[:, d].max())
            if lo == hi:
                lo, hi = lo - 0.5, hi + 0.5
        rng.append((lo, hi))
    edges = np.empty((D, bins + 1))
    counts1 = np.empty((D, bins), dtype=np.int64)
    for d in range(D):
        counts1[d], edges[d] = np.histogram(x[:, d], bins, range=rng[d])
    counts2 = np.zeros((len(pairs), bins, bins), dtype=np.int64)
    lc = np.zeros((len(pairs), len(levels)), dtype=np.int64)
    lm = np.full((len(pairs), len(levels)), np.nan)
    for p, (i, j) in enumerate(pairs):
        h = np.histogram2d(x[:, i], x[:, j], bins, range=[rng[i], rng[j]])[0]
        counts2[p] = h.astype(np.int64)
        lc[p], lm[p] = levels_of(counts2[p], levels)
    q = np.quantile(x, quantiles, axis=0).reshape(len(quantiles), D) if len(quantiles) else np.empty((0, D))
    return Marginals(n=n, pairs=pairs, edges=edges, counts1=counts1, counts2=counts2, inside1=counts1.sum(axis=1),
                     inside2=counts2.sum(axis=(1, 2)), quantile_levels=quantiles.copy(), quantiles=q,
                     levels=levels.copy(), level_counts=lc, level_mass=lm)


def _add_kde(m, x, ctx):
    """The kde fields of ``m`` through the package's ``kde_1d``, a call per column (the host route with a context)."""
    from .stats import kde_1d

    D = x.shape[1]
    m.kde_x = np.empty((D, KDE_MESH))
    m.kde_density = np.empty((D, KDE_MESH))
    m.kde_bandwidth = np.empty(D)
    for d in range(D):
        dens, mesh, bw = kde_1d(x[:, d], KDE_MESH, m.edges[d, 0], m.edges[d, -1], ctx=ctx)
        m.kde_density[d], m.kde_x[d], m.kde_bandwidth[d] = dens, mesh, float(np.ravel(bw)[0])


def _device_call(ctx, D, side, orig_flag, bins, rng2, q, lev, kde, stage_ms=None):
    """vbmc_marginals on the samples ``side`` names; returns the ``Marginals``."""
    from .stats import _call_checked

    P = D * (D - 1) // 2
    i64 = C.POINTER(C.c_int64)
    edges = np.empty((D, bins + 1))
    counts1 = np.empty((D, bins), dtype=np.int64)
    counts2 = np.zeros((P, bins, bins), dtype=np.int64)
    inside2 = np.zeros(P, dtype=np.int64)
    quant = np.empty((len(q), D))
    lc = np.zeros((P, len(lev)), dtype=np.int64)
    lm = np.full((P, len(lev)), np.nan)
    mesh = KDE_MESH if kde else 0
    kx, kd, kb = (np.empty((D, mesh)), np.empty((D, mesh)), np.empty(D)) if kde else (None, None, None)
    rc = ctx._lib.vbmc_marginals(
        ctx._h, D, C.byref(side), int(bool(orig_flag)), bins, _lib.ptr(rng2), len(q), _lib.ptr(q), len(lev), _lib.ptr(lev),
        mesh, _lib.ptr(edges), counts1.ctypes.data_as(i64), counts2.ctypes.data_as(i64), inside2.ctypes.data_as(i64),
        _lib.ptr(quant), lc.ctypes.data_as(i64), _lib.ptr(lm), _lib.ptr(kx), _lib.ptr(kd), _lib.ptr(kb),
        None if stage_ms is None else stage_ms.ctypes.data_as(C.POINTER(C.c_float)))
    _call_checked(ctx, rc, "marginals")
    return Marginals(n=int(side.n), pairs=pair_table(D), edges=edges, counts1=counts1, counts2=counts2,
                     inside1=counts1.sum(axis=1), inside2=inside2, quantile_levels=q.copy(), quantiles=quant,
                     levels=lev.copy(), level_counts=lc, level_mass=lm, kde_x=kx, kde_density=kd, kde_bandwidth=kb)


def marginals(vp, N=int(1e6), bins=40, ranges=None, quantiles=(0.025, 0.16, 0.5, 0.84, 0.975), levels=(0.5, 0.9),
              orig_flag=True, samples=None, kde=True, *, rng=None, seed=None, device=True, ctx=None, stage_ms=None):
    """``VariationalPosterior.marginals`` (the module docstring has the rules).  ``stage_ms``: a float32 array of 6 that
    the device route fills with the times of its stages (samples, sort, kde, bin indices, pair histograms, levels)."""
    from . import transformer as _xf
    from . import variational_posterior as _vpmod

    D = int(vp.D)
    bins = int(bins)
    if bins < 1:
        raise ValueError(f"bins={bins} < 1")
    q = _unit_levels(quantiles, "quantile")
    lev = _unit_levels(levels, "level")
    rng2 = np.ascontiguousarray(_ranges_arg(ranges, D))
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.float64)
        if samples.ndim != 2 or samples.shape[1] != D or samples.shape[0] < 1:
            raise ValueError(f"samples of shape {samples.shape}, the posterior D={D}")
        n = samples.shape[0]
    else:
        n = int(N)
        if n < 1:
            raise ValueError(f"N={N} < 1")
    mode = "numpy" if (samples is not None or not device) and rng is None else _vpmod._rng_mode(rng)
    _check_shape(D, bins, n)

    if not device:
        if samples is None:
            samples, _ = vp.sample(n, orig_flag, rng="numpy")
        m = marginals_host(samples, bins, rng2, q, lev)
        if kde and ctx is not None:
            _add_kde(m, samples, ctx)
        return m

    if samples is None and mode == "philox":
        # the draws of sample(n, orig_flag, rng="philox", seed): on the device when the transformer can go to its slot
        ident = isinstance(vp.parameter_transformer, _vpmod.IdentityTransformer)
        dctx = vp._upload(ctx)
        seed = _vpmod._seed_or_draw(seed)
        to_orig = bool(orig_flag) and not ident
        if not to_orig or _xf.upload(vp.parameter_transformer, dctx, 0, D) is not None:
            side = _lib.MtvSide(_lib.MTV_MIX1, n, None, int(seed), None, None)
            return _device_call(dctx, D, side, to_orig, bins, rng2, q, lev, kde, stage_ms)
        vp_ctx, vp._ctx = vp._ctx, dctx
        try:
            samples, _ = vp.sample(n, orig_flag, rng="philox", seed=seed)
        finally:
            vp._ctx = vp_ctx
    elif samples is None:
        samples, _ = vp.sample(n, orig_flag, rng="numpy")
    if ctx is None:
        ctx = vp.ctx
    x = _lib.f64(samples)
    side = _lib.MtvSide(_lib.MTV_HOST, n, _lib.ptr(x), 0, None, None)
    return _device_call(ctx, D, side, orig_flag, bins, rng2, q, lev, kde, stage_ms)


_CORNER_KEYS = ("fig", "labels", "bins", "range", "levels", "color")


def plot(vp, n_samples=int(1e5), title=None, plot_data=False, highlight_data=None, plot_vp_centres=False,
         plot_style=None, gp=None):
    """``VariationalPosterior.plot`` (:1129-1285): the corner plot of ``marginals(N=n_samples)``, drawn with matplotlib
    alone.  Returns the figure."""
    try:
        import matplotlib.pyplot as plt
    except ImportError as e:
        raise ImportError("VariationalPosterior.plot needs matplotlib; marginals() returns the numbers without it") from e
    style = dict((plot_style or {}).get("corner", {}))
    extra = sorted(k for k in style if k not in _CORNER_KEYS)
    if extra:
        _log.warning("plot: plot_style['corner'] keys ignored: %s", ", ".join(extra))
    D = vp.D
    levels = tuple(style.get("levels", (0.5, 0.9)))
    m = vp.marginals(N=n_samples, bins=style.get("bins", 40), ranges=style.get("range"), levels=levels)
    color = style.get("color", "C0")
    labels = style.get("labels") or [f"$x_{{{d}}}$" for d in range(D)]
    fig = style.get("fig") or plt.figure(figsize=(2.2 * D + 1, 2.2 * D + 1))
    axes = np.asarray(fig.subplots(D, D, squeeze=False))
    points = []  # (array in original space, marker style): data, highlighted data, component centres (:1224-1277)
    if plot_data and gp is not None:
        X = np.asarray(vp.parameter_transformer.inverse(np.asarray(gp.X)))
        points.append((X, dict(color="blue", ms=3, marker=".", ls="")))
        if highlight_data is not None and np.size(highlight_data):
            points.append((X[np.asarray(highlight_data)], dict(color="orange", ms=5, marker=".", ls="")))
    if plot_vp_centres:
        points.append((np.asarray(vp.parameter_transformer.inverse(vp.mu.T)), dict(color="red", ms=7, marker="x", ls="")))
    for i in range(D):
        for j in range(D):
            ax = axes[i, j]
            if j > i:
                ax.set_axis_off()
                continue
            if i == j:
                ax.stairs(m.density1(i), m.edges[i], color=color)
                if m.kde_density is not None:
                    ax.plot(m.kde_x[i], m.kde_density[i], color=color, lw=0.8)
                ax.set_yticks([])
            else:
                p = int(np.flatnonzero((m.pairs[:, 0] == j) & (m.pairs[:, 1] == i))[0])
                dens = m.density2(p)  # [bin of x_j, bin of x_i]
                ax.pcolormesh(m.edges[j], m.edges[i], dens.T, cmap="Greys", shading="flat")
                area = np.outer(np.diff(m.edges[j]), np.diff(m.edges[i]))[0, 0]
                cuts = sorted(set(float(c) / (m.n * area) for c in m.level_counts[p]))
                cen = lambda e: 0.5 * (e[1:] + e[:-1])
                if len(cuts) and cuts[0] > 0:
                    ax.contour(cen(m.edges[j]), cen(m.edges[i]), dens.T, levels=cuts, colors=color, linewidths=0.8)
                for X, st in points:
                    ax.plot(X[:, j], X[:, i], **st)
            if i == D - 1:
                ax.set_xlabel(labels[j])
            if j == 0 and i > 0:
                ax.set_ylabel(labels[i])
    if title is not None:
        fig.suptitle(title)
    return fig
