"""``VariationalPosterior.marginals(device=False)``: the NumPy statement of the rules in pyvbmc_amd/marginals.py against
``np.histogram`` / ``np.histogram2d`` / ``np.quantile`` called directly, the levels against a brute-force loop over
thresholds, the argument errors, and ``plot`` without matplotlib.  No GPU needed; tests/marginals_cases.py holds the
inputs, which tests/test_marginals_gpu.py uploads as well."""
import pickle
import sys

import numpy as np
import pytest
from marginals_cases import EDGE_CASES, LEVELS, QUANTILES, edge_case, plain_vp


def _direct(x, bins, rng):
    """counts1, edges, counts2 from NumPy called directly with the ranges ``rng`` (a list of (lo, hi))."""
    D = x.shape[1]
    c1 = np.array([np.histogram(x[:, d], bins, range=rng[d])[0] for d in range(D)]).reshape(D, bins)
    ed = np.array([np.histogram(x[:, d], bins, range=rng[d])[1] for d in range(D)])
    pairs = [(i, j) for i in range(D) for j in range(i + 1, D)]
    c2 = np.array([np.histogram2d(x[:, i], x[:, j], bins, range=[rng[i], rng[j]])[0] for i, j in pairs])
    return c1, ed, c2.reshape(len(pairs), bins, bins).astype(np.int64), np.array(pairs, dtype=np.int64).reshape(-1, 2)


def _brute_levels(table, level):
    """Over every threshold t that occurs: the largest t whose cells (count >= t) hold >= level * total."""
    total = int(table.sum())
    best = None
    for t in np.unique(table):
        mass = int(table[table >= t].sum())
        if mass >= level * float(total) and (best is None or t > best[0]):
            best = (int(t), mass / total)
    return best


@pytest.mark.parametrize("name", EDGE_CASES)
def test_host_route_is_numpy_called_directly(name):
    x, bins, ranges, rng = edge_case(name)
    vp = plain_vp(x.shape[1])
    m = vp.marginals(samples=x, bins=bins, ranges=ranges, quantiles=QUANTILES, levels=LEVELS, device=False)
    c1, ed, c2, pairs = _direct(x, bins, rng)
    D = x.shape[1]
    P = D * (D - 1) // 2
    assert m.n == x.shape[0]
    assert m.pairs.shape == (P, 2) and np.array_equal(m.pairs, pairs)
    assert m.edges.shape == (D, bins + 1) and np.array_equal(m.edges, ed)
    assert all(np.array_equal(m.edges[d], np.linspace(rng[d][0], rng[d][1], bins + 1)) for d in range(D))
    assert m.counts1.dtype == np.int64 and m.counts1.shape == (D, bins) and np.array_equal(m.counts1, c1)
    assert m.counts2.dtype == np.int64 and m.counts2.shape == (P, bins, bins) and np.array_equal(m.counts2, c2)
    assert np.array_equal(m.inside1, c1.sum(axis=1)) and m.inside1.shape == (D,)
    assert np.array_equal(m.inside2, c2.sum(axis=(1, 2))) and m.inside2.shape == (P,)
    assert np.array_equal(m.quantiles, np.quantile(x, QUANTILES, axis=0)) and m.quantiles.shape == (len(QUANTILES), D)
    assert m.level_counts.shape == (P, len(LEVELS)) and m.level_mass.shape == (P, len(LEVELS))
    for p in range(P):
        for k, lev in enumerate(LEVELS):
            if m.inside2[p] == 0:
                assert m.level_counts[p, k] == 0 and np.isnan(m.level_mass[p, k])
                continue
            t, mass = _brute_levels(m.counts2[p], lev)
            assert (m.level_counts[p, k], m.level_mass[p, k]) == (t, mass)
            assert m.level_mass[p, k] >= lev
    if ranges is None:
        for p, (i, j) in enumerate(m.pairs):
            assert np.array_equal(m.counts2[p].sum(axis=1), m.counts1[i])
            assert np.array_equal(m.counts2[p].sum(axis=0), m.counts1[j])
    assert m.kde_density is None  # no context: the package's kde_1d is left out
    # densities integrate to the fraction inside
    for d in range(D):
        assert np.isclose(np.sum(m.density1(d) * np.diff(m.edges[d])), m.inside1[d] / m.n, rtol=1e-12)
    for p, (i, j) in enumerate(m.pairs):
        area = np.outer(np.diff(m.edges[i]), np.diff(m.edges[j]))
        assert np.isclose(np.sum(m.density2(p) * area), m.inside2[p] / m.n, rtol=1e-12)


@pytest.mark.parametrize("table, level, want", [
    ([[5, 5, 5], [5, 0, 0], [0, 0, 0]], 0.5, (5, 1.0)),      # a tie at the boundary: all four cells count
    ([[4, 3, 3], [3, 3, 0], [0, 0, 0]], 0.5, (3, 1.0)),      # 4 + 3 < 8 <= 4 + 3 + 3: the threshold 3 takes every 3
    ([[10, 1, 1], [1, 1, 1], [1, 1, 1]], 0.5, (10, 10 / 18)),
    ([[10, 2, 2], [2, 2, 2], [0, 0, 0]], 0.5, (10, 0.5)),    # the sum meets the level exactly
    ([[2, 2], [2, 2]], 0.0, (2, 1.0)),                       # the prefix is never empty
    ([[2, 2], [1, 3]], 1.0, (1, 1.0)),
    ([[7]], 0.9, (7, 1.0)),
])
def test_levels_with_ties(table, level, want):
    from pyvbmc_amd.marginals import levels_of

    table = np.array(table, dtype=np.int64)
    lc, lm = levels_of(table, [level])
    assert (int(lc[0]), float(lm[0])) == want == _brute_levels(table, level)
    assert lm[0] >= level


def test_permutation_invariance_and_pickle():
    x, bins, ranges, _ = edge_case("mixed_ranges")
    vp = plain_vp(x.shape[1])
    a = vp.marginals(samples=x, bins=bins, ranges=ranges, device=False)
    b = vp.marginals(samples=x[np.random.RandomState(0).permutation(len(x))], bins=bins, ranges=ranges, device=False)
    assert a == b
    c = pickle.loads(pickle.dumps(a))
    assert type(c) is type(a) and c == a and c.n == a.n
    b.counts1[0, 0] += 1
    assert a != b
    text = repr(a).splitlines()
    assert len(text) == 1 + x.shape[1] and all(f"x[{d}]" in text[1 + d] for d in range(x.shape[1]))
    med, lo, hi = a.quantiles[2, 0], a.quantiles[0, 0], a.quantiles[4, 0]
    assert f"{med: .6g}" in text[1] and f"{lo: .6g}" in text[1] and f"{hi: .6g}" in text[1]


def test_own_draws_on_the_host():
    """samples=None, device=False: the draws of sample(N, orig_flag, rng="numpy") from NumPy's stream."""
    vp = plain_vp(3)
    np.random.seed(11)
    m = vp.marginals(N=500, bins=7, device=False, orig_flag=False)
    np.random.seed(11)
    x, _ = vp.sample(500, orig_flag=False)
    assert m == vp.marginals(samples=x, bins=7, device=False) and m.n == 500


@pytest.fixture
def no_context(monkeypatch):
    from pyvbmc_amd import _lib

    made = []
    monkeypatch.setattr(_lib, "default_context", lambda: made.append(1) or pytest.fail("a context was made"))
    yield
    assert not made


@pytest.mark.parametrize("device", [True, False])
def test_argument_errors_touch_no_device(no_context, device):
    from pyvbmc_amd import _lib

    vp = plain_vp(2)
    x = np.random.RandomState(1).randn(50, 2)
    kw = dict(samples=x, device=device)
    for bad in (dict(samples=x[:, :1]), dict(samples=x.ravel()), dict(samples=np.zeros((0, 2))), dict(levels=(0.5, 1.5)),
                dict(levels=(-0.1,)), dict(quantiles=(0.5, 1.0001)), dict(quantiles=(np.nan,)), dict(bins=0), dict(bins=-3),
                dict(ranges=[(1.0, 1.0), None]), dict(ranges=[(2.0, 1.0), None]), dict(ranges=np.array([[0.0, 1.0]])),
                dict(ranges=[None]), dict(ranges=[(0.0, np.inf), None]), dict(samples=None, N=0)):
        with pytest.raises(ValueError):
            vp.marginals(**{**kw, **bad})
    for bad in (dict(bins=129), dict(samples=None, N=2**22 + 1)):
        with pytest.raises(_lib.UnsupportedShape):
            vp.marginals(**{**kw, **bad})
    with pytest.raises(_lib.UnsupportedShape):
        plain_vp(33).marginals(samples=np.zeros((4, 33)), device=device)
    if not device:
        with pytest.raises(ValueError):
            vp.marginals(samples=np.array([[0.0, np.nan], [1.0, 2.0]]), device=False)


def test_plot_without_matplotlib_raises_before_sampling(monkeypatch, no_context):
    vp = plain_vp(2)
    for name in [k for k in sys.modules if k == "matplotlib" or k.startswith("matplotlib.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "matplotlib", None)
    monkeypatch.setitem(sys.modules, "matplotlib.pyplot", None)
    monkeypatch.setattr(vp, "sample", lambda *a, **k: pytest.fail("sampled"))
    monkeypatch.setattr(vp, "marginals", lambda *a, **k: pytest.fail("marginals called"))
    with pytest.raises(ImportError, match="matplotlib") as e:
        vp.plot()
    assert "\n" not in str(e.value)


def test_plot_draws_a_corner(monkeypatch):
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import logging

    vp = plain_vp(3)
    real = vp.marginals
    # (the drawing is under test: the numbers come from the host route, which needs no device)
    monkeypatch.setattr(vp, "marginals", lambda **k: real(**{**k, "device": False, "orig_flag": False}))
    np.random.seed(3)
    seen = []
    handler = logging.Handler()
    handler.emit = seen.append
    logging.getLogger("pyvbmc_amd.marginals").addHandler(handler)
    try:
        fig = vp.plot(n_samples=2000, title="t", plot_vp_centres=True,
                      plot_style={"corner": {"bins": 12, "labels": ["a", "b", "c"], "levels": (0.5,), "smooth": 1.0}})
    finally:
        logging.getLogger("pyvbmc_amd.marginals").removeHandler(handler)
    assert len(fig.axes) == 9
    assert len(seen) == 1 and "smooth" in seen[0].getMessage()
    assert fig.axes[6].get_xlabel() == "a" and fig.axes[3].get_ylabel() == "b"
    import matplotlib.pyplot as plt

    plt.close(fig)
