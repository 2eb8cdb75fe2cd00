"""``VariationalPosterior.marginals`` on the device (csrc/marginals.hip, vbmc_marginals) against its NumPy statement
(``device=False``, itself pinned to NumPy by test_marginals_host.py) on the same samples: every integer field equal,
the edges bitwise equal, the quantiles equal where (n - 1) q is an integer and within 2 ulp of the larger neighbouring
order statistic elsewhere (the interpolation is one multiply and one add; NumPy picks between two algebraically equal
forms).  Shapes: the wave (64), sort-chunk (8192) and tile boundaries in n, D up to 32, bins up to 128 -- D = 32 with
bins = 128 is the LDS plan's worst case (2 pairs a workgroup, 248 pair groups)."""
import numpy as np
import pytest
from marginals_cases import EDGE_CASES, LEVELS, QUANTILES, edge_case, plain_vp

pytestmark = pytest.mark.gpu

# (n, D, bins): every n of {1, 63, 64, 65, 8191, 8192, 8193, 100003}, D of {1, 2, 3, 10, 32}, bins of {1, 7, 40, 128}
SHAPES = [(1, 3, 7), (63, 2, 40), (64, 10, 7), (65, 1, 40), (65, 32, 1), (8191, 3, 128), (8192, 2, 1), (8192, 10, 40),
          (8193, 32, 128), (8193, 32, 40), (100003, 10, 40), (100003, 2, 128), (100003, 3, 7)]


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


def _samples(n, D, seed):
    """Columns of different scale and offset, with repeated values (the extremes among them) and a heavy tail."""
    r = np.random.RandomState(seed)
    x = r.standard_t(3, size=(n, D)) * np.exp(r.randn(D)) + 10.0 * r.randn(D)
    if n >= 8:
        x[r.randint(0, n, n // 8)] = x[r.randint(0, n, n // 8)]  # duplicate rows
        x[r.randint(0, n, 3), :] = x.max(axis=0)
        x[r.randint(0, n, 3), :] = x.min(axis=0)
    return np.ascontiguousarray(x)


def _assert_parity(dev, host, x):
    n = x.shape[0]
    assert dev.n == host.n == n
    for f in ("pairs", "counts1", "counts2", "inside1", "inside2", "level_counts"):
        a, b = getattr(dev, f), getattr(host, f)
        assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b), f
    assert dev.edges.shape == host.edges.shape and dev.edges.tobytes() == host.edges.tobytes()
    assert np.array_equal(dev.level_mass, host.level_mass, equal_nan=True)
    assert dev.quantiles.shape == host.quantiles.shape
    xs = np.sort(x, axis=0)
    for k, q in enumerate(dev.quantile_levels):
        vi = (n - 1) * q
        if vi == np.floor(vi):
            assert np.array_equal(dev.quantiles[k], host.quantiles[k]), q
        else:
            a, b = xs[int(np.floor(vi))], xs[min(int(np.floor(vi)) + 1, n - 1)]
            ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
            assert np.all(np.abs(dev.quantiles[k] - host.quantiles[k]) <= 2 * ulp), q
            assert np.all((dev.quantiles[k] >= a) & (dev.quantiles[k] <= b))


@pytest.mark.parametrize("n, D, bins", SHAPES)
def test_device_route_equals_the_host_route(ctx, n, D, bins):
    vp = plain_vp(D)
    vp.ctx = ctx
    x = _samples(n, D, 7 * n + D)
    q = QUANTILES + (0.0, 1.0, 1.0 / 3.0)
    kw = dict(samples=x, bins=bins, quantiles=q, levels=LEVELS, kde=False)
    _assert_parity(vp.marginals(**kw), vp.marginals(device=False, **kw), x)
    if D > 1 and n > 1:
        # explicit ranges that cut samples off in some dimensions, None in the others
        lo, hi = np.quantile(x, [0.1, 0.8], axis=0)
        ranges = [None if d % 3 == 2 else (lo[d], hi[d]) for d in range(D)]
        dev = vp.marginals(ranges=ranges, **kw)
        _assert_parity(dev, vp.marginals(device=False, ranges=ranges, **kw), x)
        assert dev.inside1[0] < n
    perm = np.random.RandomState(1).permutation(n)
    assert vp.marginals(**{**kw, "samples": x[perm]}) == vp.marginals(**kw)


@pytest.mark.parametrize("name", EDGE_CASES)
def test_edge_inputs_uploaded(ctx, name):
    x, bins, ranges, _ = edge_case(name)
    vp = plain_vp(x.shape[1])
    vp.ctx = ctx
    kw = dict(samples=x, bins=bins, ranges=ranges, quantiles=QUANTILES, levels=LEVELS, kde=False)
    _assert_parity(vp.marginals(**kw), vp.marginals(device=False, **kw), x)


def _posterior(kind, ctx, golden):
    if kind == "unbounded":
        vp = plain_vp(3, K=3, seed=4)
        vp.ctx = ctx
        return vp
    from pyvbmc_amd import VariationalPosterior
    from transform_host import RefShapedTransformer, golden_vp

    g = golden("transform")
    return golden_vp(VariationalPosterior, g, kind, RefShapedTransformer.from_golden(g, kind), ctx)


@pytest.mark.parametrize("orig_flag", [True, False])
@pytest.mark.parametrize("kind", ["unbounded", "probit", "roto"])
def test_own_draws_are_sample_s_draws(ctx, golden, kind, orig_flag):
    vp = _posterior(kind, ctx, golden)
    N, seed = 20001, 123
    own = vp.marginals(N, bins=24, orig_flag=orig_flag, rng="philox", seed=seed)
    x, _ = vp.sample(N, orig_flag=orig_flag, rng="philox", seed=seed)
    assert own == vp.marginals(samples=x, bins=24, orig_flag=orig_flag) and own.n == N
    # determinism: one seed, one object; another seed, other draws
    assert own == vp.marginals(N, bins=24, orig_flag=orig_flag, rng="philox", seed=seed)
    assert own != vp.marginals(N, bins=24, orig_flag=orig_flag, rng="philox", seed=seed + 1)
    _assert_parity(own, vp.marginals(samples=x, bins=24, device=False), x)


def test_kde_is_kde_1d_of_every_column(ctx):
    from pyvbmc_amd.stats import kde_1d

    x = _samples(20000, 3, 99)
    x[:, 2] = np.abs(x[:, 2])
    vp = plain_vp(3)
    vp.ctx = ctx
    ranges = [None, (float(np.quantile(x[:, 1], 0.05)), float(np.quantile(x[:, 1], 0.9))), None]
    m = vp.marginals(samples=x, ranges=ranges)
    assert m.kde_density.shape == m.kde_x.shape == (3, 2**10) and m.kde_bandwidth.shape == (3,)
    for d in range(3):
        dens, mesh, bw = kde_1d(x[:, d], 2**10, m.edges[d, 0], m.edges[d, -1], ctx=ctx)
        assert np.array_equal(m.kde_density[d], dens) and np.array_equal(m.kde_x[d], mesh)
        assert m.kde_bandwidth[d] == np.ravel(bw)[0]
        assert np.all(np.isfinite(m.kde_density[d])) and m.kde_density[d].max() > 0
    assert vp.marginals(samples=x, ranges=ranges, kde=False).kde_density is None
    # the host route with a context gets the same curves
    h = vp.marginals(samples=x, ranges=ranges, device=False, ctx=ctx)
    assert all(np.array_equal(getattr(h, f), getattr(m, f)) for f in ("kde_x", "kde_density", "kde_bandwidth"))


def test_non_finite_sample_raises_and_the_context_lives(ctx):
    vp = plain_vp(3)
    vp.ctx = ctx
    x = _samples(9000, 3, 5)
    want = vp.marginals(samples=x, bins=7)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[8500, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            vp.marginals(samples=y, bins=7)
    assert vp.marginals(samples=x, bins=7) == want
