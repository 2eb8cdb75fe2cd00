"""Inputs of the marginals tests (test_marginals_host.py runs them through NumPy, test_marginals_gpu.py uploads them):
small sample sets built to hit every branch of the binning rules of pyvbmc_amd/marginals.py."""
import numpy as np

QUANTILES = (0.025, 0.16, 0.5, 0.84, 0.975)
LEVELS = (0.0, 0.5, 0.9, 1.0)

EDGE_CASES = ("on_edges", "tenths", "default_ranges", "duplicates", "constant_column", "mixed_ranges", "d1", "bins1", "n1",
              "empty_pair")


def plain_vp(D, K=2, seed=0):
    """An unbounded posterior of dimension D (no context until it is used on a device)."""
    from kde_host import mixture_params
    from pyvbmc_amd import VariationalPosterior

    state = np.random.get_state()
    vp = VariationalPosterior(D, K)  # (perturbs its means from NumPy's global stream)
    np.random.set_state(state)
    vp.mu, vp.sigma, vp.lambd, vp.w = mixture_params(D, K, seed)
    vp.eta = np.log(vp.w)
    return vp


def _resolve(x, ranges):
    out = []
    for d in range(x.shape[1]):
        r = None if ranges is None else ranges[d]
        if r is None:
            lo, hi = float(x[:, d].min()), float(x[:, d].max())
            r = (lo - 0.5, hi + 0.5) if lo == hi else (lo, hi)
        out.append((float(r[0]), float(r[1])))
    return out


def edge_case(name):
    """``(x, bins, ranges, resolved)``: samples (n, D), the bins and ranges arguments, and the (lo, hi) per dimension
    that the ranges rule gives."""
    r = np.random.RandomState(sum(map(ord, name)))
    if name == "on_edges":
        # every edge of both dimensions, the points one ulp to either side of each, hi itself, values just outside
        bins, ranges = 10, np.array([[0.0, 1.0], [-2.0, 3.0]])
        cols = []
        for lo, hi in ranges:
            e = np.linspace(lo, hi, bins + 1)
            cols.append(np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), [hi, hi, lo],
                                        [lo - 1e-9, hi + 1e-9, lo - 5.0, hi + 5.0]]))
        x = np.stack([cols[0], r.permutation(cols[1])], axis=1)
    elif name == "tenths":
        # k / 10 and k * 0.1 against linspace(0, 1, 11): the scaled position lands on either side of the edge
        bins, ranges = 10, [(0.0, 1.0), (0.0, 0.7)]
        k = np.arange(0, 11)
        a = np.concatenate([k / 10.0, k * 0.1, 1.0 - k * 0.1])
        x = np.stack([a, r.permutation(a) * 0.7], axis=1)
    elif name == "default_ranges":
        bins, ranges = 7, None
        x = r.randn(501, 3) * np.array([1.0, 20.0, 1e-3]) + np.array([0.0, 100.0, -5.0])
    elif name == "duplicates":
        bins, ranges = 5, None
        x = r.randint(0, 4, size=(300, 3)).astype(np.float64)  # four distinct values a column, min and max repeated
    elif name == "constant_column":
        bins, ranges = 6, None
        x = r.randn(77, 3)
        x[:, 1] = 2.5
    elif name == "mixed_ranges":
        bins, ranges = 9, [None, (-0.5, 0.75), None]
        x = r.randn(400, 3)
    elif name == "d1":
        bins, ranges = 5, None
        x = r.rand(65, 1)
    elif name == "bins1":
        bins, ranges = 1, [(-1.0, 1.0), None]
        x = r.randn(130, 2)
    elif name == "n1":
        bins, ranges = 4, None
        x = np.array([[0.25, -3.0, 1e6]])
    elif name == "empty_pair":
        bins, ranges = 3, [(10.0, 11.0), None, None]  # no sample of dimension 0 inside: pairs (0, 1), (0, 2) are empty
        x = r.randn(64, 3)
    else:
        raise KeyError(name)
    x = np.ascontiguousarray(x, dtype=np.float64)
    return x, bins, ranges, _resolve(x, ranges)
