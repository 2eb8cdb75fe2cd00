"""CPU tests of VariationalPosterior.mtv / pyvbmc_amd.stats.kde_1d: argument errors raised before a device is
touched, the host-only context, and tests/kde_host.py's restatement against the reference's stored outputs
(tests/golden/kde_mtv.npz, tools/make_mtv_golden.py)."""
from pathlib import Path

import numpy as np
import pytest

import kde_host

GOLDEN = Path(__file__).resolve().parent / "golden" / "kde_mtv.npz"


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _no_device(monkeypatch):
    """Any attempt to reach the library's context fails the test."""
    from pyvbmc_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_lib, "default_context", boom)
    monkeypatch.setattr(_lib, "Context", boom)


def test_mtv_needs_vp2_or_samples(monkeypatch):
    from pyvbmc_amd import VariationalPosterior

    vp = VariationalPosterior(2, 2)
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="vp2 or samples"):
        vp.mtv()


@pytest.mark.parametrize("kw", [dict(n=0), dict(n=-4), dict(lower_bound=2.0, upper_bound=1.0),
                                dict(lower_bound=np.array([3.0]), upper_bound=np.array([0.0]))])
def test_kde_argument_errors_touch_no_device(monkeypatch, kw):
    from pyvbmc_amd.stats import kde_1d

    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        kde_1d(np.arange(10.0), **kw)


def test_host_only_context_is_a_loud_failure():
    from pyvbmc_amd import VariationalPosterior, _lib
    from pyvbmc_amd.stats import kde_1d

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    h = _lib.Context(-1)
    with pytest.raises(_lib.NoDeviceError):
        kde_1d(np.random.RandomState(0).randn(100), ctx=h)
    vp = VariationalPosterior(2, 2)
    vp.ctx = h
    with pytest.raises(_lib.NoDeviceError):
        vp.mtv(samples=np.random.RandomState(1).randn(50, 2), N=100)
    h.close()


@pytest.mark.parametrize("name", list(kde_host.KDE_CASES))
def test_kde_restatement_matches_the_reference(golden, name):
    n, lo, hi = kde_host.KDE_CASES[name]
    dens, mesh, bw, scott, nu = kde_host.kde_1d_host(kde_host.kde_samples(name), n, lo, hi)
    assert nu == int(golden[f"kde_{name}_nunique"])
    assert scott == bool(golden[f"kde_{name}_scott"])
    assert abs(bw - golden[f"kde_{name}_bandwidth"][0]) <= 1e-12 * abs(golden[f"kde_{name}_bandwidth"][0])
    ref = golden[f"kde_{name}_density"]
    got = dens if name in kde_host.FULL_DENSITY else dens[::16]
    assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(ref)
    np.testing.assert_array_equal(np.array([mesh[0], mesh[1], mesh[-1]]), golden[f"kde_{name}_mesh_ends"])


def test_fixture_branches(golden):
    """The fixture covers both bandwidth branches and the reference's IndexError on a constant column."""
    assert golden["kde_three_scott"] == 1 and golden["kde_zeros_ones_scott"] == 1
    assert golden["kde_gauss_scott"] == 0
    assert golden["kde_rounded_nunique"] < 1000
    assert golden["kde_constant_raises"] == 1


def golden_vp(g, name, side):
    """The mirror's posterior of side 1 / 2 of mtv case ``name`` (transformer from the stored fields)."""
    from pyvbmc_amd import VariationalPosterior
    from transform_host import RefShapedTransformer

    D, K = kde_host.mtv_case(name)[:2]
    p = f"mtv_{name}_pt{side}_"
    pt = None
    if not int(g[p + "identity"]):
        R, s = g[p + "R"], g[p + "scale"]
        pt = RefShapedTransformer(g[p + "type"], g[p + "lb"], g[p + "ub"], g[p + "mu"], g[p + "delta"],
                                  R if R.size else None, s if s.size else None)
    state = np.random.get_state()
    vp = VariationalPosterior(D, K, parameter_transformer=pt)
    np.random.set_state(state)
    v = g[f"mtv_{name}_vp{side}"]
    vp.mu = v[: D * K].reshape(D, K)
    vp.sigma = v[D * K: D * K + K].reshape(1, K)
    vp.lambd = v[D * K + K: D * K + K + D].reshape(D, 1)
    vp.w = v[D * K + K + D:].reshape(1, K)
    return vp


def mtv_inputs(g, name, sample):
    """The two sample sets and bounds of mtv case ``name``, drawn as the reference draws them: seed, then
    ``sample(vp1)`` and ``sample(vp2)`` (or the stored recipe's samples)."""
    D, K, N, spec1, spec2, rows = kde_host.mtv_case(name)
    vp1 = golden_vp(g, name, 1)
    seed = int(g[f"mtv_{name}_seed"])
    lb1, ub1 = g[f"mtv_{name}_pt1_lb"], g[f"mtv_{name}_pt1_ub"]
    if rows:
        xx2 = np.random.RandomState(seed + 5).randn(rows, D) * 1.3 + 0.2
        np.random.seed(seed)
        xx1 = sample(vp1, N)
        return vp1, None, xx1, xx2, lb1, ub1, np.full(D, -np.inf), np.full(D, np.inf)
    vp2 = golden_vp(g, name, 2)
    np.random.seed(seed)
    xx1 = sample(vp1, N)
    xx2 = sample(vp2, N)
    return vp1, vp2, xx1, xx2, lb1, ub1, g[f"mtv_{name}_pt2_lb"], g[f"mtv_{name}_pt2_ub"]


@pytest.mark.parametrize("name", [n for n in kde_host.MTV_CASES if n != "d32"])
def test_mtv_restatement_matches_the_reference(golden, name, monkeypatch):
    monkeypatch.setenv("VBMC_HIP_TRANSFORM", "0")  # the host transformer (no device needed)
    _, _, xx1, xx2, lb1, ub1, lb2, ub2 = mtv_inputs(golden, name, lambda vp, N: vp.sample(N, True, True)[0])
    got = kde_host.mtv_host(xx1, xx2, lb1, ub1, lb2, ub2)
    np.testing.assert_allclose(got, golden[f"mtv_{name}_value"].ravel(), rtol=0, atol=1e-12)
