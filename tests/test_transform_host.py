"""CPU tests of the device transformer's host side: which objects are recognised as the reference's
``ParameterTransformer`` (pyvbmc_amd/transformer.py), the library's checks of a descriptor on a
host-only context, and the internal consistency of tests/golden/transform.npz and transform_wide.npz (where
the restatement in transform_host.py is pinned at every padded width, so that the GPU tests can use it as
a second reference).  No kernel runs here."""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
from transform_host import CASES, WIDE_CASES, RefShapedTransformer

from oracle import mixture_ref
from oracle.transform_ref import BoundedLogit
from pyvbmc_amd import VariationalPosterior, _lib
from pyvbmc_amd import transformer as xf
from pyvbmc_amd.variational_posterior import IdentityTransformer


def _duck(**over):
    f = dict(type=np.array([3.0, 0.0]), lb_orig=np.array([[0.0, -np.inf]]), ub_orig=np.array([[1.0, np.inf]]),
             mu=np.zeros(2), delta=np.ones(2), R_mat=None, scale=None)
    f.update(over)
    return SimpleNamespace(**f)


def test_reference_shaped_fields_are_recognised(golden):
    g = golden("transform")
    for name in CASES:
        pt = RefShapedTransformer.from_golden(g, name)
        f = xf.transformer_fields(pt, pt.type.size)
        assert f is not None and f[0].size == pt.type.size
        assert (f[5] is None) == (pt.R_mat is None) and (f[6] is None) == (pt.scale is None)
        assert isinstance(xf.device_transformer(pt), xf.DeviceTransformer)
    assert xf.transformer_fields(_duck()) is not None


def test_other_objects_are_not_recognised():
    assert xf.transformer_fields(BoundedLogit(2, [[0.0, 0.0]], [[1.0, 1.0]])) is None  # no `type`
    assert xf.transformer_fields(IdentityTransformer(3)) is None
    assert xf.transformer_fields(None) is None
    assert xf.transformer_fields(_duck(type=np.array([4.0, 0.0]))) is None  # unknown type code
    assert xf.transformer_fields(_duck(lb_orig=np.array([[0.0]]))) is None  # field of the wrong size
    assert xf.transformer_fields(_duck(R_mat=np.eye(3))) is None
    assert xf.transformer_fields(_duck(ub_orig=np.array([[np.inf, np.inf]]))) is None  # bounded type, no bound
    assert xf.device_transformer(BoundedLogit(2)) is None
    h = _lib.Context(-1)
    try:
        for pt in (IdentityTransformer(2), BoundedLogit(2), _duck(type=np.array([4.0, 0.0])), None):
            assert xf.upload(pt, h, 0, 2) is None
    finally:
        h.close()


def test_dimension_mismatch_is_an_error():
    with pytest.raises(ValueError, match="D=2, the posterior D=3"):
        xf.transformer_fields(_duck(), 3)
    h = _lib.Context(-1)
    try:
        with pytest.raises(ValueError, match="D=2, the posterior D=3"):
            xf.upload(_duck(), h, 0, 3)
    finally:
        h.close()


def test_opt_out_keeps_every_transformer_on_the_host(monkeypatch):
    monkeypatch.setenv("VBMC_HIP_TRANSFORM", "0")
    assert xf.device_transformer(_duck()) is None
    h = _lib.Context(-1)
    try:
        assert xf.upload(_duck(), h, 0, 2) is None
    finally:
        h.close()


def test_library_checks_the_descriptor_on_a_host_only_context():
    h = _lib.Context(-1)
    try:
        assert xf.upload(_duck(), h, 0, 2) == 2 and xf.upload(_duck(), h, 1, 2) == 2
        lib, p = h._lib, _lib.ptr
        one, two = np.ones(2), np.array([0.0, 1.0])
        bad_type = np.array([5.0, 0.0])
        with pytest.raises(ValueError, match="type"):
            h.check(lib.vbmc_set_transformer(h._h, 0, 2, p(bad_type), p(two), p(one), p(two), p(one), None, None))
        with pytest.raises(ValueError, match="finite lb < ub"):  # bounded with lb == ub
            h.check(lib.vbmc_set_transformer(h._h, 0, 2, p(np.array([3.0, 3.0])), p(one), p(one), p(two), p(one),
                                             None, None))
        with pytest.raises(ValueError, match="slot"):
            h.check(lib.vbmc_set_transformer(h._h, 2, 2, p(two), p(two), p(one), p(two), p(one), None, None))
        big = np.zeros(33)
        with pytest.raises(_lib.UnsupportedShape):
            h.check(lib.vbmc_set_transformer(h._h, 0, 33, p(big), p(big), p(big), p(big), p(big), None, None))
        with pytest.raises(ValueError, match="direction"):
            h.check(lib.vbmc_transform(h._h, 1, 3, p(two), p(two)))
        # a recognised transformer never falls back to the host: no device is a loud error
        vp = VariationalPosterior(2, 2, parameter_transformer=_duck())
        vp.ctx = h
        with pytest.raises(_lib.NoDeviceError):
            vp.pdf(np.full((3, 2), 0.5))
        with pytest.raises(_lib.NoDeviceError):
            vp.sample(10, rng="philox", seed=1)
        with pytest.raises(_lib.NoDeviceError):
            vp.moments(10, cov_flag=True, rng="philox", seed=1)
        with pytest.raises(_lib.NoDeviceError):
            xf.DeviceTransformer(_duck(), h).inverse(np.zeros((4, 2)))
        assert h.check(lib.vbmc_clear_transformer(h._h, 0)) is None
        with pytest.raises(ValueError, match="slot 0 not set"):
            h.check(lib.vbmc_transform(h._h, 1, 0, p(two), p(two)))
    finally:
        h.close()


def test_numpy_stream_sampling_needs_no_device():
    """sample / moments with the default NumPy stream never needed a GPU: without one the recognised
    transformer's own inverse runs, and the values and NumPy's state are the host path's."""
    h = _lib.Context(-1)
    try:
        ref = RefShapedTransformer([12.0, 0.0], [-1.0, -np.inf], [2.0, np.inf], [0.1, 0.5], [1.5, 2.0])
        assert xf.transformer_fields(ref, 2) is not None
        vp = VariationalPosterior(2, 2, parameter_transformer=ref)
        vp.ctx = h
        np.random.seed(3)
        x, _ = vp.sample(500, orig_flag=True, balance_flag=True)
        m = vp.moments(400, orig_flag=True)
        st = np.random.get_state()
        np.random.seed(3)
        u, _ = vp.sample(500, orig_flag=False, balance_flag=True)
        x2 = vp.sample(400, orig_flag=False, balance_flag=True)[0]
        assert all(np.array_equal(a, b) for a, b in zip(st, np.random.get_state()))
        assert np.array_equal(x, ref.inverse(u)) and np.array_equal(m, np.mean(ref.inverse(x2), axis=0).reshape(1, -1))
    finally:
        h.close()


def _check_fixture(g, name):
    """One case of a transform fixture: the stored fields have the reference's shapes and types, R is
    orthogonal and the scale positive, and the restatement in transform_host.py reproduces the reference's
    forward, inverse and log|J|; forward and inverse agree."""
    pt = RefShapedTransformer.from_golden(g, name)
    D = pt.type.size
    assert pt.lb_orig.shape == (1, D) and pt.ub_orig.shape == (1, D) and pt.mu.shape == (D,) and pt.delta.shape == (D,)
    bounded = np.isfinite(pt.lb_orig[0]) & np.isfinite(pt.ub_orig[0])
    assert set(np.unique(pt.type[bounded])) <= {3.0, 12.0, 13.0} and np.all(pt.type[~bounded] == 0)
    x, u = g[f"{name}_x"], g[f"{name}_u"]
    assert x.shape[1] == D and u.shape[1] == D and g[f"{name}_ladj"].shape == (u.shape[0],)
    assert g[f"{name}_u_fwd"].shape == x.shape and g[f"{name}_x_inv"].shape == u.shape
    if pt.R_mat is not None:
        assert pt.R_mat.shape == (D, D) and pt.scale.shape == (D,)
        assert np.allclose(pt.R_mat @ pt.R_mat.T, np.eye(D), atol=1e-12) and np.all(pt.scale > 0)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for mine, ref in ((pt(x), g[f"{name}_u_fwd"]), (pt.inverse(u), g[f"{name}_x_inv"]),
                          (pt.log_abs_det_jacobian(u), g[f"{name}_ladj"])):
            fin = np.isfinite(ref)
            assert np.array_equal(np.isfinite(mine), fin) and np.array_equal(mine[~fin], ref[~fin], equal_nan=True)
            assert np.allclose(mine[fin], ref[fin], rtol=1e-13, atol=1e-13)
    back = pt.inverse(g[f"{name}_u_fwd"][:24])  # (the first 24 points: random, inside the bounds)
    assert np.allclose(back, x[:24], rtol=1e-6, atol=1e-6)
    return pt


def test_fixture_is_consistent(golden):
    """transform.npz: the restatement in transform_host.py reproduces the reference's stored outputs,
    forward and inverse agree, and the stored fields have the reference's shapes."""
    g = golden("transform")
    assert tuple(g["cases"]) == CASES
    for name in CASES:
        pt = _check_fixture(g, name)
        for df in ("0", "7"):
            y, ly = g[f"{name}_pdf_df{df}"], g[f"{name}_logpdf_df{df}"]
            xp = g[f"{name}_pdf_x"]
            m = np.all(xp > pt.lb_orig, axis=1) & np.all(xp < pt.ub_orig, axis=1)
            assert y.shape == (xp.shape[0], 1) and np.all(y[~m] == 0) and np.all(np.isneginf(ly[~m]))
            # (near the bounds the linear density under- or overflows, or passes through a subnormal exp(log|J|))
            pos = m & (y[:, 0] > 1e-200) & (y[:, 0] < 1e200)
            assert np.allclose(np.log(y[pos]), ly[pos], rtol=1e-12, atol=1e-9) and pos.sum() >= 5


def _host_pdf_orig(g, name, pt, xp, df, log_flag=False, grad_flag=False):
    """pdf(orig_flag=True) on the host: the reference's steps with transform_host.py's transformer and the
    oracle's transformed-space density (oracle/mixture_ref.py)."""
    mix = mixture_ref.Mixture.make(g[f"{name}_vp_mu"], g[f"{name}_vp_sigma"], g[f"{name}_vp_lambd"],
                                   g[f"{name}_vp_w"])
    m = np.all(xp > pt.lb_orig, axis=1) & np.all(xp < pt.ub_orig, axis=1)
    x = xp.copy()
    x[m] = pt(x[m])
    out = mixture_ref.pdf(mix, x, log_flag=log_flag, grad_flag=grad_flag, df=df)
    y, dy = out if grad_flag else (out, None)
    y[~m] = -np.inf if log_flag else 0.0
    lj = pt.log_abs_det_jacobian(x[m])[:, None]
    if log_flag:
        y[m] -= lj
    else:
        y[m] /= np.exp(lj)
    return (y, dy) if grad_flag else y


@pytest.mark.parametrize("name", WIDE_CASES)
def test_wide_fixture_is_consistent(golden, name):
    """transform_wide.npz, every padded width 2 .. 32 and both sides of the pairwise sum's switch at D = 8:
    the checks of transform.npz, and the host's orig-space pdf (transform_host.py's transformer, the oracle's
    density) reproduces the reference's, bounds, 1e308 / 1e200 coordinates and gradient rows included."""
    g = golden("transform_wide")
    assert tuple(g["cases"]) == WIDE_CASES
    pt = _check_fixture(g, name)
    D = pt.type.size
    assert D == int(name[1:])
    bounded = pt.type != 0
    if D >= 8:  # the bounded types are spread over the wide cases
        assert bounded.sum() >= 5 and (~bounded).sum() >= 2
    xp = g[f"{name}_pdf_x"]
    assert xp.shape[1] == D and np.all(np.isfinite(xp))
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for df in ("0", "7"):
            y, ly = g[f"{name}_pdf_df{df}"], g[f"{name}_logpdf_df{df}"]
            assert y.shape == (xp.shape[0], 1) and ly.shape == y.shape
            for mine, ref in ((_host_pdf_orig(g, name, pt, xp, float(df)), y),
                              (_host_pdf_orig(g, name, pt, xp, float(df), log_flag=True), ly)):
                fin = np.isfinite(ref)
                assert np.array_equal(mine[~fin], ref[~fin], equal_nan=True)
                assert np.allclose(mine[fin], ref[fin], rtol=1e-12, atol=0)
            if pt.R_mat is None:  # the overflowing squared distances: exactly 0 / -inf, never NaN
                big = np.any(np.abs(xp) > 1e150, axis=1)
                assert (D == 1 or big.sum() >= 4) and np.all(y[big] == 0) and np.all(np.isneginf(ly[big]))
        if f"{name}_pdf_g" in g:
            yg, dyg = _host_pdf_orig(g, name, pt, xp, 0.0, grad_flag=True)
            assert np.allclose(yg, g[f"{name}_pdf_g"], rtol=1e-12, atol=0, equal_nan=True)
            assert np.allclose(dyg, g[f"{name}_dpdf_g"], rtol=1e-12, atol=1e-300, equal_nan=True)


def test_wide_fixture_covers_every_width(golden):
    g = golden("transform_wide")
    Ds = sorted(int(n[1:]) for n in WIDE_CASES)
    dp = [2, 4, 6, 8, 10, 12, 16, 20, 24, 32]  # the device kernels' padded widths (VBMC_DISPATCH_DP)
    assert {min(p for p in dp if p >= D) for D in Ds} == set(dp) - {4}  # (D = 3..5: transform.npz's cases)
    assert any(D < 8 for D in Ds) and any(D > 8 and D % 8 for D in Ds) and any(D % 8 == 0 and D > 8 for D in Ds)
    types = {t: [int(n[1:]) for n in WIDE_CASES if t in g[f"{n}_type"]] for t in (3.0, 12.0, 13.0)}
    assert all(max(v) >= 8 for v in types.values())
    rot = [n for n in WIDE_CASES if g[f"{n}_R"].size]
    assert "w32" in rot and 4 <= len(rot) <= 8
    assert sum(f"{n}_pdf_g" in g for n in WIDE_CASES) >= 3
    assert set(np.unique(g["w16_type"])) == {0.0, 3.0, 12.0, 13.0}  # all three bounded types in one transformer
