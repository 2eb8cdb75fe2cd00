"""GPU tests of the GP kernels on ill-conditioned posteriors (cond2(A) 1e6 .. 1e9, the regime of a real VBMC run) against
the long-double restatement of tests/gp_xprec.py: predict through the product kernel and the M <= 32 kernel, the averaged
predict, gp_log_joint with gradients and with its variance, the device-built records, a one-point append and the log
marginal likelihood.

There alpha is large and alternates in sign, so k* . alpha, z_k . alpha and sf^2 - |L^-T k*|^2 cancel heavily and a
per-term error in K* or z (a fast exp, a distance by norm expansion, a float32 intermediate) is amplified by
sum |k*| |alpha| / |mu| ~ 1e6 .. 1e7 -- which the well-conditioned cases of the other GP tests cannot see.  The float64
oracle itself misses the project's 1e-10 bounds in this regime, hence the long-double truth and the tolerance

    |device - truth| <= max(B_q, 8 e64_q)

with B_q the project's existing bound of the quantity (gp_xprec.project_bound) and e64_q the error of the reference's
own float64 arithmetic against the truth (gp_xprec.e64: the oracle's triangular solves and the device's route in NumPy).
e64 is one realisation of float64 rounding under two summation orders, not a bound; the fixed factor 8 gives the
device's own order three bits of scatter over it.  Quantities with a sample axis are checked per sample: every case
carries a well-conditioned second sample, which gets no slack from the first.

The state is installed both ways: ``upload`` (host records through vbmc_set_gp, the device forms L^-1) and ``device``
(device_posterior: covariance, factor, inverse and alpha built on the device; Cholesky cases only).  Every check prints
a table row (see gp_xprec.check); profiles/gp_illcond.md holds the rows of one run.
"""
import numpy as np
import pytest

import gp_lml_host as glh
import gp_post_host as gph
import gp_xprec as gx
from helpers import PlainVP
from test_gp_post_gpu import mirror_gp

pytestmark = pytest.mark.gpu

CHOL_NAMES = [c.name for c in gx.CASES if c.L_chol]
INSTALLS = [(n, "upload") for n in gx.NAMES] + [(n, "device") for n in CHOL_NAMES]


class RecordingLib:
    """The library handle with the names of the entry points fetched from it recorded."""

    def __init__(self, lib):
        self._lib_real, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib_real, name)


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


def installed(ctx, name, route, n_train=None):
    """The case's GP (its first ``n_train`` points) with the posterior installed by ``route``."""
    from pyvbmc_amd.gp import device_posterior

    c, d = gx.BY_NAME[name], gx.data(name)
    gp = mirror_gp(ctx, d["X"][:n_train], d["y"][:n_train], c.mean)
    if route == "upload":
        gp.update(hyp=d["hyp"])
    else:
        assert device_posterior(gp, d["hyp"], ctx=ctx) is True
    assert [bool(p.L_chol) for p in gp.posteriors] == [c.L_chol, True]
    return gp


def label(name, route):
    return f"{name} cond2 {gx.cond2(name)[0]:.1e} {route}"


def check_predict(gp, name, what):
    d = gx.data(name)
    sf2 = gx.sf2_of(d["hyp"], gx.BY_NAME[name].D)
    for M in (gx.M_QUERY, gx.M_SMALL):  # the product kernel, predict_var_small_kernel
        t, e = gx.truth_predict(name, M), gx.e64(name, M)
        fmu, fs2 = gp.predict(d["xs"][:M], separate_samples=True)
        assert fmu.shape == (M, 2) and fs2.shape == (M, 2)
        gx.check("mu", fmu, t, e, sf2, f"{what} M={M}")
        gx.check("s2", fs2, t, e, sf2, f"{what} M={M}", rel_to=np.min(t["s2"], axis=0).astype(np.float64))
    t, e = gx.truth(name), gx.e64(name)
    fmu, fs2 = gp.predict(d["xs"])
    assert fmu.shape == (gx.M_QUERY, 1) and fs2.shape == (gx.M_QUERY, 1)
    gx.check("mu_avg", fmu.ravel(), t, e, sf2, what)
    gx.check("s2_avg", fs2.ravel(), t, e, sf2, what)


@pytest.mark.parametrize("name,route", INSTALLS)
def test_predict(ctx, name, route):
    check_predict(installed(ctx, name, route), name, label(name, route))


@pytest.mark.parametrize("name,route", INSTALLS)
def test_gp_log_joint(ctx, name, route):
    from pyvbmc_amd.variational_optimization import _gp_log_joint

    c, d = gx.BY_NAME[name], gx.data(name)
    t, e, sf2, what = gx.truth(name), gx.e64(name), gx.sf2_of(d["hyp"], c.D), label(name, route)
    gp = installed(ctx, name, route)
    vp = PlainVP(d["mix"])
    G, dG, _, _, _ = _gp_log_joint(vp, gp, True, True, True, False, False)
    gx.check("G", G, t, e, sf2, what + " grad")
    for key, block in gx.split_dG(dG, c.D, d["mix"].K).items():
        gx.check(key, block, t, e, sf2, what)
    G, _, varG, _, var_ss, I_sk, J_sjk = _gp_log_joint(vp, gp, False, True, True, True, True)
    for key, val in (("G", G), ("I_sk", I_sk), ("J_sjk", J_sjk), ("varG", varG), ("var_ss", var_ss)):
        gx.check(key, val, t, e, sf2, what + " var")


def test_low_noise_case_takes_the_host_path(ctx):
    """The sn^2 < 1e-6 sample is on the non-Cholesky branch: the device build declines and update(device=True) gives
    the host path's records, bit for bit (so the ``upload`` tests above are that case's only route)."""
    from pyvbmc_amd.gp import device_posterior

    (name,) = [c.name for c in gx.CASES if not c.L_chol]
    c, d = gx.BY_NAME[name], gx.data(name)
    a, b = (mirror_gp(ctx, d["X"], d["y"], c.mean) for _ in range(2))
    a.update(hyp=d["hyp"])
    b.update(hyp=d["hyp"], device=True)
    for p, q in zip(a.posteriors, b.posteriors):
        assert np.array_equal(p.L, q.L) and np.array_equal(p.alpha, q.alpha) and np.array_equal(p.sW, q.sW)
        assert p.L_chol == q.L_chol and p.sn2_mult == q.sn2_mult
    assert [bool(p.L_chol) for p in b.posteriors] == [False, True]
    assert device_posterior(mirror_gp(ctx, d["X"], d["y"], c.mean), d["hyp"], ctx=ctx) is False


@pytest.mark.parametrize("name", CHOL_NAMES)
def test_device_built_records(ctx, name):
    """alpha and L of the device-built records against the long-double truth within 4 N eps cond2(A) of their largest
    entry, the project's derived forward-error law (gp_post_host.forward_factor)."""
    d = gx.data(name)
    gp = installed(ctx, name, "device")
    t, Ls = gx.truth(name), gx.factor_truth(name)
    for s, p in enumerate(gp.posteriors):
        f = gph.forward_factor(gx.scaled_matrix(d["hyp"][s], d["X"]))
        assert np.all(np.tril(p.L, -1) == 0.0)
        e_L = float(np.max(np.abs(p.L.astype(gx.LD) - Ls[s])) / np.max(np.abs(Ls[s])))
        e_a = float(np.max(np.abs(p.alpha.ravel().astype(gx.LD) - t["alpha"][s])) / np.max(np.abs(t["alpha"][s])))
        print(f"| {label(name, 'device')} s={s} | L, alpha (relative) | bound {f:.1e} | | {e_L:.1e} / {e_a:.1e} | "
              f"{e_L / f:.1e} / {e_a / f:.1e} |")
        assert e_L <= f and e_a <= f


def test_append_one_point(ctx):
    """129 points built on the device, the 130th appended (vbmc_gp_append), predict against the truth of the 130."""
    name = gx.APPEND_CASE
    d = gx.data(name)
    N = d["X"].shape[0]
    gp = installed(ctx, name, "device", n_train=N - 1)
    real = ctx._lib
    ctx._lib = RecordingLib(real)
    try:
        gp.append(d["X"][N - 1], d["y"][N - 1, 0])
        names = ctx._lib.names
    finally:
        ctx._lib = real
    # (extended on the device: neither rebuilt nor uploaded)
    assert "vbmc_gp_append" in names and "vbmc_gp_posterior" not in names and "vbmc_set_gp" not in names
    assert gp.X.shape[0] == N and len(gp.posteriors[0].alpha) == N
    check_predict(gp, name, label(name, "append"))


@pytest.mark.parametrize("name", CHOL_NAMES)
def test_log_marginal_likelihood(ctx, name):
    from pyvbmc_amd.gp import log_marginal_likelihood

    c, d = gx.BY_NAME[name], gx.data(name)
    refs, factors = gx.lml_reference(name)
    gp = mirror_gp(ctx, d["X"], d["y"], c.mean)
    lml, dlml = log_marginal_likelihood(gp, d["hyp"], grad=True, ctx=ctx)
    assert lml.shape == (2,) and dlml.shape == d["hyp"].shape
    for s, (ref, f) in enumerate(zip(refs, factors)):
        glh.check_within(lml[s], dlml[s], ref, f, f"{label(name, 'lml')} s={s} device vs longdouble")
