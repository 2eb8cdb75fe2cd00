"""The native repeat lane of ``_neg_elcbo`` (pyvbmc_amd/csrc/pyext_step.cpp) on the device: the scenario list of
tests/test_fast_path.py (something changed between every two evaluations), once with the native ``call`` and once with
``call`` bound to the Python statement ``_call_py`` -- values, gradients and every side effect bit for bit -- and three
repeats at the headline's D and K.
"""
import numpy as np
import pytest
from helpers import PlainGP, PlainVP, oracle_gp

from pyvbmc_amd import synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyvbmc_amd import _lib

    c = _lib.Context(0)
    _lib.set_default_context(c)
    yield c
    _lib.set_default_context(None)
    c.close()


class lane:
    """``_FastElbo.call`` bound to the native method or to ``_call_py`` for the block, counting the calls that returned a
    result (``hits``) and, of those, the ones that never entered ``_call_py`` (``native_hits``)."""

    def __init__(self, native):
        self.native, self.hits, self.native_hits, self.py_calls = native, 0, 0, 0

    def __enter__(self):
        from pyvbmc_amd import variational_optimization as vo

        assert vo._step_native is not None, "pyvbmc_amd/_step_native*.so is not built (python -m pyvbmc_amd.build)"
        self.vo = vo
        self.saved = (vo._FastElbo.__dict__.get("call"), vo._FastElbo._call_py)
        native_call, call_py = vo._step_native.FastElboBase.call, vo._FastElbo._call_py
        me = self

        def counted_py(rec, theta, seed):
            me.py_calls += 1
            return call_py(rec, theta, seed)

        def counting(rec, theta, seed):
            before = me.py_calls
            r = native_call(rec, theta, seed) if me.native else counted_py(rec, theta, seed)
            me.hits += r is not None
            me.native_hits += r is not None and me.py_calls == before
            return r

        vo._FastElbo._call_py = counted_py
        vo._FastElbo.call = counting
        vo._fast_last[0] = None
        return self

    def __exit__(self, *exc):
        vo = self.vo
        if self.saved[0] is None:
            del vo._FastElbo.call
        else:
            vo._FastElbo.call = self.saved[0]
        vo._FastElbo._call_py = self.saved[1]
        vo._fast_last[0] = None


def scenario(g):
    """A sequence of fused evaluations with something changed between every two of them (tests/test_fast_path.py)."""
    from pyvbmc_amd import variational_optimization as vo

    wl = synthetic.make_workload(1, S=1)
    bnd = synthetic.default_theta_bnd(wl)
    gp = PlainGP(oracle_gp(g, g["hyp"][:1]))
    vp = PlainVP(g)
    th0 = g["theta_out"].copy()
    out = []

    def ev(theta, Ns=40, b=bnd, v=None, gpo=None, seed=None, cg=True):
        v = vp if v is None else v
        th = theta.copy()
        r = vo._neg_elcbo(th, gp if gpo is None else gpo, v, 0.0, Ns, cg, False, b, rng="philox", seed=seed)
        out.append((r[0], None if r[1] is None else r[1].copy(), r[2], r[3], th.copy(), v.mu.copy(), v.sigma.copy(),
                    v.lambd.copy(), v.w.copy(), v.eta.copy()))

    for i in range(4):  # plain repeats: calls 2.. take the repeat path
        ev(th0 + 1e-3 * i, seed=11 + i)
    bnd["lb"][0] += 0.25  # bounds edited in place: same array object, the pointer sees it
    ev(th0, seed=3)
    bnd["ub"] = bnd["ub"] - 0.5  # entry rebound
    ev(th0, seed=3)
    bnd["tol_con"] = 0.02  # scalars changed
    bnd["weight_penalty"] = 0.3
    ev(th0, seed=3)
    ev(th0, seed=3, b=None)  # no bounds
    ev(th0, seed=3, b=None)
    ev(th0, seed=3)  # and back
    vp.optimize_lambd = False  # an optimise flag flipped: a shorter theta and another mask
    K, D = vp.K, vp.D
    th_short = np.concatenate([th0[: D * K + K], th0[D * K + K + D:]])
    ev(th_short, seed=4)
    ev(th_short, seed=4)
    vp.optimize_lambd = True
    ev(th0, seed=4)
    ev(th0, Ns=80, seed=4)  # another sample count
    ev(th0, Ns=80, seed=5)
    ev(th0, Ns=0)  # the lower-bound entropy
    ev(th0, Ns=0)
    ev(th0, seed=6, cg=False)  # value only
    ev(th0, seed=6, cg=False)
    vp2 = PlainVP(g)  # another vp object
    ev(th0, seed=7, v=vp2)
    ev(th0, seed=7, v=vp)
    gp.posteriors[0].alpha[3, 0] *= 1.0 + 1e-3  # GP edited in place (interior element): the library's checksum
    ev(th0, seed=8)
    gp.posteriors[0].alpha = gp.posteriors[0].alpha * (1.0 - 1e-3)  # GP record's array rebound
    ev(th0, seed=8)
    gp2 = PlainGP(oracle_gp(g, g["hyp"][:1]))  # another GP object
    ev(th0, seed=8, gpo=gp2)
    ev(th0, seed=8, gpo=gp2)
    ev(th0)  # seeds from the context's own sequence
    ev(th0)
    return out


def test_native_lane_is_the_python_method_bit_for_bit(ctx, golden):
    from pyvbmc_amd.entropy import philox_seed

    g = golden("c1")
    runs = {}
    for native in (False, True):
        # the context's seed sequence advances with every unseeded call: start both runs from the same point
        np.random.seed(5)
        ctx.__dict__.pop("_philox_seq", None)
        with lane(native) as ln:
            runs[native] = (scenario(g), ln)
    (py, ln_py), (nat, ln_nat) = runs[False], runs[True]
    assert ln_py.native_hits == 0 and ln_py.hits >= 10
    assert ln_nat.native_hits >= 10, (ln_nat.native_hits, ln_nat.hits)  # the repeats really took the native lane
    assert ln_nat.hits == ln_py.hits
    assert len(py) == len(nat)
    for i, (a, b) in enumerate(zip(py, nat)):
        for x, y in zip(a, b):
            if x is None:
                assert y is None
            else:
                assert np.array_equal(np.asarray(x), np.asarray(y)), f"evaluation {i} differs"
    assert len({r[0] for r in nat}) >= 10  # the sequence is not constant (the changes were seen at all)
    philox_seed(ctx)


def test_headline_shape_three_repeats_on_each_lane(ctx):
    """D = 10, K = 50 (the headline's mixture and GP), 128 samples per component."""
    from pyvbmc_amd import VariationalPosterior
    from pyvbmc_amd import gp as gpm
    from pyvbmc_amd import variational_optimization as vo

    wl = synthetic.make_workload(3, Ns_total=50 * 128)
    assert (wl.D, wl.K, wl.NsK) == (10, 50, 128)
    bnd = synthetic.default_theta_bnd(wl)
    gp = gpm.GP(wl.D, gpm.SquaredExponential(), gpm.NegativeQuadratic(), gpm.GaussianNoise(constant_add=True))
    gp.update(X_new=wl.X, y_new=wl.y, hyp=wl.hyp)
    out = {}
    for native in (False, True):
        vp = VariationalPosterior(wl.D, wl.K)
        with lane(native) as ln:
            res = []
            for i in range(4):  # the first call makes the record, three repeats follow
                th = wl.theta + 1e-3 * i
                r = vo._neg_elcbo(th, gp, vp, 0.0, wl.NsK, True, False, bnd, rng="philox", seed=20 + i)
                res.append((r[0], r[1], r[2], r[3], r[4], th, vp.mu.copy(), vp.sigma.copy(), vp.lambd.copy(),
                            vp.w.copy(), vp.eta.copy()))
            assert ln.hits == 3 and ln.native_hits == (3 if native else 0)
        out[native] = res
    for a, b in zip(out[False], out[True]):
        for x, y in zip(a, b):
            assert type(x) is type(y) and np.array_equal(np.asarray(x), np.asarray(y))
    assert len({r[0] for r in out[True]}) == 4
