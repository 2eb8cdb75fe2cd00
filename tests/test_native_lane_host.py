"""The native repeat lane of ``_neg_elcbo`` (pyvbmc_amd/csrc/pyext_step.cpp) against the Python statement of the same
method (``_FastElbo._call_py``), on the CPU: the C entry is a stub -- a ctypes callback that fills F, dF, G, H and the
mixture outputs from theta and returns a chosen code -- bound into the argument block before the record is made.

Two identical worlds are built for every comparison, one driven through the native ``call``, one through ``_call_py``:
results element by element with ``type()`` equal, exceptions by type and message, and what the stub was called with.
"""
import ctypes as C
import gc
import os
import subprocess
import sys
import tracemalloc
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from pyvbmc_amd import _lib
from pyvbmc_amd import variational_optimization as vo

D, K = 2, 2
N_THETA = D * K + K + D + K  # 10
STUB_T = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(_lib.ElboCall))


class VP:
    """Attribute-only stand-in for the variational posterior (what the repeat path reads and writes)."""

    def __init__(self, ctx):
        self.D, self.K = D, K
        self.mu, self.sigma, self.lambd = np.zeros((D, K)), np.ones((1, K)), np.ones((D, 1))
        self.w, self.eta = np.full((1, K), 1.0 / K), np.zeros((1, K))
        self.optimize_mu = self.optimize_sigma = self.optimize_lambd = self.optimize_weights = True
        self._ctx = ctx


class World:
    """One record of a fused call around the stub: context (host-only), vp, gp, bounds, argument block."""

    def __init__(self, mask=15, cg=True, Ns=40, with_bnd=True, ctx_arg_explicit=False, vp_cls=VP, callback=True):
        self.ctx = ctx = _lib.Context(-1)
        self.vp = vp = vp_cls(ctx)
        vp.optimize_weights = bool(mask & 8)
        rs = np.random.RandomState(3)
        self.gp = SimpleNamespace(
            X=rs.randn(6, D),
            posteriors=[SimpleNamespace(alpha=rs.randn(6, 1), hyp=rs.randn(5)) for _ in range(2)])
        self.bnd = {"lb": np.full(N_THETA, -3.0), "ub": np.full(N_THETA, 3.0), "tol_con": 1e-3,
                    "weight_threshold": 0.01, "weight_penalty": 0.1} if with_bnd else None
        self.log, self.codes, self.logging, self.callback = [], [], True, callback
        self.fc = fc = vo._FusedCall(ctx, D, K, N_THETA)
        self.stub = STUB_T(self._entry)  # held: the block is called through its address
        fc.fn = self.stub
        fc.bind_bounds(self.bnd)
        ctx.__dict__["_fused_last"] = (D, K, N_THETA, fc)
        ctx.D, ctx.K = D, K
        gp = self.gp
        ctx._gp_quick = [id(gp.posteriors), id(gp.X), gp.X.shape[0]]
        for p in gp.posteriors:
            ctx._gp_quick += (id(p), id(p.alpha), id(p.hyp))
        self.ctx_arg = ctx if ctx_arg_explicit else None
        self.rec = vo._FastElbo(self.ctx_arg, ctx, fc, vp, gp, self.bnd, Ns, cg, "philox", mask, D, K, N_THETA,
                                _lib.EPS_PHILOX)

    def _entry(self, handle, block):
        b, fc = block.contents, self.fc
        th = np.array([b.theta[i] for i in range(b.n_theta)])
        seed = b.opts.contents.seed
        if self.logging:
            self.log.append((th.copy(), seed, handle))
        b.F[0], b.G[0], b.H[0] = float(th.sum()) + seed % 97, float(th @ th), float(th[0]) - 0.5
        for i in range(b.n_theta):
            b.dF[i] = 2.0 * th[i] + i
        fc.mu[:] = th[: D * K].reshape(K, D)
        fc.sg[:], fc.lm[:] = np.exp(th[D * K: D * K + K]), np.exp(th[D * K + K: D * K + K + D])
        tail = th[-K:] - th[-K:].max()
        fc.eta[:], fc.w[:] = tail, np.exp(tail) / np.exp(tail).sum()
        fc.th[-K:] = tail
        if self.callback:
            fc._released(None)  # (what the library does once its launches are out)
        return self.codes.pop(0) if self.codes else 0

    def run(self, native, theta, seed):
        """The outcome of one call: ('ok', result) or ('raise', type, message)."""
        fn = self.rec.call if native else self.rec._call_py
        try:
            return ("ok", fn(theta, seed))
        except Exception as e:  # noqa: BLE001 -- the comparison is of type and message
            return ("raise", type(e), str(e))

    def state(self):
        v = self.vp
        return [np.array(x) for x in (v.mu, v.sigma, v.lambd, v.w, v.eta)]

    def close(self):
        self.ctx.close()


def same(a, b):
    """Element by element, types included."""
    assert type(a) is type(b), (a, b)
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            same(x, y)
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    else:
        assert a == b or (a != a and b != b), (a, b)


def same_logs(wa, wb):
    assert len(wa.log) == len(wb.log)
    for (ta, sa, _), (tb, sb, _) in zip(wa.log, wb.log):
        assert np.array_equal(ta, tb) and sa == sb


def pair(**kw):
    return World(**kw), World(**kw)


def theta0():
    return np.linspace(-0.4, 0.5, N_THETA)


def test_the_extension_is_the_repeat_path():
    assert vo._step_native is not None, "pyvbmc_amd/_step_native*.so is not built (python -m pyvbmc_amd.build)"
    assert issubclass(vo._FastElbo, vo._step_native.FastElboBase)
    assert vo._FastElbo.call is vo._step_native.FastElboBase.call


@pytest.mark.parametrize("kw", [{}, {"cg": False}, {"with_bnd": False}, {"Ns": 0}, {"ctx_arg_explicit": True},
                                {"callback": False}])
def test_plain_repeat_equals_the_python_method(kw):
    wa, wb = pair(**kw)
    try:
        for i in range(3):
            ta, tb = theta0() + 0.1 * i, theta0() + 0.1 * i
            ra, rb = wa.run(True, ta, 7 + i), wb.run(False, tb, 7 + i)
            assert ra[0] == "ok" and ra[1] is not None
            same(ra, rb)
            same(ta, tb)  # (the max-shifted eta tail of the caller's theta)
            same(wa.state(), wb.state())
            assert wa.fc.side is None and wb.fc.side is None
        assert len(wa.log) == 3 and all(h == wa.ctx._h.value for _, _, h in wa.log)
        same_logs(wa, wb)
        if kw.get("Ns", 40) == 0:  # no draws: the seed field is left alone
            assert [s for _, s, _ in wa.log] == [0, 0, 0]
        else:
            assert [s for _, s, _ in wa.log] == [7, 8, 9]
    finally:
        wa.close(), wb.close()


def test_unseeded_calls_advance_the_contexts_sequence():
    wa, wb = pair()
    try:
        for w, native in ((wa, True), (wb, False)):
            np.random.seed(5)
            for _ in range(3):
                assert w.run(native, theta0(), None)[0] == "ok"
            assert w.run(native, theta0(), 4)[0] == "ok"
            assert w.run(native, theta0(), None)[0] == "ok"
        same_logs(wa, wb)
        seeds = [s for _, s, _ in wa.log]
        assert seeds[1] == seeds[0] + 1 and seeds[2] == seeds[0] + 2 and seeds[3] == 4 and seeds[4] == seeds[0] + 3
        assert wa.ctx.__dict__["_philox_seq"][0] == wb.ctx.__dict__["_philox_seq"][0] == seeds[4]
    finally:
        wa.close(), wb.close()


def _flip(name):
    def change(w):
        setattr(w.vp, name, False)
    return change


def _set(what, name, value):
    def change(w):
        setattr(getattr(w, what), name, value)
    return change


def _bnd(key, value):
    def change(w):
        w.bnd[key] = value(w.bnd[key]) if callable(value) else value
    return change


def _fused_last_rebuilt(w):
    w.ctx.__dict__["_fused_last"] = tuple(w.ctx.__dict__["_fused_last"])[:3] + (w.fc,)


def _other_ctx(w):
    w.other = _lib.Context(-1)
    w.vp._ctx = w.other


def _posteriors_rebound(w):
    w.gp.posteriors = list(w.gp.posteriors)


def _x_rebound(w):
    w.gp.X = w.gp.X.copy()


def _x_reshaped(w):
    w.gp.X.shape = (3, 2 * D)


def _record_replaced(w):
    p = w.gp.posteriors[1]
    w.gp.posteriors[1] = SimpleNamespace(alpha=p.alpha, hyp=p.hyp)


def _alpha_rebound(w):
    w.gp.posteriors[0].alpha = w.gp.posteriors[0].alpha.copy()


def _hyp_rebound(w):
    w.gp.posteriors[1].hyp = w.gp.posteriors[1].hyp.copy()


def _posterior_added(w):
    p = w.gp.posteriors[0]
    w.gp.posteriors.append(SimpleNamespace(alpha=p.alpha, hyp=p.hyp))


def _posterior_dropped(w):
    w.gp.posteriors.pop()


def _gp_forgotten(w):
    w.ctx._gp_quick = None


def _ctx_d_deleted(w):
    del w.ctx.D


CHANGES = {
    "optimize_mu": _flip("optimize_mu"), "optimize_sigma": _flip("optimize_sigma"),
    "optimize_lambd": _flip("optimize_lambd"), "optimize_weights": _flip("optimize_weights"),
    "vp.D": _set("vp", "D", D + 1), "vp.K": _set("vp", "K", K + 1),
    "_fused_last": _fused_last_rebuilt,
    "ctx.D": _set("ctx", "D", D + 1), "ctx.K": _set("ctx", "K", K + 1), "ctx.D deleted": _ctx_d_deleted,
    "ctx_of": _other_ctx,
    "lb": _bnd("lb", np.copy), "ub": _bnd("ub", np.copy), "tol_con": _bnd("tol_con", 2e-3),
    "weight_threshold": _bnd("weight_threshold", 0.02), "weight_penalty": _bnd("weight_penalty", 0.2),
    "posteriors": _posteriors_rebound, "X": _x_rebound, "X.shape[0]": _x_reshaped, "id(p)": _record_replaced,
    "p.alpha": _alpha_rebound, "p.hyp": _hyp_rebound, "one posterior more": _posterior_added,
    "one posterior fewer": _posterior_dropped, "_gp_quick": _gp_forgotten,
}


@pytest.mark.parametrize("name", list(CHANGES))
def test_each_recheck_returns_none(name):
    wa, wb = pair()
    try:
        same(wa.run(True, theta0(), 1), wb.run(False, theta0(), 1))  # unchanged: a result
        for w, native in ((wa, True), (wb, False)):
            CHANGES[name](w)
            before = len(w.log)
            assert w.run(native, theta0(), 2) == ("ok", None), name
            assert len(w.log) == before and w.fc.side is None  # (the entry was not reached)
    finally:
        wa.close(), wb.close()


def test_fast_path_switch_is_read_at_call_time(monkeypatch):
    wa, wb = pair()
    try:
        monkeypatch.setattr(vo, "_FAST_PATH", False)
        assert wa.run(True, theta0(), 1) == wb.run(False, theta0(), 1) == ("ok", None)
        monkeypatch.setattr(vo, "_FAST_PATH", True)
        same(wa.run(True, theta0(), 1), wb.run(False, theta0(), 1))
        assert len(wa.log) == 1
    finally:
        wa.close(), wb.close()


def test_a_block_that_is_not_all_optimised_returns_none():
    wa, wb = pair(mask=7)
    try:
        assert wa.run(True, theta0(), 1) == wb.run(False, theta0(), 1) == ("ok", None)
        assert not wa.log and not wb.log
    finally:
        wa.close(), wb.close()


def test_bounds_dropped_keys_raise_alike():
    wa, wb = pair()
    try:
        for w in (wa, wb):
            del w.bnd["tol_con"]
        ra, rb = wa.run(True, theta0(), 1), wb.run(False, theta0(), 1)
        assert ra[0] == "raise" and ra[1] is KeyError
        assert ra == rb
        for w in (wa, wb):  # optional keys fall back to 0.0: another value than the record's
            w.bnd["tol_con"] = 1e-3
            del w.bnd["weight_penalty"]
        assert wa.run(True, theta0(), 1) == wb.run(False, theta0(), 1) == ("ok", None)
    finally:
        wa.close(), wb.close()


class Sub(np.ndarray):
    pass


THETAS = {
    "float32": lambda: theta0().astype(np.float32),
    "non-contiguous": lambda: np.repeat(theta0(), 2)[::2],
    "wrong length": lambda: np.zeros(N_THETA + 1),
    "two-dimensional": lambda: theta0().reshape(2, 5),
    "subclass": lambda: theta0().view(Sub),
    "list": lambda: list(theta0()),
    "unaligned": lambda: np.frombuffer(bytearray(8 * N_THETA + 1), dtype=np.float64, count=N_THETA, offset=1),
    "read-only": lambda: np.asarray(memoryview(theta0().tobytes())).view(np.float64),
}


@pytest.mark.parametrize("form", list(THETAS))
def test_other_theta_forms_take_the_python_method(form):
    wa, wb = pair()
    try:
        ta, tb = THETAS[form](), THETAS[form]()
        if form == "unaligned":
            assert not ta.flags.aligned
            ta[:], tb[:] = theta0(), theta0()
        ra, rb = wa.run(True, ta, 3), wb.run(False, tb, 3)
        assert ra[0] == rb[0]
        same(ra, rb)
        same(list(ta) if form == "list" else np.asarray(ta), list(tb) if form == "list" else np.asarray(tb))
        same(wa.state(), wb.state())
        same_logs(wa, wb)
        if form in ("wrong length", "two-dimensional"):
            assert ra[0] == "raise" and ra[1] is ValueError
        assert wa.fc.side is None and wb.fc.side is None
    finally:
        wa.close(), wb.close()


@pytest.mark.parametrize("seed", [np.int64(5), 2 ** 64 + 9, -1, 2.5, True, "7"])
def test_seed_forms(seed):
    wa, wb = pair()
    try:
        ra, rb = wa.run(True, theta0(), seed), wb.run(False, theta0(), seed)
        same(ra, rb)
        same_logs(wa, wb)
    finally:
        wa.close(), wb.close()


@pytest.mark.parametrize("codes", [[_lib.W_GP_CHANGED], [_lib.W_GP_CHANGED, _lib.E_HIP], [_lib.E_HIP], [_lib.E_ARG],
                                   [_lib.E_UNSUP]])
@pytest.mark.parametrize("callback", [True, False])
def test_return_codes_go_through_the_python_method(monkeypatch, codes, callback):
    uploads = []
    monkeypatch.setattr(vo, "upload_gp", lambda gp, ctx, lazy=False: uploads.append((gp, ctx)))
    wa, wb = pair(callback=callback)
    try:
        wa.codes, wb.codes = list(codes), list(codes)
        ra, rb = wa.run(True, theta0(), 3), wb.run(False, theta0(), 3)
        same(ra, rb)
        same_logs(wa, wb)
        n_calls = 2 if codes[0] == _lib.W_GP_CHANGED else 1
        assert len(wa.log) == n_calls
        assert uploads == ([(wa.gp, wa.ctx), (wb.gp, wb.ctx)] if n_calls == 2 else [])
        assert ra[0] == ("ok" if codes == [_lib.W_GP_CHANGED] else "raise")
        assert wa.fc.side is None and wb.fc.side is None
        same(wa.run(True, theta0(), 4), wb.run(False, theta0(), 4))  # and the record still serves
    finally:
        wa.close(), wb.close()


class Refusing(VP):
    armed = False

    def __setattr__(self, name, value):
        if name == "sigma" and Refusing.armed:
            raise RuntimeError("no")
        object.__setattr__(self, name, value)


@pytest.mark.parametrize("callback", [True, False])
def test_an_exception_in_the_release_callback_surfaces_after_the_call(callback):
    wa, wb = pair(vp_cls=Refusing, callback=callback)
    Refusing.armed = True
    try:
        ra, rb = wa.run(True, theta0(), 3), wb.run(False, theta0(), 3)
        assert ra == rb == ("raise", RuntimeError, "no")
        assert wa.fc.side is None and wb.fc.side is None
        assert len(wa.log) == len(wb.log) == 1
        Refusing.armed = False
        same(wa.run(True, theta0(), 3), wb.run(False, theta0(), 3))
    finally:
        Refusing.armed = False
        wa.close(), wb.close()


def test_the_python_only_block_is_not_bound(monkeypatch):
    """VBMC_ELBO_CALL_BLOCK=0 (the thirteen-argument entry): the native ``call`` has no address to call through and is
    the Python method."""
    w = World()
    try:
        w.fc.block_call = False
        calls = []
        rec = vo._FastElbo(None, w.ctx, w.fc, w.vp, w.gp, w.bnd, 40, True, "philox", 15, D, K, N_THETA, _lib.EPS_PHILOX)
        monkeypatch.setattr(vo._FastElbo, "_call_py", lambda self, th, seed: calls.append(seed) or "py")
        assert rec.call(theta0(), 3) == "py" and calls == [3]
    finally:
        w.close()


def test_no_leak_over_many_calls():
    w = World()
    try:
        w.logging = False
        theta = theta0()
        rec, call = w.rec, w.rec.call
        watched = (w.vp, w.gp, w.bnd, theta, rec, None, w.fc, w.ctx)
        for _ in range(200):
            call(theta, 3)
        gc.collect()
        tracemalloc.start()
        before = [sys.getrefcount(o) for o in watched]
        mem0 = tracemalloc.get_traced_memory()[0]
        for i in range(20000):
            r = call(theta, i)
        shape = r[1].shape
        del r
        after = [sys.getrefcount(o) for o in watched]  # (before anything else runs: None's count is everybody's)
        gc.collect()
        mem1 = tracemalloc.get_traced_memory()[0]
        tracemalloc.stop()
        assert shape == (N_THETA,)
        assert after == before
        # 20000 calls: one leaked float (24 bytes) per call would be 480 kB
        assert mem1 - mem0 < 16384, mem1 - mem0
        # the None outcome does not leak either
        w.vp.optimize_mu = False
        results = 0
        before = [sys.getrefcount(o) for o in watched]
        for i in range(20000):
            results += call(theta, i) is not None
        after = [sys.getrefcount(o) for o in watched]
        assert results == 0
        assert after == before
    finally:
        tracemalloc.stop()
        w.close()


def test_without_the_extension():
    """VBMC_NATIVE_LANE=0 in a fresh process: ``call`` is the Python method and the package works."""
    here = Path(__file__).resolve().parent
    code = (
        "import sys; sys.path[:0] = [%r, %r]\n"
        "import numpy as np\n"
        "import test_native_lane_host as t\n"
        "vo = t.vo\n"
        "assert vo._step_native is None\n"
        "assert vo._FastElbo.__dict__['call'] is vo._FastElbo.__dict__['_call_py']\n"
        "assert '_step_native' not in ''.join(sys.modules)\n"
        "w = t.World()\n"
        "r = w.rec.call(t.theta0(), 3)\n"
        "assert r is not None and len(w.log) == 1 and r[4] == 0 and r[1].shape == (t.N_THETA,)\n"
        "print('python lane ok', r[0])\n"
    ) % (str(here.parent), str(here))
    env = dict(os.environ, VBMC_NATIVE_LANE="0")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "python lane ok" in p.stdout
