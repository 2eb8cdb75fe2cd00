"""The sieve's host side without a GPU: tests/sieve_host.py against the reference's recorded arrays
(tests/golden/sieve.npz, tools/make_sieve_golden.py) bit for bit, the package's own host generation
(pyvbmc_amd/sieve.py, ``device=False``) against that statement, ``get_hpd``, the refusals and ``patch_sieve``.

Bounds.  Fixture against statement: ``np.array_equal`` (the same NumPy calls on the same operands).  The package's
vectorised host generation against the statement: both are float64 NumPy; they differ in the order of a few products, in
one normalisation of ``w`` (the reference divides by the sum in the jitter and again in ``get_parameters``) and in
``np.var`` / ``np.sum`` over at most max(D, K_new) <= 5 terms.  Longest chain (a spawned component's mean): 8 roundings of
summands of size at most A = max(1, |inputs|) (1 + 2 |z|) with |z| < 8.6 for a 53-bit Box-Muller draw and < 6 for the
fixture's MT19937 draws; a log entry: at most 12 roundings of its argument.  16 eps A max(1, |theta|) covers both.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import sieve_host as sh

from pyvbmc_amd import VariationalPosterior, _lib, dropin
from pyvbmc_amd import sieve as sv

EPS = np.finfo(np.float64).eps
ATTRS = ("mu", "sigma", "lambd", "w", "eta")


@pytest.fixture(scope="module")
def z():
    return np.load(sh.GOLDEN, allow_pickle=False)


def names():
    return sh.case_names(np.load(sh.GOLDEN, allow_pickle=False))


def package_vp(c, ctx=None):
    D, K = (int(v) for v in c["shape"][:2])
    vp = VariationalPosterior(D, K)
    for a in ATTRS:
        setattr(vp, a, np.array(c["base_" + a]))
    vp.optimize_mu, vp.optimize_sigma, vp.optimize_lambd, vp.optimize_weights = (bool(f) for f in c["flags"])
    if ctx is not None:
        vp.ctx = ctx
    return vp


def stars(c):
    return sh.get_hpd(c["X"], c["y"], sh.options_of(c)["hpd_frac"])[:2]


def state_equal(st, c):
    return (st[0] == "MT19937" and np.array_equal(st[1], c["mt_key"]) and st[2] == int(c["mt_pos"])
            and st[3] == int(c["mt_has_gauss"]) and (st[3] == 0 or st[4] == float(c["mt_gauss"])))


@pytest.mark.parametrize("name", names())
def test_statement_equals_the_reference_bit_for_bit(z, name):
    c = sh.load_case(z, name)
    D, K, Kn, N, init_N, best_N = (int(v) for v in c["shape"])
    X_star, y_star = stars(c)
    assert X_star.shape[0] == round(0.8 * N)
    np.random.seed(int(c["seed"]))
    raw, thetas, fin, types = sh.candidates_host(sh.base_of(c), c["flags"], sh.split(init_N, best_N), Kn, X_star, y_star,
                                                 sh.NumpySource())
    st = np.random.get_state(legacy=True)
    assert len(raw) == len(c["F"])
    for a in ATTRS:
        assert np.array_equal(np.stack([r[a] for r in raw]), c["raw_" + a]), ("raw", a)
        assert np.array_equal(np.stack([f[a] for f in fin]), c["fin_" + a]), ("fin", a)
    assert np.array_equal(thetas, c["thetas"])
    assert np.array_equal(types, c["types"])
    assert state_equal(st, c)


def amplitude(c, zmax):
    return max(1.0, float(np.max(np.abs(c["X"]))), float(np.max(np.abs(c["base_mu"])))) * (1.0 + 2.0 * zmax)


@pytest.mark.parametrize("name", names())
def test_package_host_generation_numpy(z, name):
    c = sh.load_case(z, name)
    Kn, init_N, best_N = int(c["shape"][2]), int(c["shape"][4]), int(c["shape"][5])
    X_star, y_star = stars(c)
    vp = package_vp(c)  # (its constructor draws from NumPy's stream)
    np.random.seed(int(c["seed"]))
    cand = sv._generate(vp, sh.split(init_N, best_N), Kn, X_star, y_star, "numpy", None, False, None)
    assert state_equal(np.random.get_state(legacy=True), c)
    assert np.array_equal(cand.types, c["types"])
    err = np.abs(cand.thetas - c["thetas"]) / np.maximum(1.0, np.abs(c["thetas"]))
    assert err.max() <= 16 * EPS * amplitude(c, 6.0), err.max() / EPS


@pytest.mark.parametrize("name", [n for n in names() if n.endswith("_7")])
def test_package_host_generation_philox(z, name):
    c = sh.load_case(z, name)
    D, K, Kn, init_N, best_N = (int(c["shape"][i]) for i in (0, 1, 2, 4, 5))
    X_star, y_star = stars(c)
    counts = sh.split(init_N, best_N)
    seed = 0x1234567 + int(c["seed"])
    _, want, _, _ = sh.candidates_host(sh.base_of(c), c["flags"], counts, Kn, X_star, y_star, sh.PhiloxSource(seed, D, K, Kn))
    vp = package_vp(c)
    st = np.random.get_state(legacy=True)
    cand = sv._generate(vp, counts, Kn, X_star, y_star, "philox", seed, False, None)
    st1 = np.random.get_state(legacy=True)
    assert np.array_equal(st[1], st1[1]) and st[2] == st1[2]  # a given seed: NumPy's global stream is not touched
    err = np.abs(cand.thetas - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= 16 * EPS * amplitude(c, 8.6), err.max() / EPS


def test_get_hpd_equals_the_reference(z):
    for i in range(3):
        got = sv.get_hpd(z[f"hpd{i}_X"], z[f"hpd{i}_y"], float(z[f"hpd{i}_frac"]))
        for g, k in zip(got, ("hX", "hy", "range", "idx")):
            assert np.array_equal(g, z[f"hpd{i}_{k}"], equal_nan=True), (i, k)
    assert z["hpd2_idx"].size == 0 and np.all(np.isnan(z["hpd2_range"]))  # the hpd_N = 0 case is among them


def test_to_vps_objects_and_selection_idioms(z):
    c = sh.load_case(z, "d2k2n4_all_7")
    X_star, y_star = stars(c)
    vp = package_vp(c)
    np.random.seed(int(c["seed"]))
    cand = sv._generate(vp, (3, 3, 1), 4, X_star, y_star, "numpy", None, False, None)
    vps = cand.to_vps()
    assert vps.dtype == object and vps.shape == (7,)
    for b, v in enumerate(vps):
        assert v.K == 4 and v.bounds is None and v.stats is None and v.parameter_transformer is vp.parameter_transformer
        assert v.mu is not vps[(b + 1) % 7].mu and v.mu.shape == (2, 4) and v.sigma.shape == (1, 4) and v.lambd.shape == (2, 1)
        th = v.get_parameters()
        th[-4:] -= np.amax(th[-4:])
        # exp then log of an entry, twice the renormalisation by nl = 1 + O(D eps): (4 + D) eps max(1, |theta|)
        assert np.all(np.abs(th - cand.thetas[b]) <= (4 + 2) * EPS * np.maximum(1.0, np.abs(cand.thetas[b])))
    assert vp.K == 2 and vp.mu.shape == (2, 2)  # the base is untouched
    # optimize_vp's idioms (:189-199): the first candidate of a type, indexing, np.delete
    types = cand.types
    idx = np.where(types == 2)[0][0]
    assert idx == 3 and vps[idx].K == 4
    assert np.delete(vps, idx).shape == (6,) and np.delete(types, idx).shape == (6,)


# ---- refusals ----------------------------------------------------------------------------------------------------------

OPTIONS = {"hpd_frac": 0.8, "tol_length": 1e-6, "tol_weight": 1e-2, "tol_con_loss": 0.01, "weight_penalty": 0.1,
           "ns_ent": lambda K: 100 + 15 * K, "ns_ent_fast": 0, "ns_elbo": lambda K: 50 * K}


def refusal_cases():
    def vp_of(D, K, **flags):
        v = VariationalPosterior(D, K)
        for k, val in flags.items():
            setattr(v, k, val)
        return v

    return {
        "D>32": (lambda: vp_of(33, 2), None, {}, _lib.UnsupportedShape),
        "K>128": (lambda: vp_of(2, 2), 129, {}, _lib.UnsupportedShape),
        "sigma off": (lambda: vp_of(2, 2, optimize_sigma=False), None, {}, _lib.UnsupportedShape),
        "K_new<K": (lambda: vp_of(2, 3), 2, {}, _lib.UnsupportedShape),
        "K_new>K without mu": (lambda: vp_of(2, 2, optimize_mu=False), 3, {}, _lib.UnsupportedShape),
        "ns_ent_fast": (lambda: vp_of(2, 2), None, {"ns_ent_fast": 10}, _lib.UnsupportedShape),
        "no device": (lambda: vp_of(2, 2), None, {}, _lib.NoDeviceError),
    }


@pytest.mark.parametrize("what", list(refusal_cases()))
@pytest.mark.parametrize("rng", ["numpy", "philox"])
def test_refusals_leave_numpy_and_vp_untouched(what, rng):
    make, K, opts, exc = refusal_cases()[what]
    host = _lib.Context(-1)
    try:
        vp = make()
        before = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vp.__dict__.items() if k != "_ctx"}
        r = np.random.default_rng(1)
        gp = SimpleNamespace(X=r.standard_normal((10, vp.D)), y=r.standard_normal((10, 1)))
        np.random.seed(7)
        st = np.random.get_state(legacy=True)
        with pytest.raises(exc):
            sv.sieve(dict(OPTIONS, **opts), {"entropy_switch": False}, vp, gp, 7, 3, K, rng=rng, ctx=host)
        st1 = np.random.get_state(legacy=True)
        assert np.array_equal(st[1], st1[1]) and st[2:] == st1[2:]
        after = {k: v for k, v in vp.__dict__.items() if k != "_ctx"}
        assert before.keys() == after.keys()
        for k, v in before.items():
            assert np.array_equal(v, after[k]) if isinstance(v, np.ndarray) else v is after[k], k
        assert vp.bounds is None
    finally:
        host.close()


def test_init_N_zero_is_the_reference_return():
    host = _lib.Context(-1)
    try:
        vp = VariationalPosterior(2, 2)
        gp = SimpleNamespace(X=np.random.default_rng(1).standard_normal((10, 2)), y=np.zeros((10, 1)))
        out = sv.sieve(OPTIONS, {"entropy_switch": False}, vp, gp, 0, 1, None, ctx=host)
        assert out[0] is not vp and np.array_equal(out[0].mu, vp.mu) and out[1:] == (1, 0, False, math_ceil((100 + 30) / 2), 0)
    finally:
        host.close()


def math_ceil(x):
    import math

    return math.ceil(x)


# ---- patch_sieve ---------------------------------------------------------------------------------------------------------

def test_patch_sieve_binds_restores_and_falls_back():
    calls = []

    def ref_sieve(options, optim_state, vp, gp, init_N=None, best_N=1, K=None):
        calls.append((init_N, best_N, K))
        return "reference"

    vo = SimpleNamespace(_sieve=ref_sieve)
    assert dropin.patch_sieve(vo) is vo and vo._sieve is not ref_sieve and vo._sieve.__wrapped__ is sv.sieve
    first = vo._sieve
    dropin.patch_sieve(vo)  # idempotent: the saved binding is still the reference's
    assert vo._sieve is not first and getattr(vo, dropin._SAVED_SIEVE) is ref_sieve
    # a refused shape (optimize_sigma off) reaches the previous binding, with the reference's arguments
    vp = VariationalPosterior(2, 2)
    vp.optimize_sigma = False
    gp = SimpleNamespace(X=np.zeros((4, 2)), y=np.zeros((4, 1)))
    assert vo._sieve(OPTIONS, {"entropy_switch": False}, vp, gp, 5, 3) == "reference" and calls == [(5, 3, None)]
    dropin.unpatch_sieve(vo)
    assert vo._sieve is ref_sieve and not hasattr(vo, dropin._SAVED_SIEVE)
    dropin.unpatch_sieve(vo)  # a second time changes nothing
    assert vo._sieve is ref_sieve


def test_patch_sieve_keeps_make_sieve_behind_it():
    def ref_sieve(*a):
        return "reference"

    vo = SimpleNamespace(_sieve=ref_sieve, _neg_elcbo=lambda *a, **k: None)
    dropin.patch(vo, adam=False)
    wrapper = vo._sieve
    assert wrapper is not ref_sieve and wrapper.__wrapped__ is ref_sieve
    dropin.patch_sieve(vo)
    assert getattr(vo, dropin._SAVED_SIEVE) is wrapper
    dropin.unpatch_sieve(vo)
    assert vo._sieve is wrapper
    dropin.unpatch(vo)
    assert vo._sieve is ref_sieve
