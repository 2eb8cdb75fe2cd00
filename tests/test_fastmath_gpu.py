"""The device primitives of csrc/fastmath.h, each on its own (through libvbmc_devprobe.so, csrc/devprobe.hip), against
the long-double references of tests/fastmath_ref.py (themselves within 0.01 ulp of mpmath: tests/test_fastmath_host.py).

The caps are hard, in ulps of float64 at the true value (fastmath_ref.ulp_error), and come from the headers' own claims
and a host model of the same FMA sequences, not from what the device returns:

    exp2_fast      1     mixture_dev.h's "<= 1 ulp"; only exact IEEE operations; host model 0.93
    rcp_fast       1     fastmath.h "~1 ulp"; host model 0.50
    rsqrt_fast     1.5   fastmath.h "~1 ulp"; host model 0.998 with a seed that is not the hardware's
    sincospi_fast  2     fastmath.h's upper figure, at the zeros as well; host model 1.80
    log_fast       2.5   fastmath.h's upper figure plus a quarter: the host model already reaches 1.99

Each test prints the maximum it measured and the argument where it occurs (profiles/fastmath_ulp.md keeps the figures).
The DPP reductions run in blocks of 256 threads (four full waves) and every lane's own result is compared.
"""
import ctypes

import numpy as np
import pytest

import fastmath_ref as fr

pytestmark = pytest.mark.gpu

CAP = {"exp2": 1.0, "rcp": 1.0, "rsqrt": 1.5, "sincospi": 2.0, "log": 2.5}
EPS = float(np.finfo(np.float64).eps)

_DP = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def probe():
    from pyvbmc_amd import build as b

    lib = ctypes.CDLL(str(b.PROBE_LIB))  # a missing probe library is an error, not a skip
    lib.vbmc_probe_unary.argtypes = [ctypes.c_int, _DP, _DP, ctypes.c_size_t]
    lib.vbmc_probe_sincospi.argtypes = [_DP, _DP, _DP, ctypes.c_size_t]
    lib.vbmc_probe_wave.argtypes = [ctypes.c_int, _DP, _DP, ctypes.c_int]
    for f in (lib.vbmc_probe_unary, lib.vbmc_probe_sincospi, lib.vbmc_probe_wave):
        f.restype = ctypes.c_int
    return lib


def _ptr(a):
    return a.ctypes.data_as(_DP)


def unary(probe, fn, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.full_like(x, np.nan)
    rc = probe.vbmc_probe_unary(fn, _ptr(x), _ptr(y), x.size)
    assert rc == 0, f"vbmc_probe_unary: HIP error {rc}"
    return y


def sincospi(probe, y):
    y = np.ascontiguousarray(y, dtype=np.float64)
    s, c = np.full_like(y, np.nan), np.full_like(y, np.nan)
    rc = probe.vbmc_probe_sincospi(_ptr(y), _ptr(s), _ptr(c), y.size)
    assert rc == 0, f"vbmc_probe_sincospi: HIP error {rc}"
    return s, c


def wave(probe, op, v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    assert v.ndim == 2 and v.shape[1] == fr.WAVE_BLOCK
    out = np.full_like(v, np.nan)
    rc = probe.vbmc_probe_wave(op, _ptr(v), _ptr(out), v.shape[0])
    assert rc == 0, f"vbmc_probe_wave: HIP error {rc}"
    return out


def measure(label, x, got, ref, cap):
    """Print the maximum ulp error and where; assert every result finite and within the cap."""
    assert np.all(np.isfinite(got)), (label, x[~np.isfinite(got)][:8])
    err = fr.ulp_error(got, ref)
    i = int(np.argmax(err))
    print(f"{label}: max {err[i]:.3f} ulp at x = {float(x[i]).hex()} ({x[i]!r}), {x.size} points, cap {cap}")
    assert err[i] <= cap, (label, err[i], float(x[i]).hex())
    return err


# ---- exp2_fast ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("family", fr.EXP2_FAMILIES)
def test_exp2_fast(probe, family):
    x = fr.exp2_families()[family][1]
    got = unary(probe, fr.FN_EXP2, x)
    measure(f"exp2_fast[{family}]", x, got, fr.ref_exp2(x), CAP["exp2"])
    if family == "integers":  # f = 0 makes p exactly 1
        assert np.array_equal(got, np.ldexp(1.0, x.astype(np.int64)))


def test_exp2_fast_underflow_and_overflow(probe):
    z = unary(probe, fr.FN_EXP2, fr.EXP2_ZERO)
    assert np.array_equal(z, np.zeros_like(z)) and not np.any(np.signbit(z)), z
    o = unary(probe, fr.FN_EXP2, fr.EXP2_INF)
    assert np.array_equal(o, np.full_like(o, np.inf)), o


def test_exp2_fast_guarded(probe):
    """exp2_fast(exp2_arg(x)), the form the mixture density uses."""
    z = unary(probe, fr.FN_EXP2_GUARDED, fr.EXP2_GUARDED_ZERO)
    assert np.array_equal(z, np.zeros_like(z)), z
    assert np.isnan(unary(probe, fr.FN_EXP2_GUARDED, np.array([np.nan]))[0])
    x = fr.dense_sample(fr.exp2_families()["uniform"][1])  # the guard leaves everything above -2048 alone
    assert np.array_equal(unary(probe, fr.FN_EXP2_GUARDED, x), unary(probe, fr.FN_EXP2, x))


# ---- log_fast -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("family", fr.LOG_FAMILIES)
def test_log_fast(probe, family):
    x = fr.log_families()[family][1]
    measure(f"log_fast[{family}]", x, unary(probe, fr.FN_LOG, x), fr.ref_log(x), CAP["log"])


def test_log_fast_of_zero(probe):
    y = unary(probe, fr.FN_LOG, np.array([0.0, -0.0]))
    assert np.array_equal(y, [-np.inf, -np.inf]), y


# ---- rcp_fast, rsqrt_fast -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("family", fr.RCP_FAMILIES)
def test_rcp_fast(probe, family):
    x = fr.rcp_families()[family][1]
    got = unary(probe, fr.FN_RCP, x)
    measure(f"rcp_fast[{family}]", x, got, fr.ref_rcp(x), CAP["rcp"])
    if family == "powers_of_two":
        assert np.array_equal(got, 1.0 / x)


@pytest.mark.parametrize("family", fr.RSQRT_FAMILIES)
def test_rsqrt_fast(probe, family):
    x = fr.rsqrt_families()[family][1]
    got = unary(probe, fr.FN_RSQRT, x)
    measure(f"rsqrt_fast[{family}]", x, got, fr.ref_rsqrt(x), CAP["rsqrt"])
    if family == "powers_of_four":  # 4^n -> 2^-n
        assert np.array_equal(got, np.ldexp(1.0, -np.arange(-511, 512)))


# ---- sincospi_fast --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("family", fr.SINCOSPI_FAMILIES)
def test_sincospi_fast(probe, family):
    y = fr.sincospi_families()[family][1]
    s, c = sincospi(probe, y)
    rs, rc = fr.ref_sincospi(y)
    measure(f"sincospi_fast[{family}] sin", y, s, rs, CAP["sincospi"])
    measure(f"sincospi_fast[{family}] cos", y, c, rc, CAP["sincospi"])


def test_sincospi_fast_exact_points(probe):
    y, es, ec = fr.SINCOSPI_EXACT
    s, c = sincospi(probe, y)
    assert np.array_equal(s, es) and np.array_equal(c, ec), (s, c)  # 0.0 == -0.0: the sign of a zero is not asserted
    last = np.array([np.nextafter(2.0, 0.0)])
    s, c = sincospi(probe, last)
    rs, rc = fr.ref_sincospi(last)
    measure("sincospi_fast[nextafter(2, 0)] sin", last, s, rs, CAP["sincospi"])
    measure("sincospi_fast[nextafter(2, 0)] cos", last, c, rc, CAP["sincospi"])


# ---- DPP reductions -------------------------------------------------------------------------------------------------


def same_bits(got, want, label):
    bad = np.argwhere(got.view(np.int64) != np.asarray(want, dtype=np.float64).view(np.int64))
    print(f"{label}: {got.size - len(bad)} of {got.size} lanes bit-equal")
    assert len(bad) == 0, (label, bad[:8].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def same_values(got, want, label):
    """Equal as numbers (infinities included); every lane."""
    bad = np.argwhere(~(got == want))
    print(f"{label}: {got.size - len(bad)} of {got.size} lanes equal")
    assert len(bad) == 0, (label, bad[:8].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("op,expect", [(fr.OP_SUM, lambda v: fr.expect_per_wave(v, np.sum)), (fr.OP_ROW16, fr.expect_per_row16)],
                         ids=["wave_sum_dpp", "row16_sum_dpp"])
def test_wave_sums_exact(probe, op, expect):
    v = fr.wave_distinct_integers()
    same_bits(wave(probe, op, v), expect(v), "distinct integers")
    v = fr.wave_one_hot(0.0, [3.0, 5.0, 7.0, 11.0])
    same_bits(wave(probe, op, v), expect(v), "one-hot")


def test_wave_sum_dpp_real_values(probe):
    v = fr._rng(20).standard_normal((1, fr.WAVE_BLOCK))
    got = wave(probe, fr.OP_SUM, v)
    ref = fr.fsum_per_wave(v)[0]
    bound = 6 * EPS * np.abs(fr._waves(v)[0]).sum(axis=1)  # six rounding levels
    g = fr._waves(got)[0]
    err = np.abs(g - ref[:, None]).max(axis=1)
    print(f"wave_sum_dpp on standard normals: max error {np.max(err / bound):.3f} of 6 eps sum|v|")
    assert np.all(err <= bound)
    assert np.all(g == g[:, :1])  # the same value in every lane of a wave


def test_wave_max_dpp(probe):
    for label, v in (("all negative", fr.wave_max_negative()), ("-inf rows", fr.wave_max_neg_inf())):
        same_values(wave(probe, fr.OP_MAX, v), fr.expect_per_wave(v, np.max), f"wave_max_dpp, {label}")
    v = fr.wave_max_neg_inf()
    assert fr.expect_per_wave(v, np.max)[1, 128] == np.inf and fr.expect_per_wave(v, np.max)[0, 192] == -np.inf


def test_wave_prod_dpp(probe):
    v = fr.wave_prod_exact()
    same_bits(wave(probe, fr.OP_PROD, v), fr.expect_per_wave(v, np.prod), "wave_prod_dpp, signs and powers of two")
    v = fr.wave_one_hot(1.0, [3.0, 5.0, 7.0, 11.0])
    same_bits(wave(probe, fr.OP_PROD, v), fr.expect_per_wave(v, np.prod), "wave_prod_dpp, one-hot")
    v = fr.wave_prod_with_zero()
    same_values(wave(probe, fr.OP_PROD, v), np.zeros_like(v), "wave_prod_dpp, a zero in every wave")
    v = fr._rng(21).uniform(0.9, 1.1, (1, fr.WAVE_BLOCK))
    g = fr._waves(wave(probe, fr.OP_PROD, v))[0]
    ref = np.prod(fr._waves(v)[0].astype(fr.L), axis=1)
    rel = np.asarray(np.abs(g.astype(fr.L) - ref[:, None]) / ref[:, None], dtype=np.float64).max(axis=1)
    print(f"wave_prod_dpp on (0.9, 1.1): max relative error {np.max(rel) / EPS:.2f} eps, bound 64 eps")
    assert np.all(rel <= 64 * EPS)  # 63 roundings
    assert np.all(g == g[:, :1])
