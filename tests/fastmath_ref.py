"""Inputs, long-double references and the ulp metric for the device primitives of csrc/fastmath.h
(tests/test_fastmath_gpu.py runs them through libvbmc_devprobe.so; tests/test_fastmath_host.py checks the references
themselves against mpmath).

References are computed in np.longdouble (64-bit significand: 2^-11 of a double's ulp).  The error of a device result is
|got - ref| / spacing(float64(|ref|)), with 2^-1074 as the spacing where the result is subnormal or zero.

Every input family is deterministic (seeded default_rng) and is either "dense" (a random sweep) or "edge" (a list built
around the points where the code changes path: rint ties, the mantissa split of log_fast, quadrant boundaries, the
subnormal range).
"""
import functools
import math

import numpy as np

L = np.longdouble
assert np.finfo(L).eps <= 2.0**-63, "np.longdouble is not the 80-bit extended type: no reference for 1-2 ulp bounds"

TINY = 2.0**-1074
MIN_NORMAL = 2.0**-1022
DBL_MAX = np.finfo(np.float64).max
PI_L = L("3.14159265358979323846264338327950288419716939937510")
SQRT_HALF = float.fromhex("0x1.6a09e667f3bcdp-1")  # log_fast's mantissa split

# vbmc_probe_unary's fn / vbmc_probe_wave's op (csrc/devprobe.hip)
FN_EXP2, FN_LOG, FN_RCP, FN_RSQRT, FN_EXP2_GUARDED = range(5)
OP_SUM, OP_MAX, OP_PROD, OP_ROW16 = range(4)
WAVE_BLOCK = 256
WAVE_BLOCKS = 64


# ---- the metric -----------------------------------------------------------------------------------------------------


def ulp_spacing(ref):
    """spacing(float64(|ref|)); 2^-1074 where that is subnormal or zero."""
    a = np.abs(np.asarray(ref)).astype(np.float64)
    return np.where(a < MIN_NORMAL, TINY, np.spacing(a))


def ulp_error(got, ref):
    """|got - ref| in units of ulp_spacing(ref); got float64, ref long double, both finite."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=L)
    return np.asarray(np.abs(got.astype(L) - ref) / ulp_spacing(ref).astype(L), dtype=np.float64)


# ---- references -----------------------------------------------------------------------------------------------------


def ref_exp2(x):
    return np.exp2(np.asarray(x, dtype=np.float64).astype(L))


def ref_log(x):
    return np.log(np.asarray(x, dtype=np.float64).astype(L))


def ref_rcp(x):
    return L(1) / np.asarray(x, dtype=np.float64).astype(L)


def ref_rsqrt(x):
    return L(1) / np.sqrt(np.asarray(x, dtype=np.float64).astype(L))


def sincospi_reduce(y):
    """k = rint(2 y), r = y - k / 2: exact in float64 for y in [0, 2)."""
    y = np.asarray(y, dtype=np.float64)
    k = np.rint(2.0 * y)
    return k.astype(np.int64), y - 0.5 * k


def ref_sincospi(y):
    """(sin(pi y), cos(pi y)): reduced exactly first, so the values keep their relative accuracy at the zeros."""
    k, r = sincospi_reduce(y)
    a = PI_L * r.astype(L)
    s, c = np.sin(a), np.cos(a)
    q = k & 3
    return (np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s]))


# ---- input helpers --------------------------------------------------------------------------------------------------


def _rng(tag):
    return np.random.default_rng([20240607, tag])


def neighbours(c, n, lo=0.0, hi=np.inf):
    """The n doubles on either side of c > 0 (or above c = 0), and c: those that lie in [lo, hi)."""
    bits = np.array([c], dtype=np.float64).view(np.int64)[0] + np.arange(-n, n + 1, dtype=np.int64)
    x = bits[bits >= 0].view(np.float64)
    return x[(x >= lo) & (x < hi)]


def log_uniform(rng, n, e_lo, e_hi):
    """2^e (1 + u), e uniform over the integers e_lo .. e_hi, u uniform in [0, 1)."""
    e = rng.integers(e_lo, e_hi + 1, size=n)
    return np.ldexp(1.0 + rng.random(n), e)


# ---- input families: name -> (kind, x) ------------------------------------------------------------------------------
# (the names are listed apart so that collecting the tests computes nothing)

EXP2_FAMILIES = ("uniform", "fraction_shifted", "ties", "integers", "subnormal_results")
LOG_FAMILIES = ("log_uniform", "half_to_one", "one_to_two", "near_one", "mantissa_split", "subnormals", "box_muller",
                "dbl_max")
RCP_FAMILIES = ("log_uniform", "powers_of_two")
RSQRT_FAMILIES = ("log_uniform", "powers_of_four")
SINCOSPI_FAMILIES = ("uniform", "quarter_neighbours", "powers_of_two")


@functools.lru_cache(maxsize=None)
def exp2_families():
    rng = _rng(1)
    f = rng.uniform(-0.5, 0.5, 2**16)
    f[:2] = (-0.5, 0.5)
    n_tie = np.arange(-1080, 1024, dtype=np.float64)
    return {
        "uniform": ("dense", rng.uniform(-1022.0, 1023.99, 2**20)),
        "fraction_shifted": ("dense", np.concatenate([n + f for n in (0.0, 1.0, -1.0, 1023.0, -1022.0)])),
        "ties": ("edge", np.concatenate([n_tie - 0.5, n_tie + 0.5])),
        "integers": ("edge", np.arange(-1074, 1024, dtype=np.float64)),
        "subnormal_results": ("dense", rng.uniform(-1075.0, -1022.0, 2**16)),
    }


EXP2_ZERO = np.array([-1076.0, -1100.0, -2048.0, -(2.0**31), -(2.0**31) - 1.0, -3e9, -1e300, -DBL_MAX])
EXP2_INF = np.array([1024.0, 1500.0, 2.0**31, 1e300])
EXP2_GUARDED_ZERO = np.array([-np.inf, -1e308, -2049.0, -2048.0])


@functools.lru_cache(maxsize=None)
def log_families():
    rng = _rng(2)
    k = np.arange(0, 1025, dtype=np.float64)
    j = np.repeat(np.arange(1, 53), 8)
    u = rng.random(j.size)
    near = np.concatenate([1.0 - k * 2.0**-53, 1.0 + k * 2.0**-53, 1.0 - np.ldexp(u, -j), 1.0 + np.ldexp(u, -j)])
    split = neighbours(SQRT_HALF, 1025)  # frexp mantissas in [1/2, 1)
    sub = np.concatenate([
        np.array([1.0, 2.0, 3.0]), 2.0 ** np.arange(0, 52), rng.integers(1, 2**52, size=2**14).astype(np.float64)
    ]) * TINY
    kk = np.arange(1, 1025, dtype=np.float64)
    return {
        "log_uniform": ("dense", log_uniform(rng, 2**20, -1022, 1023)),
        "half_to_one": ("dense", rng.uniform(0.5, 1.0, 2**18)),  # e ln2 and ln m cancel here
        "one_to_two": ("dense", rng.uniform(1.0, 2.0, 2**18)),
        "near_one": ("edge", near),
        # binary exponents -1022, -1, 0, 1, 1023 of x = mantissa * 2^(exponent + 1)
        "mantissa_split": ("edge", np.concatenate([np.ldexp(split, e + 1) for e in (-1022, -1, 0, 1, 1023)])),
        "subnormals": ("edge", sub),
        "box_muller": ("edge", np.concatenate([kk * 2.0**-53, (2.0**53 - 1024.0 + np.arange(0, 1025)) * 2.0**-53])),
        "dbl_max": ("edge", np.array([DBL_MAX])),
    }


@functools.lru_cache(maxsize=None)
def rcp_families():
    rng = _rng(3)
    x = log_uniform(rng, 2**20, -1021, 1020)  # |x| in [2^-1021, 2^1021): x and 1/x both normal
    p2 = 2.0 ** np.arange(-1021, 1022)
    return {
        "log_uniform": ("dense", np.where(rng.random(x.size) < 0.5, -x, x)),
        "powers_of_two": ("edge", np.concatenate([p2, -p2])),
    }


@functools.lru_cache(maxsize=None)
def rsqrt_families():
    rng = _rng(4)
    return {
        "log_uniform": ("dense", log_uniform(rng, 2**20, -1022, 1023)),  # even and odd exponents
        "powers_of_four": ("edge", 4.0 ** np.arange(-511, 512)),
    }


SINCOSPI_EXACT = (np.array([0.0, 0.5, 1.0, 1.5]), np.array([0.0, 1.0, 0.0, -1.0]), np.array([1.0, 0.0, -1.0, 0.0]))


@functools.lru_cache(maxsize=None)
def sincospi_families():
    rng = _rng(5)
    return {
        "uniform": ("dense", rng.uniform(0.0, 2.0, 2**20)),
        # around k / 4: odd k are the ties of rint(2 y), even k the zeros and extrema; nextafter(2, 0) is the last one
        "quarter_neighbours": ("edge", np.concatenate([neighbours(k / 4.0, 1025, 0.0, 2.0) for k in range(9)])),
        "powers_of_two": ("edge", 2.0 ** -np.arange(1.0, 1075.0)),
    }


def dense_sample(x, n=4096):
    """n points of a dense sweep, evenly strided (the sweep is in random order)."""
    return x[:: max(1, x.size // n)][:n]


# ---- wave reductions: (v [blocks][256], expected) -------------------------------------------------------------------


def _waves(v):
    return v.reshape(v.shape[0], WAVE_BLOCK // 64, 64)


def wave_distinct_integers():
    """Small distinct integers: every partial sum is exact, so the result is the same bits in every lane."""
    return _rng(10).permutation(WAVE_BLOCKS * WAVE_BLOCK).astype(np.float64).reshape(WAVE_BLOCKS, WAVE_BLOCK) - 4096.0


def wave_one_hot(fill, values):
    """Block b: `fill` everywhere, but values[w] at lane b of wave w -- finds a dropped or doubled lane."""
    v = np.full((WAVE_BLOCKS, WAVE_BLOCK // 64, 64), float(fill))
    for b in range(WAVE_BLOCKS):
        v[b, :, b] = values
    return v.reshape(WAVE_BLOCKS, WAVE_BLOCK)


def expect_per_wave(v, reduce):
    """reduce over each wave's 64 lanes, broadcast back to [blocks][256]."""
    w = _waves(v)
    return np.broadcast_to(reduce(w, axis=2)[:, :, None], w.shape).reshape(v.shape)


def expect_per_row16(v):
    r = v.reshape(v.shape[0], WAVE_BLOCK // 16, 16)
    return np.broadcast_to(r.sum(axis=2)[:, :, None], r.shape).reshape(v.shape)


def wave_max_negative():
    """All-negative rows with the maximum at lane b of every wave: a 0 injected by a masked DPP step would win."""
    rng = _rng(11)
    v = -rng.uniform(2.0, 1000.0, (WAVE_BLOCKS, WAVE_BLOCK // 64, 64))
    for b in range(WAVE_BLOCKS):
        v[b, :, b] = -rng.uniform(0.5, 1.5, WAVE_BLOCK // 64)
    return v.reshape(WAVE_BLOCKS, WAVE_BLOCK)


def wave_max_neg_inf():
    """-inf in most lanes (as mode.hip feeds it): block b keeps finite values at lanes b and (5 b + 3) % 64; block 0's
    wave 3 is -inf throughout; block 1's wave 2 contains +inf."""
    rng = _rng(12)
    v = np.full((WAVE_BLOCKS, WAVE_BLOCK // 64, 64), -np.inf)
    for b in range(WAVE_BLOCKS):
        v[b, :, b] = rng.standard_normal(WAVE_BLOCK // 64) * 100.0
        v[b, :, (5 * b + 3) % 64] = rng.standard_normal(WAVE_BLOCK // 64) * 100.0
    v[0, 3, :] = -np.inf
    v[1, 2, 40] = np.inf
    return v.reshape(WAVE_BLOCKS, WAVE_BLOCK)


def wave_prod_exact():
    """Signs and powers of two whose products stay far from over- and underflow: exact."""
    rng = _rng(13)
    e = rng.integers(-8, 9, (WAVE_BLOCKS, WAVE_BLOCK))
    s = np.where(rng.random((WAVE_BLOCKS, WAVE_BLOCK)) < 0.5, -1.0, 1.0)
    v = s * np.ldexp(1.0, e)
    v[0] = s[0]  # signs alone
    v[1] = np.ldexp(1.0, e[1])  # powers of two alone
    return v


def wave_prod_with_zero():
    v = wave_prod_exact()
    for b in range(WAVE_BLOCKS):
        _waves(v)[b, :, b] = 0.0 if b % 2 else -0.0
    return v


def fsum_per_wave(v):
    w = _waves(v)
    return np.array([[math.fsum(w[b, i]) for i in range(w.shape[1])] for b in range(w.shape[0])])
