"""CPU side of the fastmath.h primitive tests.

* The long-double references of tests/fastmath_ref.py, on their own: over every edge list and 4096 points of every dense
  sweep they agree with mpmath at 50 digits to within 0.01 ulp of a double, so an error measured against them on the
  device (caps of 1 - 2.5 ulp, tests/test_fastmath_gpu.py) is the primitive's.
* libvbmc_devprobe.so, the probe library those tests call, is built, loads and exports its three entry points.
"""
import ctypes

import numpy as np
import pytest

import fastmath_ref as fr

REF_TOL = 0.01  # ulp of float64


def to_mpf(mp, v):
    """A long double as an mpf, exactly."""
    m, e = np.frexp(v)
    return mp.mpf(int(np.ldexp(m, 64))) * mp.mpf(2) ** (int(e) - 64)


def worst(mp, xs, refs, exact):
    """max over the points of |ref - exact(x)| in ulps of float64 at ref, and where."""
    sp = fr.ulp_spacing(refs)
    w, at = 0.0, None
    for x, r, s in zip(xs, refs, sp):
        e = float(abs(to_mpf(mp, r) - exact(mp.mpf(float(x)))) / mp.mpf(float(s)))
        if e > w:
            w, at = e, float(x)
    return w, at


def points(families):
    return np.concatenate([x if kind == "edge" else fr.dense_sample(x) for kind, x in families.values()])


@pytest.fixture(scope="module")
def mp():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    return mpmath


@pytest.mark.parametrize(
    "name,families,ref,exact",
    [
        ("exp2", fr.exp2_families, fr.ref_exp2, lambda mp: lambda x: mp.mpf(2) ** x),
        ("log", fr.log_families, fr.ref_log, lambda mp: mp.log),
        ("rcp", fr.rcp_families, fr.ref_rcp, lambda mp: lambda x: 1 / x),
        ("rsqrt", fr.rsqrt_families, fr.ref_rsqrt, lambda mp: lambda x: 1 / mp.sqrt(x)),
    ],
)
def test_long_double_reference_against_mpmath(mp, name, families, ref, exact):
    xs = points(families())
    w, at = worst(mp, xs, ref(xs), exact(mp))
    print(f"{name}: reference within {w:.2e} ulp of mpmath over {xs.size} points (worst at {at!r})")
    assert w <= REF_TOL


def test_sincospi_reference_against_mpmath(mp):
    xs = np.concatenate([points(fr.sincospi_families()), fr.SINCOSPI_EXACT[0]])
    s, c = fr.ref_sincospi(xs)
    ws, at_s = worst(mp, xs, s, mp.sinpi)
    wc, at_c = worst(mp, xs, c, mp.cospi)
    print(f"sincospi: reference within {ws:.2e} / {wc:.2e} ulp of mpmath over {xs.size} points "
          f"(worst at {at_s!r} / {at_c!r})")
    assert ws <= REF_TOL and wc <= REF_TOL
    # the reduction is exact and lands in [-1/4, 1/4]
    k, r = fr.sincospi_reduce(xs)
    assert np.all(np.abs(r) <= 0.25) and np.all(r.astype(fr.L) + k.astype(fr.L) / 2 == xs.astype(fr.L))


def test_family_names():
    for names, fam in ((fr.EXP2_FAMILIES, fr.exp2_families), (fr.LOG_FAMILIES, fr.log_families),
                       (fr.RCP_FAMILIES, fr.rcp_families), (fr.RSQRT_FAMILIES, fr.rsqrt_families),
                       (fr.SINCOSPI_FAMILIES, fr.sincospi_families)):
        assert tuple(fam()) == names


def test_ulp_metric():
    got = np.array([1.0, 1.0 + 2.0**-52, 2.0**-1074, 0.0, 3 * 2.0**-1074, 2.0**-1022])
    ref = np.array([1.0, 1.0, 0.0, 0.0, 2.0**-1073, 2.0**-1022 - 2.0**-1074], dtype=fr.L)
    ref[3] = fr.L(2.0) ** -1075  # below float64's range
    assert fr.ulp_error(got, ref).tolist() == [0.0, 1.0, 1.0, 0.5, 1.0, 1.0]
    assert fr.ulp_error(np.array([1.0]), np.array([1.0], dtype=fr.L) - fr.L(2.0) ** -54)[0] == 0.25


def test_probe_library_is_built_and_exports_its_entry_points():
    from pyvbmc_amd import build as b

    assert b.PROBE_LIB.exists(), "python -m pyvbmc_amd.build builds libvbmc_devprobe.so next to libvbmc_hip.so"
    assert "devprobe.hip" not in b.SOURCES  # a shared object of its own, not part of libvbmc_hip.so
    lib = ctypes.CDLL(str(b.PROBE_LIB))
    for sym in ("vbmc_probe_unary", "vbmc_probe_sincospi", "vbmc_probe_wave"):
        assert hasattr(lib, sym), sym
    main = ctypes.CDLL(str(b.LIB))
    assert not hasattr(main, "vbmc_probe_unary") and main.vbmc_abi_version() == 2
