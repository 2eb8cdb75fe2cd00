"""Every polynomial of csrc/fastmath.h is the one tools/fit_polys.py fits, bit for bit: exp2_fast (degree 11), log_fast
(c[1:] of the degree-8 atanh(s)/s fit), sincospi_fast (the two degree-6 fits) and the entropy kernels' degree-8 2^f.

The entropy kernels' exp2 polynomial (csrc/fastmath.h VBMC_ENT_EXP2_COEFFS) is what tools/fit_polys.py fits:
degree 8 on |f| <= 1/2, Chebyshev-node interpolation in 60-digit arithmetic, and its error in float64 Horner
evaluation is the 1.07e-12 the header's accuracy argument starts from."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def header_coeffs():
    text = (ROOT / "pyvbmc_amd" / "csrc" / "fastmath.h").read_text()
    n = int(re.search(r"#define VBMC_ENT_EXP2_N (\d+)", text).group(1))
    body = text[text.index("#define VBMC_ENT_EXP2_COEFFS"):]
    body = body[: body.index("}") + 1]
    vals = [float.fromhex(h) for h in re.findall(r"0x[0-9a-fA-F.]+p[-+]?\d+", body)]
    assert len(vals) == n
    return n, vals


def test_entropy_exp2_polynomial_is_the_fitted_one():
    pytest.importorskip("mpmath")
    sys.path.insert(0, str(ROOT / "tools"))
    import mpmath as mp
    from fit_polys import cheb_fit, horner64

    n, vals = header_coeffs()
    half = mp.mpf(1) / 2
    c = cheb_fit(lambda x: mp.mpf(2) ** x, -half, half, n)
    assert abs(float(c[0]) - 1.0) < 1e-15  # the kernels use the constant 1 exactly
    assert [float(x).hex() for x in c[1:]] == [v.hex() for v in vals]
    f = np.linspace(-0.5, 0.5, 400001)
    err = np.max(np.abs(horner64([1.0] + vals, f) / np.exp2(f) - 1))
    assert 5e-13 < err < 1.1e-12, err


HEX = r"-?0x[0-9a-fA-F.]+p[-+]?\d+"


def horner_coeffs(fn, var):
    """The constants of `var`'s Horner chain in fm::`fn`, in the header's order (highest degree first): the hex
    initialiser of `double var = ...;` and the addend of every `var = fma(var, <arg>, <addend>);` after it."""
    text = (ROOT / "pyvbmc_amd" / "csrc" / "fastmath.h").read_text()
    body = text[text.index(f" {fn}(double "):]
    body = body[: body.index("\n}\n")]
    first = re.search(rf"double {var} = ({HEX});", body)
    rest = re.findall(rf"\b{var} = fma\({var}, \w+, ([^)]+)\);", body[first.end():])
    return [first.group(1)] + rest


def fitted(c):
    return [float(x).hex() for x in c]


def as_hex(tokens):
    return [float.fromhex(t).hex() for t in tokens]


@pytest.fixture(scope="module")
def fits():
    pytest.importorskip("mpmath")
    sys.path.insert(0, str(ROOT / "tools"))
    import fit_polys

    return fit_polys


def test_exp2_fast_polynomial_is_the_fitted_one(fits):
    c = fitted(fits.fit_exp2(11))
    toks = horner_coeffs("exp2_fast", "p")
    assert len(toks) == 12 and toks[-1] == "1.0" and c[0] == (1.0).hex()  # f = 0 gives p = 1 exactly
    assert as_hex(toks[:-1]) == c[:0:-1]


def test_log_fast_polynomial_is_the_fitted_one(fits):
    c = fitted(fits.fit_atanh(8))
    toks = horner_coeffs("log_fast", "p")
    assert len(toks) == 8 and c[0] == (1.0).hex()  # ln m = 2 s (1 + u p): the kernel uses the constant 1 exactly
    assert as_hex(toks) == c[:0:-1]


def test_sincospi_fast_polynomials_are_the_fitted_ones(fits):
    cs, cc = fitted(fits.fit_sinpi(6)), fitted(fits.fit_cospi(6))
    ts, tc = horner_coeffs("sincospi_fast", "ps"), horner_coeffs("sincospi_fast", "pc")
    assert len(ts) == 7 and as_hex(ts) == cs[::-1]
    assert len(tc) == 7 and tc[-1] == "1.0" and cc[0] == (1.0).hex()  # cos(0) = 1 exactly
    assert as_hex(tc[:-1]) == cc[:0:-1]
