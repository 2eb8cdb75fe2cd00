"""csrc/scratch.h, the carver every entry point lists its device scratch through, run on the host through the probe
library (libvbmc_devprobe.so, csrc/devprobe.hip: vbmc_probe_scratch_layout).  No GPU needed.

The two fixed layouts at the end are derived by hand from the entry points as they were before they were converted to the
carver: a conversion that reorders, resizes or realigns a piece fails here.
"""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def carve():
    from pyvbmc_amd import build as b

    lib = ctypes.CDLL(str(b.PROBE_LIB))
    fn = lib.vbmc_probe_scratch_layout
    ptr = ctypes.POINTER(ctypes.c_size_t)
    fn.argtypes = [ctypes.c_int, ptr, ptr, ptr, ptr, ptr]
    fn.restype = None

    def run(pieces):
        """pieces: (count, element bytes, alignment in doubles) -> (offsets, total), in doubles"""
        cols = [np.ascontiguousarray([p[i] for p in pieces], dtype=np.uintp) for i in range(3)]
        off = np.zeros(len(pieces), dtype=np.uintp)
        total = ctypes.c_size_t(0)
        fn(len(pieces), *[c.ctypes.data_as(ptr) for c in cols], off.ctypes.data_as(ptr), ctypes.byref(total))
        return [int(o) for o in off], int(total.value)

    return run


def occupied(count, elem_bytes):
    return -(-count * elem_bytes // 8)  # ceil(bytes / 8) doubles


def test_carver_properties(carve):
    pieces = [(15, 8, 1), (5, 4, 1), (0, 8, 32), (7, 8, 32), (3, 4, 1), (1, 1, 1), (0, 4, 1), (9, 8, 4), (2, 8, 1),
              (1, 8, 64), (0, 8, 1)]
    off, total = carve(pieces)
    end = 0
    for (count, eb, align), o in zip(pieces, off):
        assert o >= end  # increasing, no overlap
        if count == 0:
            assert o == end  # takes nothing, not even alignment padding
            continue
        assert o % align == 0 and o - end < align  # aligned, with no more padding than that needs
        end = o + occupied(count, eb)
    assert total == end  # the end of the last piece
    # a typed piece is rounded up to whole doubles: the piece behind it starts there
    off, total = carve([(5, 4, 1), (1, 8, 1)])
    assert off == [0, 3] and total == 4
    off, total = carve([(1, 1, 1), (1, 2, 1), (3, 4, 1), (4, 4, 1)])
    assert off == [0, 1, 2, 4] and total == 6
    assert carve([]) == ([], 0)
    assert carve([(0, 8, 32), (0, 4, 1)]) == ([0, 0], 0)


def test_mixture_sample_layout(carve):
    # mixture_sample_impl, N = 5, D = 3, K = 2, labels wanted: x (N D doubles) | labels (N int32) | selector (2 K + 2)
    N, D, K = 5, 3, 2
    off, total = carve([(N * D, 8, 1), (N, 4, 1), (2 * K + 2, 8, 1)])
    assert off == [0, 15, 18] and total == 24
    # without labels the selector follows x
    off, total = carve([(N * D, 8, 1), (0, 4, 1), (2 * K + 2, 8, 1)])
    assert off == [0, 15, 15] and total == 21


def test_predict_plan_layout(carve):
    # predict_plan, M = 5 (so mb = 5), D = 3, N = 65, S = 2, no pieces of the caller's:
    # xs (mb D) | Ks [S][64-row tiles of mb][ld = 128], 32-double aligned | part, fpart [S][ntiles = 2][mb] | fmu | fs2
    mb, D, N, S = 5, 3, 65, 2
    ld, rows, ntiles = 128, 64, 2
    off, total = carve([(mb * D, 8, 1), (S * rows * ld, 8, 32), (2 * S * ntiles * mb, 8, 1), (S * mb, 8, 1), (S * mb, 8, 1)])
    assert off == [0, 32, 16416, 16456, 16466] and total == 16476


def test_every_dispatch_width_has_a_sweep_dimension():
    """Every width VBMC_DISPATCH_DP (csrc/common.h) instantiates is the padded width of a D in {2, 3} or SWEEP_D
    (tests/width_cases.py): a width added to the macro without a case, or a D taken out of the list, fails here."""
    import re

    import width_cases as wc

    widths = wc.dispatch_widths()
    assert len(widths) >= 10 and list(widths) == sorted(set(widths)) and widths[-1] == 32
    # the macro's thresholds are its widths: "(D) <= w" picks CALL(w), the last width takes the rest
    text = wc.COMMON_H.read_text()
    body = text[text.index("#define VBMC_DISPATCH_DP"):].split("while (0)")[0]
    assert tuple(int(t) for t in re.findall(r"\(D\) <= (\d+)", body)) == widths[:-1]
    dims = wc.SMALL_D + wc.SWEEP_D
    reached = {wc.padded_width(D, widths) for D in dims}
    assert reached == set(widths), f"no sweep dimension for the widths {sorted(set(widths) - reached)}"
    assert len(dims) == len(widths)  # one D per width
    ws = [wc.padded_width(D, widths) for D in wc.SWEEP_D]
    assert all(D == w or (D % 2 == 1 and D < w) for D, w in zip(wc.SWEEP_D, ws))  # the width itself, or odd and padded
    assert any(D == w for D, w in zip(wc.SWEEP_D, ws)) and any(D < w for D, w in zip(wc.SWEEP_D, ws))
    assert set(wc.WORKLOAD_D) <= set(wc.SWEEP_D)
    assert {wc.padded_width(D, widths) for D in (1, 2, 6, 10, 20, 32) + wc.MODE_D} == set(widths)
    # removing any one dimension leaves a width without a case
    for D in dims:
        assert {wc.padded_width(d, widths) for d in dims if d != D} != set(widths)
