"""The dimensions of the width sweeps.  TEST INFRASTRUCTURE.

Kernels templated on the padded dimension are instantiated by ``VBMC_DISPATCH_DP`` (csrc/common.h) at ten widths, and D is
rounded up to the next of them.  D = 2 and 3 (the small cases of every family) reach the first two; ``SWEEP_D`` holds one D
for each of the other eight, some "odd, below the width" -- where a pair loop's second element lands on index D and a
padded lane follows the last real one -- and some "exactly the width", where nothing is padded:

    D      5  7  10  11  13  20  21  32
    width  6  8  10  12  16  20  24  32

tests/test_scratch_layout.py asserts that {2, 3} and SWEEP_D together reach every width the macro names, so that a width
added there without a case here fails on the CPU.  ``WORKLOAD_D`` are the benchmark's two dimensions, the subset for the
chain-type families whose host replays take seconds per case.
"""
import re
from pathlib import Path

SMALL_D = (2, 3)
SWEEP_D = (5, 7, 10, 11, 13, 20, 21, 32)
WORKLOAD_D = (10, 20)
MODE_D = (3, 7, 11, 13, 21)  # the widths tests/test_mode_gpu.py's cases (D = 1, 2, 6, 10, 20, 32) do not reach

COMMON_H = Path(__file__).resolve().parent.parent / "pyvbmc_amd" / "csrc" / "common.h"


def dispatch_widths(text=None):
    """The widths ``VBMC_DISPATCH_DP`` instantiates, in the macro's order, read from csrc/common.h."""
    text = COMMON_H.read_text() if text is None else text
    start = text.index("#define VBMC_DISPATCH_DP")
    lines = []
    for line in text[start:].splitlines():  # the macro's body: up to the first line without a continuation
        lines.append(line)
        if not line.rstrip().endswith("\\"):
            break
    return tuple(int(w) for w in re.findall(r"CALL\((\d+)\)", "\n".join(lines)))


def padded_width(D, widths):
    """The width the macro picks for D: the first one >= D, the last one past that."""
    return next((w for w in widths if D <= w), widths[-1])
