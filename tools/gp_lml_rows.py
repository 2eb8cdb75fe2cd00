#!/usr/bin/env python
"""Wall-clock milliseconds of the batched GP log marginal likelihood on the device, next to the host route on the same
box.

    python tools/gp_lml_rows.py [--reps 10] [--warm 2] [--host-reps 3] [--out profiles/gp_lml_rows.json]

Shapes (D, N, B): (10, 400, 1), (10, 400, 256), (20, 800, 1), (20, 800, 64), each for the value alone and for value
plus gradient.  Rows, medians after warm-up calls:
  a  the host route, ``log_marginal_likelihood(device=False)`` (NumPy / SciPy's LAPACK at the box's thread setting);
  b  the device call end to end, ``log_marginal_likelihood(device=True)`` (uploads, chunks, downloads included);
  c  ``vbmc_last_kernel_ms(T_GP_LML)``: factorisation plus value / gradient kernels of ONE chunk, measured on a call of
     ``kernel_B`` = min(B, chunk) candidates so that the interval covers all of them.
``grad_tile_ms`` is c with the gradient minus c without it: the gradient-tile kernel plus the two small kernels behind
it, hence an upper bound of the tile kernel's time, and ``grad_tile_fp64_peak_fraction`` the share of the FP64 matrix
peak (78.6 TFLOP/s) that kernel_B N^3 / 3 flops in that time amount to (a lower bound).  Every shape runs in a fresh child
process under ``timeout -k 10 <--limit>``; after a child that does not exit with 0 nothing further is started and the
tool exits with that status.  One JSON line per shape, collected by the parent and written to --out."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pyvbmc_amd import _lib  # noqa: E402
from pyvbmc_amd import gp as gpm  # noqa: E402

SHAPES = ((10, 400, 1), (10, 400, 256), (20, 800, 1), (20, 800, 64))
FP64_MATRIX_PEAK = 78.6e12
CAP_BYTES = 1 << 30  # csrc/common.h GP_LML_CAP_BYTES


def plan_chunk(N, D, B):
    """csrc/common.h gp_lml_plan: candidates per chunk under the byte cap."""
    nb = (N + 63) // 64
    per = 8 * (2 * N * N + (64 * nb) ** 2 + nb * 4096 + nb * (nb + 1) // 2 * (D + 2))
    return max(1, min(B, CAP_BYTES // per))


def make_case(D, N, B, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D)) * 2.0
    y = (-0.5 * np.sum(X**2, axis=1) / D + 0.3 * rng.standard_normal(N)).reshape(-1, 1)
    hyp = np.array([np.concatenate([np.log(0.8 * np.sqrt(D) * (1 + 0.2 * rng.random(D))), [np.log(1.0 + 0.3 * rng.random())],
                                    [np.log(0.3 * (1 + 0.2 * rng.random()))], [0.1], 0.1 * rng.standard_normal(D),
                                    np.log(2.0 + rng.random(D))]) for _ in range(B)])
    return X, y, hyp


def timed(fn, reps, warm):
    t = []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warm:
            t.append(dt)
    return round(statistics.median(t), 3), [round(min(t), 3), round(max(t), 3)]


def run_shape(D, N, B, reps, warm, host_reps):
    ctx = _lib.Context(0)
    _lib.set_default_context(ctx)
    X, y, hyp = make_case(D, N, B, 100 + B)
    gp = gpm.GP(D, gpm.SquaredExponential(), gpm.NegativeQuadratic(), gpm.GaussianNoise(constant_add=True))
    gp.ctx = ctx
    gp.X, gp.y = X, y
    kb = plan_chunk(N, D, B)
    row = {"row": f"D{D}_N{N}_B{B}", "reps": reps, "warm": warm, "host_reps": host_reps, "kernel_B": kb}
    for grad, tag in ((False, "value"), (True, "grad")):
        row[f"a_host_{tag}_ms"], row[f"a_host_{tag}_min_max_ms"] = timed(
            lambda: gpm.log_marginal_likelihood(gp, hyp, grad=grad, device=False), host_reps, 1)
        row[f"b_device_{tag}_ms"], row[f"b_device_{tag}_min_max_ms"] = timed(
            lambda: gpm.log_marginal_likelihood(gp, hyp, grad=grad, ctx=ctx), reps, warm)
        ctx.set_timing(1)
        k = []
        for _ in range(warm + reps):
            gpm.log_marginal_likelihood(gp, hyp[:kb], grad=grad, ctx=ctx)
            k.append(ctx.last_kernel_ms(_lib.T_GP_LML))
        ctx.set_timing(0)
        row[f"c_kernels_{tag}_ms"] = round(statistics.median(k[warm:]), 4)
        row[f"device_lt_host_{tag}"] = row[f"b_device_{tag}_ms"] < row[f"a_host_{tag}_ms"]
    tile = row["c_kernels_grad_ms"] - row["c_kernels_value_ms"]
    row["grad_tile_ms"] = round(tile, 4)
    row["grad_tile_fp64_peak_fraction"] = round(kb * N**3 / 3 / (tile * 1e-3) / FP64_MATRIX_PEAK, 4) if tile > 0 else None
    print(json.dumps(row), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    ap.add_argument("--shape", type=int, default=None, help="(child) run shape number SHAPE in this process")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gp_lml_rows.json"))
    a = ap.parse_args()
    if a.shape is not None:
        run_shape(*SHAPES[a.shape], a.reps, a.warm, a.host_reps)
        return 0
    lines = []
    for i in range(len(SHAPES)):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, str(Path(__file__).resolve()), "--shape", str(i),
               "--reps", str(a.reps), "--warm", str(a.warm), "--host-reps", str(a.host_reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f"shape {SHAPES[i]}: child ended with status {p.returncode}; nothing further is started", file=sys.stderr)
            return p.returncode
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
