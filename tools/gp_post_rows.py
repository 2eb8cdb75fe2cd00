#!/usr/bin/env python
"""Wall-clock milliseconds of building and extending the GP posterior on the device, next to the host route on the same
box.

    python tools/gp_post_rows.py [--reps 20] [--warm 3] [--out profiles/gp_post_rows.json]

Shapes (D, N, S): (10, 400, 1) and (20, 800, 8).  Rows, each the median of --reps calls after --warm warm-up calls and
each ending with the GP usable on the device (``upload_gp`` returned):
  a  the host route: ``GP.update`` (SciPy Cholesky per sample) then ``upload_gp`` (vbmc_set_gp ships L);
  b  ``GP.update(device=True, fetch=True)`` then ``upload_gp`` (which ships nothing);
  c  the same with ``fetch=False``;
  d  the host route for one added point: ``GP.update`` on N + 1 rows then ``upload_gp``;
  e  ``GP.append`` with fetch (the N-point posterior is rebuilt on the device before every call, outside the timing);
  f  ``GP.append`` without fetch.
``chol_kernels_ms`` is the blocked Cholesky factorisation alone (all its block steps), between HIP events
(vbmc_last_kernel_ms(6)).  Every shape runs in a fresh child process under ``timeout -k 10 <--limit>`` (a hung device
call cannot be ended from inside its own interpreter); after a child that does not exit with 0 nothing further is
started and the tool exits with that status.  One JSON line per shape, collected by the parent and written to --out."""
import argparse
import json
import subprocess
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from pyvbmc_amd import _lib  # noqa: E402
from pyvbmc_amd import gp as gpm  # noqa: E402


def make_case(D, N, S, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N + 1, D))
    y = (-0.5 * np.sum(X**2, axis=1) + 0.05 * rng.standard_normal(N + 1)).reshape(-1, 1)
    hyp = np.array([np.concatenate([np.log(1.5 + rng.random(D)), [np.log(2.0 + 0.1 * s)], [np.log(0.05 + 0.01 * s)], [0.1],
                                    np.zeros(D), np.log(3.0) * np.ones(D)]) for s in range(S)])
    return X, y, hyp


def timed(fn, reps, warm, before=None):
    t = []
    for i in range(warm + reps):
        if before is not None:
            before()
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warm:
            t.append(dt)
    return round(statistics.median(t), 3), round(min(t), 3), round(max(t), 3)


SHAPES = ((10, 400, 1), (20, 800, 8))


def run_shape(D, N, S, reps, warm):
    """All rows of one shape in this process; prints the JSON line."""
    ctx = _lib.Context(0)
    _lib.set_default_context(ctx)
    X, y, hyp = make_case(D, N, S, 100 + S)
    gp = gpm.GP(D, gpm.SquaredExponential(), gpm.NegativeQuadratic(), gpm.GaussianNoise(constant_add=True))
    gp.ctx = ctx

    def build(n, device, fetch):
        gp.update(X[:n], y[:n], None, hyp, device=device, fetch=fetch)
        gpm.upload_gp(gp, ctx)

    def grow(fetch):
        gp.append(X[N], y[N, 0], fetch=fetch)
        gpm.upload_gp(gp, ctx)

    row = {"row": f"D{D}_N{N}_S{S}", "reps": reps, "warm": warm}
    for key, fn, before in (
        ("a_host_update_upload_ms", lambda: build(N, False, True), None),
        ("b_device_update_fetch_ms", lambda: build(N, True, True), None),
        ("c_device_update_nofetch_ms", lambda: build(N, True, False), None),
        ("d_host_update_n_plus_1_upload_ms", lambda: build(N + 1, False, True), None),
        ("e_append_fetch_ms", lambda: grow(True), lambda: build(N, True, True)),
        ("f_append_nofetch_ms", lambda: grow(False), lambda: build(N, True, False)),
    ):
        row[key], lo, hi = timed(fn, reps, warm, before)
        row[key.replace("_ms", "_min_max_ms")] = [lo, hi]
    ctx.set_timing(1)
    k = []
    for _ in range(warm + reps):
        build(N, True, False)
        k.append(ctx.last_kernel_ms(_lib.T_GP_POST))
    ctx.set_timing(0)
    row["chol_kernels_ms"] = round(statistics.median(k[warm:]), 4)
    row["c_lt_a"] = row["c_device_update_nofetch_ms"] < row["a_host_update_upload_ms"]
    row["f_lt_d"] = row["f_append_nofetch_ms"] < row["d_host_update_n_plus_1_upload_ms"]
    print(json.dumps(row), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--limit", type=int, default=180, help="seconds a shape's child process may take")
    ap.add_argument("--shape", type=int, default=None, help="(child) run shape number SHAPE in this process")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gp_post_rows.json"))
    a = ap.parse_args()
    if a.shape is not None:
        run_shape(*SHAPES[a.shape], a.reps, a.warm)
        return 0
    lines = []
    for i in range(len(SHAPES)):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, str(Path(__file__).resolve()), "--shape", str(i),
               "--reps", str(a.reps), "--warm", str(a.warm)]
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
