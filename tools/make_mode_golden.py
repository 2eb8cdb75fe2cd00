#!/usr/bin/env python
"""Generate tests/golden/mode.npz by RUNNING THE REFERENCE's VariationalPosterior.mode.  TEST INFRASTRUCTURE,
like tools/make_mtv_golden.py: it runs only where the reference checkout is present (that tool's REF, or the
VBMC_REFERENCE environment variable), imports it at run time and stores numbers only.

    python tools/make_mode_golden.py        # rewrites tests/golden/mode.npz (several minutes)

Per case of tests/mode_host.py CASES the transformer's fields, and per case, per orig_flag and per NumPy seed
of mode_host.SEEDS: the reference's x, its log-density there (the reference's own pdf; may be NaN), its wall
time, the seed, and whether the reference raised (x and the log-density are NaN then).  The mixtures are not
stored: mode_host.case_mixture regenerates them.
"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

from make_mtv_golden import _fields  # noqa: E402  (puts the reference checkout and the stubs on sys.path)

import kde_host  # noqa: E402
import mode_host  # noqa: E402
from pyvbmc.parameter_transformer import ParameterTransformer  # noqa: E402
from pyvbmc.variational_posterior import VariationalPosterior  # noqa: E402

OUT = ROOT / "tests" / "golden" / "mode.npz"


def ref_vp(name):
    D, K, kind, seed, _ = mode_host.CASES[name]
    pt = None
    if kind != "identity":
        lb, ub, plb, pub, ttype, roto = kde_host.transformer_spec(kind, D, seed)
        R, scale = mode_host.rotoscale(D, seed) if roto else (None, None)
        pt = ParameterTransformer(D, lb.reshape(1, -1), ub.reshape(1, -1), plb.reshape(1, -1), pub.reshape(1, -1),
                                  scale=scale, rotation_matrix=R, transform_type=ttype)
    vp = VariationalPosterior(D, K, parameter_transformer=pt)
    vp.mu, vp.sigma, vp.lambd, vp.w = mode_host.case_mixture(name)
    return vp, pt


def main():
    out = {}
    for name in mode_host.CASES:
        D = mode_host.CASES[name][0]
        vp, pt = ref_vp(name)
        for k, v in _fields(pt, D).items():
            out[f"{name}_pt_{k}"] = v
        for orig in (0, 1):
            xs, fs, ts, raised = [], [], [], []
            for seed in mode_host.SEEDS:
                vp._mode = None
                np.random.seed(seed)
                t0 = time.perf_counter()
                try:
                    with np.errstate(all="ignore"):
                        x = np.asarray(vp.mode(orig_flag=bool(orig)), dtype=float).ravel()
                        f = float(np.ravel(vp.pdf(x, orig_flag=bool(orig), log_flag=True))[0])
                    r = 0
                except Exception as e:  # (D = 1 in the original space: AxisError)
                    print(name, orig, seed, "raised", type(e).__name__, flush=True)
                    x, f, r = np.full(D, np.nan), np.nan, 1
                ts.append(time.perf_counter() - t0)
                xs.append(x)
                fs.append(f)
                raised.append(r)
                print(name, orig, seed, f, round(ts[-1], 2), flush=True)
            out[f"{name}_o{orig}_x"] = np.array(xs)
            out[f"{name}_o{orig}_f"] = np.array(fs)
            out[f"{name}_o{orig}_time"] = np.array(ts)
            out[f"{name}_o{orig}_raised"] = np.array(raised)
        out[f"{name}_seeds"] = np.array(mode_host.SEEDS)
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
