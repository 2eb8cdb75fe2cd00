#!/usr/bin/env python
"""Generate tests/golden/kde_mtv.npz by RUNNING THE REFERENCE's kde_1d and VariationalPosterior.mtv.  TEST
INFRASTRUCTURE, like tools/make_transform_golden.py: it runs only where the reference checkout is present
(REF below, or the VBMC_REFERENCE environment variable), imports it at run time and stores numbers only.

    python tools/make_mtv_golden.py        # rewrites tests/golden/kde_mtv.npz

The samples are not stored: tests/kde_host.py regenerates them from the same RandomState recipes.
kde cases (tests/kde_host.py KDE_CASES): bandwidth, len(np.unique), the Scott flag (whether the reference's
_root returned None) and the density, in full for FULL_DENSITY and every 16th point otherwise.  mtv cases
(MTV_CASES): the posteriors' parameters, each side's transformer fields, the NumPy seed set before the
call and the reference's output.
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("VBMC_REFERENCE", "/root/reference"))
sys.path.insert(0, str(ROOT / "oracle" / "_stubs"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(REF))

import importlib  # noqa: E402

import kde_host  # noqa: E402
from pyvbmc.parameter_transformer import ParameterTransformer  # noqa: E402
from pyvbmc.variational_posterior import VariationalPosterior  # noqa: E402

ref_kde = importlib.import_module("pyvbmc.stats.kde_1d")

OUT = ROOT / "tests" / "golden" / "kde_mtv.npz"


def _fields(pt, D):
    if pt is None:
        return {"type": np.zeros(D), "lb": np.full(D, -np.inf), "ub": np.full(D, np.inf), "mu": np.zeros(D),
                "delta": np.ones(D), "R": np.zeros(0), "scale": np.zeros(0), "identity": np.array(1)}
    return {"type": np.ravel(pt.type).astype(float), "lb": np.ravel(pt.lb_orig), "ub": np.ravel(pt.ub_orig),
            "mu": np.ravel(pt.mu), "delta": np.ravel(pt.delta),
            "R": np.zeros(0) if pt.R_mat is None else np.asarray(pt.R_mat, dtype=float),
            "scale": np.zeros(0) if pt.scale is None else np.ravel(pt.scale), "identity": np.array(0)}


def _ref_vp(D, K, spec, seed):
    pt = None
    if spec is not None and spec[0] != "identity":
        lb, ub, plb, pub, ttype, roto = kde_host.transformer_spec(spec[0], D, spec[1])
        R = scale = None
        if roto:  # non-trivial rotoscaling
            r = np.random.RandomState(seed + 77)
            R, _ = np.linalg.qr(r.randn(D, D))
            scale = np.exp(r.randn(D) * 0.2)
        pt = ParameterTransformer(D, lb.reshape(1, -1), ub.reshape(1, -1), plb.reshape(1, -1), pub.reshape(1, -1),
                                  scale=scale, rotation_matrix=R, transform_type=ttype)
    vp = VariationalPosterior(D, K, parameter_transformer=pt)
    vp.mu, vp.sigma, vp.lambd, vp.w = kde_host.mixture_params(D, K, seed)
    return vp, pt


def main():
    out = {}
    ref_root = ref_kde._root
    for name, (n, lo, hi) in kde_host.KDE_CASES.items():
        x = kde_host.kde_samples(name)
        seen = {}

        def spy(*a, **k):
            seen["t"] = ref_root(*a, **k)
            return seen["t"]

        ref_kde._root = spy
        try:
            dens, mesh, bw = ref_kde.kde_1d(x, n, lo, hi)
        finally:
            ref_kde._root = ref_root
        keep = dens if name in kde_host.FULL_DENSITY else dens[::16]
        out[f"kde_{name}_density"] = keep
        out[f"kde_{name}_mesh_ends"] = np.array([mesh[0], mesh[1], mesh[-1]])
        out[f"kde_{name}_bandwidth"] = np.ravel(bw).astype(float)
        out[f"kde_{name}_bw_is_array"] = np.array(int(isinstance(bw, np.ndarray) and bw.ndim > 0))
        out[f"kde_{name}_scott"] = np.array(int(seen["t"] is None))
        out[f"kde_{name}_nunique"] = np.array(np.unique(x).size)
    try:
        ref_kde.kde_1d(kde_host.kde_samples("constant"), 2**10)
        out["kde_constant_raises"] = np.array(0)
    except IndexError:
        out["kde_constant_raises"] = np.array(1)

    for name in kde_host.MTV_CASES:
        D, K, N, spec1, spec2, rows = kde_host.mtv_case(name)
        seed = 1000 + kde_host.hash_name(name) % 1000
        vp1, pt1 = _ref_vp(D, K, spec1, spec1[1])
        for k, v in _fields(pt1, D).items():
            out[f"mtv_{name}_pt1_{k}"] = v
        out[f"mtv_{name}_vp1"] = np.concatenate([vp1.mu.ravel(), vp1.sigma.ravel(), vp1.lambd.ravel(), vp1.w.ravel()])
        if rows:
            r = np.random.RandomState(seed + 5)
            samples = r.randn(rows, D) * 1.3 + 0.2
            np.random.seed(seed)
            val = vp1.mtv(samples=samples, N=N)
        else:
            vp2, pt2 = _ref_vp(D, K, spec2, spec2[1] + 50)
            for k, v in _fields(pt2, D).items():
                out[f"mtv_{name}_pt2_{k}"] = v
            out[f"mtv_{name}_vp2"] = np.concatenate([vp2.mu.ravel(), vp2.sigma.ravel(), vp2.lambd.ravel(),
                                                     vp2.w.ravel()])
            np.random.seed(seed)
            val = vp1.mtv(vp2, N=N)
        out[f"mtv_{name}_seed"] = np.array(seed)
        out[f"mtv_{name}_value"] = np.asarray(val, dtype=float)
        print(name, np.ravel(val)[:4], flush=True)
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
