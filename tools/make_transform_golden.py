#!/usr/bin/env python
"""Generate tests/golden/transform.npz and transform_wide.npz by RUNNING THE REFERENCE's ParameterTransformer and
VariationalPosterior.  TEST INFRASTRUCTURE, like oracle/make_golden.py: it runs only where the
reference checkout is present (REF below, or the VBMC_REFERENCE environment variable), imports it at
run time and stores numbers only -- the transformers' fields, the points and the reference's outputs.

    python tools/make_transform_golden.py        # rewrites tests/golden/transform.npz and transform_wide.npz

Cases: one per bounded type (logit, probit, student4), a mixed case with unbounded dimensions and
plausible bounds (mu / delta not trivial), and a rotoscaled probit case (random orthogonal R_mat,
scale).  Points: inside, on the bounds, one ulp inside, outside, non-finite, and values whose unit-
interval image rounds to 0 or 1 (the nudges); u points include extremes that saturate z to 0 / 1.
The wide cases (WIDE below) add rows with 1e308, 1e200, -1e160 and -1e308 in unbounded dimensions, keep
them among the pdf points, and store pdf(..., grad_flag=True) for a few of them.
"""
import os
import sys
import warnings
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("VBMC_REFERENCE", "/root/reference"))
sys.path.insert(0, str(ROOT / "oracle" / "_stubs"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(REF))

from pyvbmc.parameter_transformer import ParameterTransformer  # noqa: E402
from pyvbmc.variational_posterior import VariationalPosterior  # noqa: E402

OUT = ROOT / "tests" / "golden" / "transform.npz"
OUT_WIDE = ROOT / "tests" / "golden" / "transform_wide.npz"
INF = np.inf

# name: (transform type, lb, ub, plb, pub, rotoscaled)
CASES = {
    "logit": ("logit", [0.0, -1e6, -3.0], [10.0, 10.0, 3.0], [1.0, -10.0, -2.0], [9.0, 5.0, 2.5], False),
    "probit": ("probit", [0.0, -1e6, -3.0], [10.0, 10.0, 3.0], [1.0, -10.0, -2.0], [9.0, 5.0, 2.5], False),
    "student4": ("student4", [0.0, -1e6, -3.0], [10.0, 10.0, 3.0], [1.0, -10.0, -2.0], [9.0, 5.0, 2.5], False),
    "mixed": ("logit", [-INF, 0.0, -INF, -5.0, 1.0], [INF, 2.0, INF, 5.0, 4.0],
              [-3.0, 0.5, 10.0, -4.0, 1.5], [1.0, 1.5, 30.0, 4.0, 3.0], False),
    "roto": ("probit", [-2.0, 0.0, -INF, 1.0], [2.0, 5.0, INF, 9.0], [-1.0, 1.0, -4.0, 2.0], [1.5, 4.0, 6.0, 8.0],
             True),
}

# transform_wide.npz, one case per padded width of the device kernels (2 .. 32) and both sides of the pairwise
# sum's switch at D = 8: name -> (D, transform type, rotoscaled).  "mixed3" gives the bounded dimensions the
# codes 3, 12, 13 in turn.  The names are tests/transform_host.py's WIDE_CASES.
WIDE = {
    "w1": (1, "logit", False),
    "w2": (2, "student4", True),
    "w6": (6, "probit", False),
    "w7": (7, "logit", True),
    "w8": (8, "probit", False),
    "w9": (9, "student4", True),
    "w12": (12, "logit", False),
    "w16": (16, "mixed3", False),
    "w17": (17, "probit", True),
    "w24": (24, "student4", False),
    "w25": (25, "logit", True),
    "w32": (32, "probit", True),
}
WIDE_GRAD = ("w1", "w9", "w16", "w32")  # cases that also store pdf(..., grad_flag=True)


def x_points(rng, lb, ub, plb, pub):
    D = lb.size
    fin = np.isfinite(lb) & np.isfinite(ub)
    lo = np.where(fin, lb, plb - 3 * (pub - plb))
    hi = np.where(fin, ub, pub + 3 * (pub - plb))
    rows = [lo + (hi - lo) * rng.random(D) for _ in range(24)]
    mid = np.where(fin, 0.5 * (lb + ub), 0.5 * (plb + pub))
    for d in range(D):
        if not fin[d]:
            continue
        for v in (lb[d], ub[d], np.nextafter(lb[d], INF), np.nextafter(ub[d], -INF), lb[d] - 1.0, ub[d] + 0.5,
                  lb[d] + 5e-324, lb[d] + 1e-300, ub[d] - 1e-12 * (ub[d] - lb[d])):
            r = mid.copy()
            r[d] = v
            rows.append(r)
    for v in (np.nan, INF, -INF, 1e308, -1e308):
        r = mid.copy()
        r[rng.integers(D)] = v
        rows.append(r)
    return np.array(rows)


def u_points(rng, u_in, D):
    rows = [u for u in u_in if np.all(np.isfinite(u))]
    for v in (40.0, -40.0, 800.0, -800.0, 1e4, -1e4, 1e300, -1e300, 0.0, 38.5, -38.5):
        r = np.zeros(D)
        r[rng.integers(D)] = v
        rows.append(r)
        rows.append(np.full(D, v))
    return np.array(rows)


def wide_case(rng, D, ttype, roto):
    """Bounds of a WIDE case: every third dimension (from the second) unbounded, the others bounded with
    random spans; plausible bounds strictly inside."""
    lb, ub = np.full(D, -INF), np.full(D, INF)
    plb, pub = np.empty(D), np.empty(D)
    for d in range(D):
        c, w = 4.0 * rng.standard_normal(), np.exp(rng.standard_normal())
        if D > 1 and d % 3 == 1:
            plb[d], pub[d] = c - w, c + w
        else:
            lb[d], ub[d] = c - 3 * w, c + 2 * w
            plb[d], pub[d] = lb[d] + 0.5 * w, ub[d] - 0.4 * w
    return (ttype, lb, ub, plb, pub, roto)


def make_pt(rng, D, lb, ub, plb, pub, ttype, roto):
    if ttype == "mixed3":
        # the reference's methods loop over bounded_types: per-dimension codes set after construction are
        # honoured once that list holds them and the per-type functions are set up again; mu / delta are then
        # recentred on the plausible bounds as the constructor does
        pt = ParameterTransformer(D, lb, ub, plb, pub, transform_type="logit")
        b = np.flatnonzero(pt.type)
        pt.type[b] = np.resize([3.0, 12.0, 13.0], b.size)
        pt.bounded_types = [3, 12, 13]
        pt._set_bounded_transforms()
        pt.mu, pt.delta = np.zeros(D), np.ones(D)
        lo, hi = pt(plb), pt(pub)
        fin = np.isfinite(lo[0]) & np.isfinite(hi[0])
        pt.mu[fin] = 0.5 * (lo[0, fin] + hi[0, fin])
        pt.delta[fin] = hi[0, fin] - lo[0, fin]
    else:
        pt = ParameterTransformer(D, lb, ub, plb, pub, transform_type=ttype)
    if roto:  # as a warp leaves it: rotation and scale set after the centring
        q, r = np.linalg.qr(rng.standard_normal((D, D)))
        pt.R_mat = q * np.sign(np.diag(r))
        pt.scale = np.exp(0.5 * rng.standard_normal(D))
    return pt


def extremes(lb, ub, plb, pub):
    """Rows with a huge coordinate in an unbounded dimension: the squared distance overflows, the density is 0."""
    fin = np.isfinite(lb) & np.isfinite(ub)
    with np.errstate(invalid="ignore"):
        mid = np.where(fin, 0.5 * (lb + ub), 0.5 * (plb + pub))
    rows = []
    for d in np.flatnonzero(~fin)[:2]:
        for v in (1e308, 1e200, -1e160, -1e308):
            r = mid.copy()
            r[d] = v
            rows.append(r)
    return np.array(rows).reshape(-1, lb.size)


def run_case(rng, out, name, spec, wide):
    ttype, lb, ub, plb, pub, roto = spec
    lb, ub, plb, pub = (np.array(v, dtype=np.float64).reshape(1, -1) for v in (lb, ub, plb, pub))
    D = lb.shape[1]
    pt = make_pt(rng, D, lb, ub, plb, pub, ttype, roto)
    with np.errstate(invalid="ignore"):
        x = x_points(rng, lb[0], ub[0], plb[0], pub[0])
    if wide:
        x = np.vstack([x, extremes(lb[0], ub[0], plb[0], pub[0])])
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        u_fwd = pt(x)
        inside = np.all(x > lb, axis=1) & np.all(x < ub, axis=1)
        u = u_points(rng, u_fwd[inside], D)
        x_inv = pt.inverse(u)
        ladj = pt.log_abs_det_jacobian(u)
        K = 3
        vp = VariationalPosterior(D, K, parameter_transformer=pt)
        vp.mu = 0.6 * rng.standard_normal((D, K))
        vp.sigma = np.exp(0.3 * rng.standard_normal((1, K))) * 0.7
        vp.lambd = np.exp(0.2 * rng.standard_normal((D, 1)))
        vp.w = rng.dirichlet(np.ones(K)).reshape(1, -1)
        vp.eta = np.log(vp.w)
        if wide:  # pdf points: every finite one, 1e308 / 1e200 coordinates in unbounded dimensions included
            xp = x[np.all(np.isfinite(x), axis=1)]
        else:
            # pdf points: finite, and no 1e308 coordinate in an unbounded dimension (its squared distance overflows;
            # kept as it was so that transform.npz does not change: transform_wide.npz holds such points)
            xp = x[np.all(np.isfinite(x) & (np.abs(x) < 1e300), axis=1)]
        for df in (0.0, 7.0):
            out[f"{name}_pdf_df{df:g}"] = vp.pdf(xp, orig_flag=True, df=df)
            out[f"{name}_logpdf_df{df:g}"] = vp.log_pdf(xp, orig_flag=True, df=df)
        if wide and name in WIDE_GRAD:
            out[f"{name}_pdf_g"], out[f"{name}_dpdf_g"] = vp.pdf(xp, orig_flag=True, grad_flag=True)
    out[f"{name}_type"] = np.asarray(pt.type, dtype=np.float64)
    out[f"{name}_lb"], out[f"{name}_ub"] = lb, ub
    out[f"{name}_mu"], out[f"{name}_delta"] = pt.mu, pt.delta
    out[f"{name}_R"] = pt.R_mat if pt.R_mat is not None else np.zeros((0, 0))
    out[f"{name}_scale"] = pt.scale if pt.scale is not None else np.zeros(0)
    out[f"{name}_x"], out[f"{name}_u_fwd"] = x, u_fwd
    out[f"{name}_u"], out[f"{name}_x_inv"], out[f"{name}_ladj"] = u, x_inv, ladj
    out[f"{name}_vp_mu"], out[f"{name}_vp_sigma"] = vp.mu, vp.sigma
    out[f"{name}_vp_lambd"], out[f"{name}_vp_w"] = vp.lambd, vp.w
    out[f"{name}_pdf_x"] = xp


def main():
    rng = np.random.default_rng(20261016)
    out = {"cases": np.array(list(CASES))}
    for name, spec in CASES.items():
        run_case(rng, out, name, spec, wide=False)
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes")

    rng = np.random.default_rng(20261017)
    out = {"cases": np.array(list(WIDE))}
    for name, (D, ttype, roto) in WIDE.items():
        run_case(rng, out, name, wide_case(rng, D, ttype, roto), wide=True)
    np.savez_compressed(OUT_WIDE, **out)
    print(OUT_WIDE, OUT_WIDE.stat().st_size, "bytes")

if __name__ == "__main__":
    main()
