#!/usr/bin/env python
"""Generate tests/golden/whitening.npz by RUNNING THE REFERENCE's ``unscent_warp``, ``warp_input`` and
``warp_gp_and_vp`` (whitening/whitening.py).  TEST INFRASTRUCTURE, like tools/make_search_golden.py: it runs only where
the reference checkout is present (tools/make_mtv_golden.py's REF, or the VBMC_REFERENCE environment variable), imports
it at run time with the stand-ins of oracle/_stubs and stores numbers only.

    python tools/make_whitening_golden.py        # rewrites tests/golden/whitening.npz

Per case: the mixture, the logger arrays, the GP's X and hyper-parameters, the option values, the old transformer's
fields (``old_*``) and the new one's (``new_*``), the ``np.random`` seed set before ``warp_input``, one ``np.random.rand()``
drawn after it (``next_draw``: where the global stream was left) and every output: the ``optim_state`` fields
``warp_input`` sets, the re-mapped X / y / search cache, ``hyp_warped`` and the warped mixture, and ``unscent_warp`` of the
mixture's (mu, sigma lambda) rows with its warped points.  The uniform box draws are not stored: a reader regenerates
them from the seed.  tests/whitening_host.py ``load_case`` reads a case back.

  a  D = 2   the reference's own MATLAB case (testing/whitening/test_rotoscaling.py and the tables next to it, stored here
             as ``matlab_*``): K = 50, an unbounded transformer, NegativeQuadratic; and its two-transformer unscent_warp
             example (``ua_*``)
  b  D = 3   K = 3, N = 37, S = 2, NegativeQuadratic; types 0 / 3 / 12; first warp (R_mat and scale None);
             warp_roto_corr_thresh 0.2, warp_cov_reg 0.1
  c  D = 3   K = 3, N = 37, S = 2, ConstantMean; types 0 / 13 / 3; second warp (the old transformer rotated and scaled);
             temperature 2; a search cache of 6 rows
  d  D = 32  K = 2, N = 5, S = 1, NegativeQuadratic; bounded codes 3, 12, 13 in turn; the old transformer rotated
"""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

from make_mtv_golden import REF, _fields  # noqa: E402  (puts the reference checkout and the stubs on sys.path)

import gpyreg  # noqa: E402  (oracle/_stubs)
from pyvbmc.parameter_transformer import ParameterTransformer  # noqa: E402
from pyvbmc.variational_posterior import VariationalPosterior  # noqa: E402
from pyvbmc.whitening import unscent_warp, warp_gp_and_vp, warp_input  # noqa: E402

OUT = ROOT / "tests" / "golden" / "whitening.npz"
TABLES = REF / "pyvbmc" / "testing" / "whitening"
INF = np.inf
STATE_KEYS = ("plb_tran", "pub_tran", "lb_search", "ub_search", "recompute_var_post", "skip_active_sampling",
              "warping_count", "last_warping", "last_successful_warping", "last_run_avg")

#        D   K  N   S  mean                 thresh cov_reg T  cache rows  old rotated
CASES = {
    "a": (2, 50, 0, 1, "NegativeQuadratic", 0.05, 0, None, 0, False),
    "b": (3, 3, 37, 2, "NegativeQuadratic", 0.2, 0.1, None, 0, False),
    "c": (3, 3, 37, 2, "ConstantMean", 0.05, 0, 2.0, 6, True),
    "d": (32, 2, 5, 1, "NegativeQuadratic", 0.05, 0, None, 0, True),
}


def table(name):
    return np.loadtxt(TABLES / name, delimiter=",")


def typed_pt(D, lb, ub, plb, pub, codes, rng, roto):
    """A transformer whose bounded dimensions take ``codes`` in turn (tools/make_transform_golden.py make_pt)."""
    pt = ParameterTransformer(D, lb, ub, plb, pub, transform_type="logit")
    b = np.flatnonzero(pt.type)
    pt.type[b] = np.resize(codes, b.size)
    pt.bounded_types = sorted(set(int(c) for c in codes))
    pt._set_bounded_transforms()
    pt.mu, pt.delta = np.zeros(D), np.ones(D)
    lo, hi = pt(plb), pt(pub)
    fin = np.isfinite(lo[0]) & np.isfinite(hi[0])
    pt.mu[fin] = 0.5 * (lo[0, fin] + hi[0, fin])
    pt.delta[fin] = hi[0, fin] - lo[0, fin]
    if roto:
        q, r = np.linalg.qr(rng.standard_normal((D, D)))
        pt.R_mat = q * np.sign(np.diag(r))
        pt.scale = np.exp(0.3 * rng.standard_normal(D))
    return pt


def case_inputs(name):
    D, K, N, S, mean, thresh, reg, T, n_cache, roto = CASES[name]
    r = np.random.default_rng(7000 + ord(name))
    c = {"D": D, "K": K, "S": S, "np_seed": 5200 + ord(name), "mean": mean, "thresh": thresh, "cov_reg": reg,
         "temperature": 0.0 if T is None else T, "iter": 7, "warping_count": 1 if roto else 0}
    if name == "a":
        angle = 1.309355600770139
        R = np.array([[np.cos(angle), np.sin(angle)], [-np.sin(angle), np.cos(angle)]])
        rands = table("test_warp_input_rands.txt")
        rands[:, 0] = 10 * rands[:, 0]
        mus = rands @ R
        vp = VariationalPosterior(D, K, mus)
        pt = vp.parameter_transformer
        gp_X, hyp = table("test_warp_gp_and_vp_gp_X.txt"), np.atleast_2d(table("test_warp_gp_and_vp_gp_hyps.txt"))
        c["plb_orig"], c["pub_orig"] = np.full((1, D), -10.0), np.full((1, D), 10.0)
    else:
        if name == "b":
            lb, ub, codes = np.array([[-INF, 0.0, -3.0]]), np.array([[INF, 10.0, 3.0]]), [3.0, 12.0]
        elif name == "c":
            lb, ub, codes = np.array([[-INF, 0.0, -3.0]]), np.array([[INF, 10.0, 3.0]]), [13.0, 3.0]
        else:
            lb, ub = np.full((1, D), -INF), np.full((1, D), INF)
            lb[0, 1::2], ub[0, 1::2] = -2.0 - r.random(D // 2), 3.0 + r.random(D // 2)
            codes = [3.0, 12.0, 13.0]
        fin = np.isfinite(lb)
        mid, half = np.where(fin, 0.5 * (np.where(fin, lb, 0) + np.where(fin, ub, 0)), 0.5), np.where(fin, 1.0, 2.0)
        plb, pub = mid - half, mid + half
        c["plb_orig"], c["pub_orig"] = plb, pub
        pt = typed_pt(D, lb, ub, plb, pub, codes, r, roto)
        vp = VariationalPosterior(D, K, parameter_transformer=pt)
        vp.mu = 0.8 * r.standard_normal((D, K))
        vp.sigma = (0.3 + 0.5 * r.random((1, K)))
        lam = 0.5 + r.random((D, 1))
        vp.lambd = lam / np.sqrt(np.sum(lam**2) / D)
        w = 0.2 + r.random((1, K))
        vp.w = w / np.sum(w)
        gp_X = 0.9 * r.standard_normal((N, D))
        P = D + 1 + 1 + (1 if mean == "ConstantMean" else 1 + 2 * D)
        hyp = 0.3 * r.standard_normal((S, P))
        if mean == "NegativeQuadratic":
            hyp[:, D + 3:D + 3 + D] = 0.5 * r.standard_normal((S, D))
    # the logger's arrays are longer than the evaluated part (X_flag)
    n_log = gp_X.shape[0]
    X_inf = np.vstack([gp_X, np.zeros((4, D))])
    c["X_flag"] = np.arange(n_log + 4) < n_log
    c["X_orig"] = pt.inverse(X_inf)
    c["y_orig"] = (-0.5 * np.sum(X_inf**2, axis=1) + 0.1 * r.standard_normal(n_log + 4)).reshape(-1, 1)
    c["X"], c["y"] = X_inf.copy(), c["y_orig"] + pt.log_abs_det_jacobian(X_inf).reshape(-1, 1)
    c["lb_search"], c["ub_search"] = np.full((1, D), -1.4) - 0.2 * r.random((1, D)), np.full((1, D), 1.2) + 0.2 * r.random((1, D))
    c["search_cache"] = 0.7 * r.standard_normal((n_cache, D))
    c["gp_X"], c["hyp"] = gp_X, hyp
    c["mu"], c["sigma"], c["lambd"], c["w"] = vp.mu.copy(), vp.sigma.copy(), vp.lambd.copy(), vp.w.copy()
    return c, vp, pt


def stub_gp(D, mean, X, hyp):
    gp = gpyreg.GP(D, gpyreg.covariance_functions.SquaredExponential(), getattr(gpyreg.mean_functions, mean)(),
                   gpyreg.noise_functions.GaussianNoise(constant_add=True))
    gp.X = X
    gp.posteriors = [SimpleNamespace(hyp=h.copy()) for h in hyp]
    return gp


def main():
    out = {}
    # the reference test's two-transformer unscent_warp example and its MATLAB answers (test_rotoscaling.py:43-132)
    a1, a2 = np.pi / 6.6, np.pi / 3
    R1 = np.array([[np.cos(a1), np.sin(a1)], [-np.sin(a1), np.cos(a1)]])
    R2 = np.array([[np.cos(a2), np.sin(a2)], [-np.sin(a2), np.cos(a2)]])
    p1 = ParameterTransformer(2, rotation_matrix=R1, scale=np.array([0.9, 0.7]))
    p2 = ParameterTransformer(2, rotation_matrix=R2, scale=np.array([1.2, 0.5]))
    sigma = np.array([3.0, 0.7])
    mu = np.array([[1.2, -3.3], [-1.7, 0.5], [-3.4, -np.pi], [5.01, 9.8]])
    muw, sigmaw, muu = unscent_warp(lambda x: p2(p1.inverse(np.copy(x))), mu, sigma)
    for k, v in _fields(p1, 2).items():
        out[f"ua_old_{k}"] = v
    for k, v in _fields(p2, 2).items():
        out[f"ua_new_{k}"] = v
    out.update(ua_x=mu, ua_sigma=sigma, ua_mean=muw, ua_sd=sigmaw, ua_pts=muu)
    out["matlab_ua_mean"] = np.array([[1.79786175315009, -2.71880715597597], [-1.23028515945097, -1.06548342843230],
                                      [-1.15442046351576, -7.00874808879672], [0.0703468098253310, 16.4174973622584]])
    out["matlab_ua_sd"] = np.tile([1.90565079837152, 3.03363336606057], (4, 1))
    m1 = [1.7979, -1.2303, -1.1544, 0.0703, 4.4747, 1.4466, 1.5224, 2.7472, -0.879, -3.9071, -3.8313, -2.6065, 1.4857,
          -1.5425, -1.4666, -0.2419, 2.1101, -0.9181, -0.8422, 0.3826]
    m2 = [-2.7188, -1.0655, -7.0087, 16.4175, 1.4099, 3.0633, -2.8800, 20.5462, -6.8475, -5.1942, -11.1375, 12.2888,
          -1.5529, 0.1004, -5.8428, 17.5834, -3.8847, -2.2314, -8.1747, 15.2516]
    out["matlab_ua_pts"] = np.array(list(zip(m1, m2))).reshape([5, 4, 2])
    # the MATLAB tables of the reference's warp_input / warp_gp_and_vp tests (case a's known answers)
    for key, f in (("R_mat", "test_warp_input_R_mat.txt"), ("scale", "test_warp_input_scale.txt"),
                   ("hyp_warped", "test_warp_gp_and_vp_gp_hyps_new.txt"), ("vp_mu", "test_warp_gp_and_vp_vp_mu.txt"),
                   ("vp_w", "test_warp_gp_and_vp_vp_w.txt"), ("vp_sigma", "test_warp_gp_and_vp_vp_sigma.txt"),
                   ("vp_lambda", "test_warp_gp_and_vp_vp_lambda.txt")):
        out[f"matlab_a_{key}"] = np.atleast_2d(table(f))

    for name in CASES:
        c, vp, pt = case_inputs(name)
        D = c["D"]
        T = c["temperature"]
        state = {"plb_orig": c["plb_orig"], "pub_orig": c["pub_orig"], "lb_search": c["lb_search"], "ub_search": c["ub_search"],
                 "search_cache": c["search_cache"].tolist(), "warping_count": c["warping_count"], "iter": c["iter"], "N": 0,
                 "run_mean": [1.0], "run_cov": [1.0], "last_run_avg": 3.0}
        if T:
            state["temperature"] = T
        flog = SimpleNamespace(X=c["X"].copy(), y=c["y"].copy(), X_orig=c["X_orig"], y_orig=c["y_orig"], X_flag=c["X_flag"],
                               parameter_transformer=pt)
        options = {"warp_rotoscaling": True, "warp_nonlinear": False, "warp_roto_corr_thresh": c["thresh"],
                   "warp_cov_reg": c["cov_reg"]}
        np.random.seed(c["np_seed"])
        new_pt, state2, flog2, action = warp_input(vp, state, flog, options)
        next_draw = np.random.rand()
        assert action == "rotoscale" and state2["run_mean"] == [] and state2["run_cov"] == []
        gp = stub_gp(D, c["mean"], c["gp_X"], c["hyp"])
        vbmc = SimpleNamespace(D=D, optim_state=state2)
        vp2, hyp_warped = warp_gp_and_vp(new_pt, gp, vp, vbmc)

        def warpfun(x):
            return new_pt(pt.inverse(x))

        un = unscent_warp(warpfun, vp.mu.T, (vp.lambd * vp.sigma).T)
        print(name, "R", new_pt.R_mat.shape, "hyp_warped", hyp_warped.shape, flush=True)
        for k, v in c.items():
            out[f"{name}_{k}"] = np.asarray(v)
        for k, v in _fields(pt, D).items():
            out[f"{name}_old_{k}"] = v
        for k, v in _fields(new_pt, D).items():
            out[f"{name}_new_{k}"] = v
        for k in STATE_KEYS:
            out[f"{name}_out_{k}"] = np.asarray(state2[k], dtype=np.float64)
        out[f"{name}_out_search_cache"] = np.asarray(state2["search_cache"], dtype=np.float64).reshape(-1, D)
        out[f"{name}_out_X"], out[f"{name}_out_y"], out[f"{name}_next_draw"] = flog2.X, flog2.y, np.array(next_draw)
        out[f"{name}_hyp_warped"] = hyp_warped
        out[f"{name}_vp_mu"], out[f"{name}_vp_sigma"] = vp2.mu, vp2.sigma
        out[f"{name}_vp_lambd"], out[f"{name}_vp_w"] = vp2.lambd, vp2.w
        out[f"{name}_un_mean"], out[f"{name}_un_sd"], out[f"{name}_un_pts"] = un
    out["cases"] = np.array(list(CASES))
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
