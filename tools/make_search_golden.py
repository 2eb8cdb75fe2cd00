#!/usr/bin/env python
"""Generate tests/golden/search.npz by RUNNING THE REFERENCE's ``_get_search_points`` (vbmc/active_sample.py:647-837).
TEST INFRASTRUCTURE, like tools/make_mode_golden.py: it runs only where the reference checkout is present (that tool's
REF, or the VBMC_REFERENCE environment variable), imports it at run time and stores numbers only.

    python tools/make_search_golden.py        # rewrites tests/golden/search.npz

Per case: the inputs (mixture, logger arrays, caches, bounds, option values, transformer fields), the ``np.random`` seed
and the reference's ``search_X`` / ``idx_cache`` (or that it raised ``ValueError``).  tests/search_host.py ``load_case``
reads a case back.  The cases, at D = 3, K = 3, N = 37, number_of_points = 300 unless said:
  a  default fractions, empty cache, finite search bounds          e  N = 4, HPD on: rank-deficient covariances and the
  b  a 5-row cache, infinite search bounds (the plausible box)        empty-set fallback (round(0.1 * 4) == 0)
  c  a 200-row cache: more than ceil(300 * cache_frac), short output  f  D = 1, HPD on (the scalar covariance broadcast)
  d  search cache and HPD on, all six HPD fractions populated        g  fractions that sum above 1: ValueError
"""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

from make_mtv_golden import _fields  # noqa: E402  (puts the reference checkout and the stubs on sys.path)

from pyvbmc.parameter_transformer import ParameterTransformer  # noqa: E402
from pyvbmc.variational_posterior import VariationalPosterior  # noqa: E402
from pyvbmc.vbmc.active_sample import _get_search_points  # noqa: E402

OUT = ROOT / "tests" / "golden" / "search.npz"
OPTION_KEYS = ("cache_frac", "search_cache_frac", "heavy_tail_search_frac", "mvn_search_frac", "hpd_search_frac",
               "box_search_frac", "hpd_frac")
DEFAULTS = dict(cache_frac=0.5, search_cache_frac=0.0, heavy_tail_search_frac=0.25, mvn_search_frac=0.25,
                hpd_search_frac=0.0, box_search_frac=0.25, hpd_frac=0.8)
#        D  N   cache rows  finite bounds  option overrides
CASES = {
    "a": (3, 37, 0, True, {}),
    "b": (3, 37, 5, False, {}),
    "c": (3, 37, 200, True, {}),
    "d": (3, 37, 0, True, dict(search_cache_frac=0.125, heavy_tail_search_frac=0.125, mvn_search_frac=0.125,
                               hpd_search_frac=0.25, box_search_frac=0.125)),
    "e": (3, 4, 0, True, dict(hpd_search_frac=0.25, mvn_search_frac=0.125)),
    "f": (1, 37, 3, True, dict(hpd_search_frac=0.25, mvn_search_frac=0.125)),
    "g": (3, 37, 0, True, dict(heavy_tail_search_frac=0.5, mvn_search_frac=0.5, box_search_frac=0.25)),
}
K, NUMBER_OF_POINTS = 3, 300


def case_inputs(name):
    D, N, n_cache, finite, over = CASES[name]
    r = np.random.default_rng(1000 + ord(name))
    c = {"D": D, "K": K, "N": N, "number_of_points": NUMBER_OF_POINTS, "np_seed": 4200 + ord(name)}
    c["mu"] = 1.5 * r.standard_normal((D, K))
    c["sigma"] = np.array([[0.4, 0.6, 0.9]])
    lam = 0.5 + r.random((D, 1))
    c["lambd"] = lam / np.sqrt(np.sum(lam**2) / D)
    c["w"] = np.array([[0.2, 0.3, 0.5]])
    # the logger's arrays are longer than the evaluated part (X_flag)
    X = r.standard_normal((N + 5, D)) * 1.2
    c["X"] = X
    c["y"] = (-0.5 * np.sum(X**2, axis=1) + 0.1 * r.standard_normal(N + 5)).reshape(-1, 1)
    c["X_flag"] = np.arange(N + 5) < N
    c["pt_lb_orig"], c["pt_ub_orig"] = np.full((1, D), -10.0), np.full((1, D), 10.0)
    c["pt_plb"], c["pt_pub"] = np.full((1, D), -3.0), np.full((1, D), 3.0)
    c["x_orig"] = r.uniform(-8, 8, size=(n_cache, D))
    # (only case d takes rows from the search cache; it is the last thing drawn, so the other inputs do not depend on it)
    c["search_cache"] = 0.8 * r.standard_normal((50, D)) if over.get("search_cache_frac", 0) > 0 else np.zeros((0, D))
    c["lb_search"] = np.full((1, D), -1.6) if finite else np.full((1, D), -np.inf)
    c["ub_search"] = np.full((1, D), 1.9) if finite else np.full((1, D), np.inf)
    c["plb_tran"], c["pub_tran"] = np.full((1, D), -1.0), np.full((1, D), 1.0)
    opts = dict(DEFAULTS, **over)
    c["options"] = np.array([opts[k] for k in OPTION_KEYS])
    return c


def main():
    out = {}
    for name in CASES:
        c = case_inputs(name)
        D = c["D"]
        pt = ParameterTransformer(D, c["pt_lb_orig"], c["pt_ub_orig"], c["pt_plb"], c["pt_pub"])
        vp = VariationalPosterior(D, K, parameter_transformer=pt)
        vp.mu, vp.sigma, vp.lambd, vp.w = c["mu"].copy(), c["sigma"].copy(), c["lambd"].copy(), c["w"].copy()
        optim_state = {"cache": {"x_orig": c["x_orig"]}, "search_cache": c["search_cache"], "lb_search": c["lb_search"],
                       "ub_search": c["ub_search"], "plb_tran": c["plb_tran"], "pub_tran": c["pub_tran"]}
        flog = SimpleNamespace(X=c["X"], y=c["y"], X_flag=c["X_flag"], parameter_transformer=pt)
        options = dict(zip(OPTION_KEYS, c["options"].tolist()))
        np.random.seed(c["np_seed"])
        try:
            search_X, idx_cache = _get_search_points(c["number_of_points"], optim_state, flog, vp, options)
            raised = 0
        except ValueError:
            search_X, idx_cache, raised = np.zeros((0, D)), np.zeros(0), 1
        print(name, search_X.shape, idx_cache.shape, "raised" if raised else "", flush=True)
        for k, v in c.items():
            out[f"{name}_{k}"] = np.asarray(v)
        for k, v in _fields(pt, D).items():
            out[f"{name}_pt_{k}"] = v
        out[f"{name}_search_X"], out[f"{name}_idx_cache"], out[f"{name}_raised"] = search_X, idx_cache, np.array(raised)
    out["option_keys"] = np.array(OPTION_KEYS)
    out["cases"] = np.array(list(CASES))
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
