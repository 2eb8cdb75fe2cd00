#!/usr/bin/env python
"""Record tests/golden/train_gp.npz FROM THE REFERENCE's functions.  TEST INFRASTRUCTURE, our own code.

    python tools/train_gp_golden.py <path to the reference tree>

Calls the reference's ``_get_gp_training_options``, ``_get_hyp_cov`` and ``_gp_hyp``
(pyvbmc/vbmc/gaussian_process_train.py) on the plain dicts of tests/train_gp_cases.py and stores what they return: data
only.  The reference imports with oracle/_stubs standing in for its third-party packages, as oracle/make_golden.py runs
it.  gpyreg is not part of the reference tree, so the GP handed to ``_gp_hyp`` is a subclass of the stand-in GP, defined
here, whose ``get_bounds`` / ``set_bounds`` / ``get_priors`` / ``set_priors`` keep the name-keyed dicts as they are given, and
whose covariance, mean and noise objects answer ``get_bounds_info`` with THIS PACKAGE'S rule (pyvbmc_amd/gp.py) -- the
inputs of ``_gp_hyp``'s decisions, not part of them.  Needs the reference tree, so it never runs with the test-suite or
on a GPU machine; the committed .npz is what the tests read (tests/test_train_gp_host.py)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]


def flat(v, n):
    return np.array(np.broadcast_to(np.ravel(np.asarray(v, dtype=np.float64)), (n,)))


def main(ref):
    sys.path[:0] = [str(ROOT / "oracle" / "_stubs"), str(ROOT), str(ROOT / "tests"), str(ref)]
    import gpyreg as gpr
    import train_gp_cases as tc
    from pyvbmc.vbmc import gaussian_process_train as ref_gpt

    from pyvbmc_amd import gp as pkg

    ours = {gpr.covariance_functions.SquaredExponential: pkg.SquaredExponential(), gpr.mean_functions.ZeroMean: pkg.ZeroMean(),
            gpr.mean_functions.ConstantMean: pkg.ConstantMean(), gpr.mean_functions.NegativeQuadratic: pkg.NegativeQuadratic(),
            gpr.noise_functions.GaussianNoise: pkg.GaussianNoise(constant_add=True)}
    for cls, obj in ours.items():
        cls.get_bounds_info = (lambda o: lambda self, X, y: o.get_bounds_info(X, y))(obj)

    class DictGP(gpr.GP):
        def blocks(self):
            return pkg._hyp_blocks(self.D, {0: 0, 1: 1, 2: 1 + 2 * self.D}[self.mean.kind])

        def get_bounds(self):
            return getattr(self, "_b", {nm: (np.full(n, -np.inf), np.full(n, np.inf)) for nm, _, n in self.blocks()})

        def set_bounds(self, b):
            self._b = dict(b)

        def get_priors(self):
            return getattr(self, "_p", {nm: None for nm, _, _ in self.blocks()})

        def set_priors(self, p):
            self._p = dict(p)

    out = {}
    for name, (st, hist, opts, hd, s_N) in tc.training_option_cases().items():
        cov = ref_gpt._get_hyp_cov(st, hist, opts, hd)
        out[f"cov/{name}"] = np.zeros(0) if cov is None else np.asarray(cov, dtype=np.float64)
        for k, v in ref_gpt._get_gp_training_options(st, hist, opts, hd, s_N).items():
            out[f"opt/{name}/{k}"] = np.array(v) if isinstance(v, str) else np.zeros(0) if v is None else np.asarray(v, dtype=np.float64)
    means = {"zero": gpr.mean_functions.ZeroMean, "const": gpr.mean_functions.ConstantMean,
             "negquad": gpr.mean_functions.NegativeQuadratic}
    for name, (st, opts, noisy) in tc.gp_hyp_cases().items():
        X, y, _ = tc.data(noisy)
        gp = DictGP(tc.D, gpr.covariance_functions.SquaredExponential(), means[st["gp_mean_fun"]](),
                    gpr.noise_functions.GaussianNoise(constant_add=True, user_provided_add=noisy))
        gp, hyp0, s_N = ref_gpt._gp_hyp(st, opts, tc.PLB, tc.PUB, gp, X, y)
        out[f"hyp/{name}/hyp0"], out[f"hyp/{name}/gp_s_N"] = np.asarray(hyp0, dtype=np.float64), np.array(float(s_N))
        for nm, _, n in gp.blocks():
            lo, hi = gp._b[nm]
            out[f"hyp/{name}/lb/{nm}"], out[f"hyp/{name}/ub/{nm}"] = flat(lo, n), flat(hi, n)
            spec = gp._p[nm]
            out[f"hyp/{name}/prior/{nm}"] = np.zeros((0, n)) if spec is None else np.stack([flat(v, n) for v in spec[1]])
            out[f"hyp/{name}/prior_kind/{nm}"] = np.array("none" if spec is None else spec[0])
    dst = ROOT / "tests" / "golden" / "train_gp.npz"
    np.savez_compressed(dst, **out)
    print(f"{dst}: {len(out)} arrays, {dst.stat().st_size} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(Path(sys.argv[1]))
