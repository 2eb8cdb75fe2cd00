#!/usr/bin/env python
"""A whole inference with no PyVBMC installed (needs an MI355X and the built library): a correlated 2-D normal in a box.

    vbmc_demo.py [checkpoint.pkl]

With a path the run writes a checkpoint at the end of every iteration; started again with the same path after it was
killed, it goes on from the file and ends where the uninterrupted run would have ended, bit for bit.  (The target is a
function of this module, which is what the checkpoint names: a lambda would need dill.)"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pyvbmc_amd import VBMC  # noqa: E402

P, MEAN = np.linalg.inv(np.array([[1.0, 0.6], [0.6, 0.5]])), np.array([0.5, -0.25])  # lnZ = 0


def log_density(x):
    return float(-0.5 * (np.ravel(x) - MEAN) @ P @ (np.ravel(x) - MEAN) - np.log(2 * np.pi) + 0.5 * np.log(np.linalg.det(P)))


checkpoint = Path(sys.argv[1]) if len(sys.argv) > 1 else None
if checkpoint is not None and checkpoint.exists():
    vbmc = VBMC.load(checkpoint)
    if vbmc.is_finished:  # (optimize() would go on past the budget: VBMC.load(..., new_options=...) is the way to extend it)
        sys.exit("%s holds a finished run of %d iterations; remove it to start again" % (checkpoint, vbmc.iteration + 1))
    print("resuming after iteration %d (%d evaluations)" % (vbmc.iteration, vbmc.function_logger.func_count))
else:
    box = [np.full((1, 2), v) for v in (-10.0, 10.0, -2.0, 2.0)]  # hard bounds, then the plausible box
    vbmc = VBMC(log_density, np.zeros((1, 2)), *box, {"warp_rotoscaling": False, "max_fun_evals": 80}, seed=0)
vp, results = vbmc.optimize(checkpoint=checkpoint)
print("elbo %.3f +- %.3f, mean" % (results["elbo"], results["elbo_sd"]), vp.moments(rng="philox", seed=1).ravel(), results["timings"])
print(vp.marginals(rng="philox", seed=2))  # the credible intervals per dimension (the numbers vp.plot() draws)
