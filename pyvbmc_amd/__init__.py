"""pyvbmc_amd -- MI355X-native (gfx950) implementation of PyVBMC's ELBO-evaluation
hot path, behind the reference's own Python names.

    from pyvbmc_amd import VariationalPosterior, entmc_vbmc, entlb_vbmc
    from pyvbmc_amd.variational_optimization import _neg_elcbo, _gp_log_joint
    pyvbmc_amd.patch()        # or: route the reference's own module through all of it (pyvbmc_amd/dropin.py)

Host code is plain Python calling hand-written HIP kernels through the C ABI of
libvbmc_hip.so (include/vbmc_hip.h) via ctypes.  No PyTorch, no CPU fallback.
"""
from .active_importance_sampling import (  # noqa: F401
    active_importance_sampling,
    active_sample_proposal_pdf,
    fess,
    get_mcmc_opts,
    renormalize_weights,
)
from .active_search import get_search_points, refine, search  # noqa: F401
from . import whitening  # noqa: F401
from .dropin import patch, patch_active_sampling, unpatch, unpatch_active_sampling  # noqa: F401  (pyvbmc_amd.patch(vo): the whole drop-in in one call)
from .dropin import patch_whitening, unpatch_whitening  # noqa: F401
from .dropin import patch_active_sample_loop, unpatch_active_sample_loop  # noqa: F401
from .dropin import patch_sieve, unpatch_sieve  # noqa: F401
from . import sieve  # noqa: F401
from .dropin import patch_optimize_vp, unpatch_optimize_vp  # noqa: F401
from .optimize_vp import optimize_vp  # noqa: F401
from .dropin import patch_train_gp, unpatch_train_gp  # noqa: F401
from .gaussian_process_train import train_gp  # noqa: F401
from .entropy import entlb_vbmc, entmc_vbmc  # noqa: F401
from .gp import GP, append_point, log_marginal_likelihood, reupdate  # noqa: F401
from .variational_posterior import VariationalPosterior  # noqa: F401
from .active_sample import active_sample  # noqa: F401
from .parameter_transformer import ParameterTransformer  # noqa: F401
from .function_logger import FunctionLogger  # noqa: F401
from .options import Options  # noqa: F401
from . import driver_rules  # noqa: F401
from .vbmc import VBMC  # noqa: F401  (the inference loop over the stages above: no PyVBMC needed)

__all__ = ["VariationalPosterior", "entmc_vbmc", "entlb_vbmc", "patch", "unpatch", "active_importance_sampling",
           "active_sample_proposal_pdf", "fess", "get_mcmc_opts", "renormalize_weights", "patch_active_sampling",
           "unpatch_active_sampling", "GP", "log_marginal_likelihood", "get_search_points", "search", "refine",
           "whitening", "patch_whitening", "unpatch_whitening", "active_sample", "append_point", "reupdate",
           "patch_active_sample_loop", "unpatch_active_sample_loop", "sieve", "patch_sieve", "unpatch_sieve",
           "optimize_vp", "patch_optimize_vp", "unpatch_optimize_vp", "train_gp", "patch_train_gp", "unpatch_train_gp",
           "VBMC", "Options", "FunctionLogger", "ParameterTransformer", "driver_rules"]
