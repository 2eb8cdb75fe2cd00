"""INTEGRATION.md section 2's run-time patch, applied verbatim to a stand-in for the reference module.

The reference is not part of the repository: its module ``pyvbmc.vbmc.variational_optimization`` is a stand-in
here, the parameter lists of the four callables the patch replaces are the reference's own, stored by
oracle/make_golden.py (tests/golden/integration.npz), and the reference's kind of objects are tests/helpers.py's
attribute-only ``PlainVP`` and the gpyreg stand-in in oracle/_stubs.  tools/check_integration_patch.py runs the
same patch against the actual reference, its ``_sieve`` and ``optimize_vp`` where a reference checkout exists."""
import ast
import inspect
import re
import sys
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("entmc_vbmc", "entlb_vbmc", "_gp_log_joint", "_neg_elcbo")


def _stand_in_reference(monkeypatch):
    """Empty ``pyvbmc``, ``pyvbmc.vbmc`` and ``pyvbmc.vbmc.variational_optimization`` modules: the leaf names the
    reference binds at import, and nothing else."""
    mods = {}
    for name in ("pyvbmc", "pyvbmc.vbmc", "pyvbmc.vbmc.variational_optimization"):
        mods[name] = types.ModuleType(name)
        mods[name].__path__ = []
        monkeypatch.setitem(sys.modules, name, mods[name])
    mods["pyvbmc"].vbmc = mods["pyvbmc.vbmc"]
    vo = mods["pyvbmc.vbmc"].variational_optimization = mods["pyvbmc.vbmc.variational_optimization"]
    for name in NAMES:
        setattr(vo, name, None)
    return vo


def test_runtime_patch_resolves_and_accepts_reference_objects(monkeypatch, golden):
    vo = _stand_in_reference(monkeypatch)

    # 1. the patch, verbatim from the document
    doc = (ROOT / "INTEGRATION.md").read_text()
    m = re.search(r"at run time:\s*```python\n(.*?)```", doc, re.S)
    assert m, "INTEGRATION.md: run-time patch block not found"
    exec(compile(m.group(1), "INTEGRATION.md#runtime-patch", "exec"), {})

    import pyvbmc_amd
    import pyvbmc_amd.variational_optimization as avo
    from pyvbmc_amd import _lib, synthetic

    assert vo.entmc_vbmc is pyvbmc_amd.entmc_vbmc and vo.entlb_vbmc is pyvbmc_amd.entlb_vbmc
    assert vo._gp_log_joint is avo._gp_log_joint and vo._neg_elcbo is avo._neg_elcbo

    # 2. every patched callable takes the reference's positional parameters: names, order, defaults
    g = golden("integration")
    for name in NAMES:
        ps = [p for p in inspect.signature(getattr(vo, name)).parameters.values() if p.kind != p.KEYWORD_ONLY]
        assert [p.name for p in ps] == list(g[f"{name}_params"]), name
        for p, has, ref in zip(ps, g[f"{name}_has_default"], g[f"{name}_defaults"]):
            assert (p.default is not p.empty) == bool(has), (name, p.name)
            if has:
                assert p.default == ast.literal_eval(str(ref)), (name, p.name, p.default, ref)

    # 3. the reference's kind of objects reach the device boundary: a host-only context uploads the mixture (every
    # attribute read of vp) and fingerprints the GP for real, then the first launch refuses with NoDeviceError --
    # not an AttributeError on a member the reference's classes do not have
    monkeypatch.syspath_prepend(str(ROOT / "oracle" / "_stubs"))
    import gpyreg as gpr
    from helpers import PlainVP

    from oracle import mixture_ref

    wl = synthetic.make_workload(1)
    vp = PlainVP(mixture_ref.Mixture.make(wl.mu, wl.sigma, wl.lambd, wl.w, wl.eta))
    gp = gpr.GP(D=wl.D, covariance=gpr.covariance_functions.SquaredExponential(),
                mean=gpr.mean_functions.NegativeQuadratic(),
                noise=gpr.noise_functions.GaussianNoise(constant_add=True))
    gp.update(X_new=wl.X, y_new=wl.y, hyp=wl.hyp)
    bnd = synthetic.default_theta_bnd(wl)
    calls = {
        "_neg_elcbo (as optimize_vp calls it)": lambda: vo._neg_elcbo(wl.theta.copy(), gp, vp, 0.0, wl.NsK, True, False, bnd),
        "_neg_elcbo (as _sieve calls it)": lambda: vo._neg_elcbo(wl.theta.copy(), gp, vp, 0.0, 0, False, False, bnd),
        "_neg_elcbo (as _eval_full_elcbo calls it)": lambda: vo._neg_elcbo(wl.theta.copy(), gp, vp, 0.0, wl.NsK, False, True,
                                                                           None, 0.0, True),
        "_gp_log_joint": lambda: vo._gp_log_joint(vp, gp, True, True, True, False, False),
        "entmc_vbmc": lambda: vo.entmc_vbmc(vp, wl.NsK),
        "entlb_vbmc": lambda: vo.entlb_vbmc(vp),
    }
    prev, ctx = _lib._default_ctx, _lib.Context(-1)
    _lib.set_default_context(ctx)  # the reference's objects carry no context: the default one is used
    try:
        for what, call in calls.items():
            try:
                call()
            except _lib.NoDeviceError:
                continue
            raise AssertionError(f"{what}: returned from a host-only context -- a CPU fallback crept in")
    finally:
        _lib.set_default_context(prev)
        ctx.close()
