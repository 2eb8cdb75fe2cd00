"""Build recipe for libvbmc_hip.so and the tests' probe library libvbmc_devprobe.so (gfx950 only, in-tree).

    python -m pyvbmc_amd.build           # rebuild if sources are newer
    python -m pyvbmc_amd.build --force

hipcc cross-compiles without a GPU; the resulting .so is git-ignored but travels
to the GPU box with the working-tree snapshot.
"""
import os
import subprocess
import sys
import sysconfig
from pathlib import Path

HERE = Path(__file__).resolve().parent
CSRC = HERE / "csrc"
LIB = HERE / "libvbmc_hip.so"
SOURCES = [
    "ctx.hip",
    "entropy.hip",
    "entropy_small.hip",
    "prep.hip",
    "api_entropy.hip",
    "mixture.hip",
    "gp.hip",
    "api_gp.hip",
    "gp_post.hip",
    "api_gp_post.hip",
    "gp_lml.hip",
    "api_gp_lml.hip",
    "lockstep.hip",
    "gp_hyp.hip",
    "api_gp_hyp.hip",
    "gp_opt.hip",
    "api_gp_opt.hip",
    "gp_fit.hip",
    "api_gp_fit.hip",
    "api_elbo.hip",
    "api_batch.hip",
    "adam.hip",
    "adam_fused.hip",
    "api_acq.hip",
    "api_acq_is.hip",
    "acq_is_prep.hip",
    "acq_is_mcmc.hip",
    "search.hip",
    "api_search.hip",
    "sieve.hip",
    "api_sieve.hip",
    "elcbo_full.hip",
    "api_elcbo_full.hip",
    "cmaes.hip",
    "api_cmaes.hip",
    "sample.hip",
    "transform.hip",
    "kde.hip",
    "marginals.hip",
    "api_marginals.hip",
    "mode.hip",
    "warp.hip",
    "api_warp.hip",
    "comm.hip",
    "host_randn.hip",
    "device_randn.hip",
]
# Test infrastructure, a shared object of its own: entry points that run one fastmath.h primitive per thread
# (tests/test_fastmath_gpu.py).  Same FLAGS, so the primitives compile as they do inside the kernels.
PROBE_SRC = CSRC / "devprobe.hip"
PROBE_LIB = HERE / "libvbmc_devprobe.so"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# The native repeat lane of _neg_elcbo: a CPython extension (host C++ only) next to the library
STEP_DEPS = [CSRC / "pyext_step.cpp", CSRC / "step_lane.h"]
STEP_LIB = HERE / ("_step_native" + (sysconfig.get_config_var("EXT_SUFFIX") or ".so"))
HOST_CXX = os.environ.get("CXX", "c++")
FLAGS = [
    "--offload-arch=gfx950",
    "-O3",
    "-std=c++17",
    "-fPIC",
    "-ffp-contract=off",  # explicit fma() only: keep the arithmetic reproducible
    "-Wall",
    "-Wno-unused-function",
    # a kernel that misses its __launch_bounds__ occupancy ("failed to meet occupancy target": one more register array in a
    # rider path once cost the headline entropy kernel its second wave per SIMD, silently) or a "#pragma unroll" the
    # compiler does not honour fails the build
    "-Werror=pass-failed",
]


WS_DPS = [2, 4, 6, 8, 10, 12, 16, 20, 24, 32]  # must match VBMC_WS_DPS in entropy_args.h
MFMA_DPS = [12, 16, 20, 24, 32]  # padded D of the entropy kernel's matrix-pipe form (entropy_mfma.hip), one object each
WS_EXTRA = os.environ.get("VBMC_WS_EXTRA_FLAGS", "").split()  # experiments on the entropy kernel only
ALL_EXTRA = os.environ.get("VBMC_EXTRA_FLAGS", "").split()    # experiments: flags for every translation unit


def _sources():
    return [CSRC / s for s in SOURCES if (CSRC / s).exists()]


SOURCE_FLAGS = {}  # per-source extra flags (file name -> list)


def _jobs(bdir):
    """(source, object, extra flags) for every translation unit; the wave-split entropy
    kernel is compiled once per padded D so the instantiations build in parallel."""
    jobs = [(src, bdir / (src.stem + ".o"), list(ALL_EXTRA) + SOURCE_FLAGS.get(src.name, [])) for src in _sources()]
    for dp in WS_DPS:
        jobs.append((CSRC / "entropy_ws.hip", bdir / f"entropy_ws_dp{dp}.o", [f"-DVBMC_DP={dp}"] + WS_EXTRA))
    for dp in MFMA_DPS:
        jobs.append((CSRC / "entropy_mfma.hip", bdir / f"entropy_mfma_dp{dp}.o", [f"-DVBMC_MFMA_DP={dp}"] + ALL_EXTRA))
    return jobs


def _headers():
    return [h for h in CSRC.glob("*.h") if h not in STEP_DEPS] + [HERE.parent / "include" / "vbmc_hip.h"]


def _stale(lib, deps):
    return not lib.exists() or any(p.stat().st_mtime > lib.stat().st_mtime for p in deps)


def _lib_stale():
    return _stale(LIB, _sources() + [CSRC / "entropy_ws.hip", CSRC / "entropy_mfma.hip"] + _headers())


def _probe_stale():
    return _stale(PROBE_LIB, [PROBE_SRC] + _headers())


def _step_stale():
    return _step_buildable() and _stale(STEP_LIB, STEP_DEPS)


def needs_build():
    return _lib_stale() or _probe_stale() or _step_stale()


def _step_includes():
    import numpy

    return [sysconfig.get_paths()["include"], numpy.get_include()]


def _step_buildable():
    """The extension needs a host C++ compiler and the headers of this interpreter and of NumPy."""
    import shutil

    py, npy = (Path(p) for p in _step_includes())
    return bool(shutil.which(HOST_CXX)) and (py / "Python.h").exists() and (npy / "numpy" / "arrayobject.h").exists()


def build_step(verbose=True):
    """The native repeat lane of _neg_elcbo (csrc/pyext_step.cpp), a CPython extension next to the library.  Without a
    host compiler or the headers it is left out: variational_optimization then keeps its Python repeat path."""
    if not _step_buildable():
        print(f"{STEP_LIB.name}: no host C++ compiler or no Python / NumPy headers; the Python repeat path stays",
              file=sys.stderr, flush=True)
        return None
    cmd = [HOST_CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall",
           *(f"-I{p}" for p in _step_includes()), str(STEP_DEPS[0]), "-o", str(STEP_LIB)]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return STEP_LIB


def build_probe(verbose=True):
    cmd = [HIPCC, *FLAGS, *ALL_EXTRA, "-shared", str(PROBE_SRC), "-o", str(PROBE_LIB), "-Wl,-rpath,/opt/rocm/lib"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return PROBE_LIB


def build(force=False, verbose=True):
    if force or _probe_stale():
        build_probe(verbose)
    if force or _step_stale():
        build_step(verbose)
    if not force and not _lib_stale():
        return LIB
    objs = []
    procs = []
    bdir = CSRC / "_obj"
    bdir.mkdir(exist_ok=True)
    import concurrent.futures as cf

    def run(job):
        src, obj, extra = job
        cmd = [HIPCC, *FLAGS, *extra, "-c", str(src), "-o", str(obj)]
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        return obj, p

    jobs = _jobs(bdir)
    with cf.ThreadPoolExecutor(max_workers=max(2, (os.cpu_count() or 4))) as ex:
        results = list(ex.map(run, jobs))
    for (src, obj, _), (_, p) in zip(jobs, results):
        objs.append(obj)
        procs.append((obj, p))
    failed = False
    for src, p in procs:
        out = p.stdout
        if p.returncode != 0:
            failed = True
            sys.stderr.write(f"--- {src.name} failed ---\n{out.decode()}\n")
        elif verbose and out.strip():
            sys.stderr.write(out.decode())
    if failed:
        raise RuntimeError("hipcc failed")
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", *map(str, objs), "-o", str(LIB),
           "-ldl", "-Wl,-rpath,/opt/rocm/lib"]  # librccl is dlopen'ed lazily (csrc/comm.hip)
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
    print(PROBE_LIB)
    print(STEP_LIB)
