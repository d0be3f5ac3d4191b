"""Build liblfr_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

One object per source under csrc/_obj (rebuilt when the source or any header is newer), compiled in
parallel, then linked: an edit of one source recompiles that file alone, and the forward kernels
(lfr_solve.hip, the longest compile by far) only when they or a header change.  At most MAX_JOBS
compilers run at a time where that is set, and never more than 16.
"""
import glob
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(_HERE))
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
OBJ = os.path.join(CSRC, "_obj")
SOURCES = ["lfr_wire.cpp", "lfr_graph.cpp", "lfr_treeplan.cpp", "lfr_devctx.cpp", "lfr_solve.hip", "lfr_batch.hip", "lfr_backward.hip",
           "lfr_covariance.hip", "lfr_inputs.hip", "lfr_evaluate.hip", "lfr_jvp.hip", "lfr_hessian_product.hip", "lfr_hessian_solve.hip", "lfr_assemble.hip", "lfr_graphstage.hip", "lfr_graphbuild.hip"]
OUT = os.path.join(_HERE, "liblfr_hip.so")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.sep not in c or os.path.exists(c)):
            return c
    return "hipcc"


def _flags():
    return ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
            "-munsafe-fp-atomics",          # hardware fp64 atomic add for the HBM-matrix kernel
            "-I", os.path.join(ROOT, "include"), "-I", CSRC] + os.environ.get("LFR_HIPCC_FLAGS", "").split()


def _jobs():
    try:
        n = int(os.environ.get("MAX_JOBS", ""))
    except ValueError:
        n = os.cpu_count() or 1
    return max(1, min(n, 16))


def _header_mtime():
    deps = glob.glob(os.path.join(CSRC, "*.hpp")) + [os.path.join(ROOT, "include", "lfr.h")]     # every header: none can be forgotten
    return max(os.path.getmtime(d) for d in deps)


def _stale_objects(force):
    flags_tag = " ".join(_flags())
    tag_path = os.path.join(OBJ, "flags.txt")
    old_tag = open(tag_path).read() if os.path.exists(tag_path) else None
    ht = _header_mtime()
    stale = []
    for f in SOURCES:
        src, obj = os.path.join(CSRC, f), os.path.join(OBJ, f + ".o")
        if force or old_tag != flags_tag or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), ht):
            stale.append((src, obj))
    return stale, flags_tag, tag_path


def needs_build():
    if not os.path.exists(OUT):
        return True
    stale, _, _ = _stale_objects(False)
    if stale:
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.getmtime(os.path.join(OBJ, f + ".o")) > t for f in SOURCES)


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 -> lfr_amd/liblfr_hip.so.  Returns the path."""
    if not force and not needs_build():
        return OUT
    os.makedirs(OBJ, exist_ok=True)
    stale, flags_tag, tag_path = _stale_objects(force)

    def compile_one(pair):
        src, obj = pair
        cmd = [_hipcc()] + _flags() + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=max(1, min(len(stale), _jobs()))) as ex:
        list(ex.map(compile_one, stale))
    open(tag_path, "w").write(flags_tag)
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + [os.path.join(OBJ, f + ".o") for f in SOURCES] + ["-o", OUT]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return OUT
