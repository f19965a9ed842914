"""Builds tests/rccl_shim/librccl_shim.so, the stand-in collective library of tests/test_rccl_ranks_gpu.py, when it is missing
or older than its sources.  Test-only: nothing in the product or in bench.py knows it."""
import os
import shutil
import subprocess

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rccl_shim")
SOURCES = [os.path.join(HERE, f) for f in ("rccl_shim.hip", "shim_group.c", "shim_group.h")]
LIB = os.path.join(HERE, "librccl_shim.so")
VERSION = 10203            # NB_SHIM_VERSION in rccl_shim.hip: what ncclGetVersion reports


def hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def build(force=False):
    """Path of the library; compiles it for gfx950 first if it is stale (hipcc cross-compiles without a GPU)."""
    if not force and os.path.exists(LIB) and os.path.getmtime(LIB) >= max(os.path.getmtime(s) for s in SOURCES):
        return LIB
    tmp = LIB + ".tmp%d" % os.getpid()       # linked under another name and renamed: nobody loads a half-written library
    obj = os.path.join(HERE, "shim_group.%d.o" % os.getpid())
    try:
        subprocess.check_call(["gcc", "-std=c11", "-O2", "-g", "-fPIC", "-Wall", "-Wextra", "-c", SOURCES[1], "-o", obj])
        subprocess.check_call([hipcc(), "-O2", "-g", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall", "-Wextra",
                               "-shared", "-o", tmp, obj, SOURCES[0], "-lpthread"])      # the object first: hipcc puts -x hip in front of the .hip file
        os.replace(tmp, LIB)
    finally:
        for f in (tmp, obj):
            if os.path.exists(f):
                os.remove(f)
    return LIB
