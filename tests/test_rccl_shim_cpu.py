"""The stand-in collective library of tests/test_rccl_ranks_gpu.py, as far as a machine without a GPU can take it: its rank
groups (join, matched barriers, abort; tests/rccl_shim/shim_group.c has no HIP in it) run under a sanitizer in a program of
their own, and the HIP part and the worker at least compile.  Nothing here loads into Python."""
import os
import shutil
import subprocess

import pytest

import rccl_shim_build

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def test_rank_groups_under_a_sanitizer(tmp_path):
    """tests/c/shim_group_sanitize.c: 2, 3 and 4 threads through a thousand matched barriers with a late joiner; an abort, a
    rank that stops coming, ranks out of step and a rank that leaves each send every other rank home inside the cap."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "shim_group_sanitize")
    src = [os.path.join(ROOT, "tests", "c", "shim_group_sanitize.c"), os.path.join(ROOT, "tests", "rccl_shim", "shim_group.c")]
    ran = None
    for san in ("thread", "address,undefined"):
        cc = subprocess.run([gcc, "-std=c11", "-O1", "-g", "-fsanitize=" + san, "-fno-sanitize-recover=all", "-Wall", "-Wextra"] + src +
                            ["-o", exe, "-lpthread"], capture_output=True, text=True, timeout=300)
        if cc.returncode != 0 and any(w in cc.stderr for w in ("sanitize", "tsan", "asan")):
            continue                                  # this gcc does not link that runtime
        assert cc.returncode == 0, cc.stderr[-2000:]
        run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        if san == "thread" and run.returncode != 0 and "unexpected memory mapping" in run.stderr:
            continue                                  # the thread sanitizer's runtime cannot start under this kernel's address layout
        ran = san
        break
    if ran is None:
        pytest.skip("this gcc has no sanitizer runtime")
    print("sanitizer: " + ran)
    assert run.returncode == 0 and "ok shim groups under the sanitizer" in run.stdout, run.stdout[-1500:] + run.stderr[-3000:]
    assert run.stdout.count("ok matched barriers") == 3 and run.stdout.count("ok a rank") == 12, run.stdout


def test_the_library_and_the_worker_compile():
    """hipcc cross-compiles the HIP part for gfx950 without a GPU; the library exports the twelve entry points the engine resolves."""
    lib = rccl_shim_build.build(force=True)
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, timeout=60)
    assert nm.returncode == 0, nm.stderr
    have = {line.split()[-1] for line in nm.stdout.splitlines() if line.strip()}
    want = {"ncclGetUniqueId", "ncclCommInitRank", "ncclCommInitAll", "ncclCommDestroy", "ncclCommCount", "ncclCommUserRank", "ncclAllGather",
            "ncclReduceScatter", "ncclGroupStart", "ncclGroupEnd", "ncclGetErrorString", "ncclGetVersion"}
    assert want <= have, sorted(want - have)
    with open(os.path.join(ROOT, "tests", "rccl_shim", "rccl_shim.hip")) as f:
        text = f.read()
    assert "#define NB_SHIM_VERSION %d " % rccl_shim_build.VERSION in text and rccl_shim_build.VERSION < 20000
    assert "hipStreamSynchronize" not in text and "hipDeviceSynchronize" not in text      # collectives stay asynchronous
    worker = os.path.join(ROOT, "tests", "rccl_shim", "rccl_ranks_worker.py")
    with open(worker) as f:
        compile(f.read(), worker, "exec")
