"""The neighbour lists from JavaScript.  Without a GPU: the addon exports neighborLists, the wrapper has
Simulation.prototype.neighborLists, and an uninitialised simulation answers with the usual "call init(particles) first" error.  On
the GPU: an N = 1,025 lattice at cap 16 (truncating) and 128 against a double loop in JavaScript."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_neighbor_lists_tests.js")
JS = os.path.join(ROOT, "nbody3d-webgpu_amd", "js")
ADDON = os.path.join(JS, "addon", "nb_napi.node")


def run(mode):
    src = os.path.join(JS, "addon", "nb_napi.c")
    if not os.path.exists(ADDON) or os.path.getmtime(ADDON) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", JS, "-s"])
    p = subprocess.run([NODE, SCRIPT, mode], capture_output=True, text=True, timeout=300)
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert line, "node produced no result: rc=%d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(line[-1])
    failed = {k: v for k, v in res["results"].items() if not v["pass"]}
    assert res["ok"] and p.returncode == 0, failed
    return res["results"]


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_neighbor_lists_surface_cpu():
    results = run("cpu")
    for k in ("addon_exports_neighborLists", "wrapper_has_neighborLists", "neighborLists_before_init_throws"):
        assert results[k]["pass"]


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_neighbor_lists_on_the_gpu():
    results = run("gpu")
    for k in ("gpu_lists_cap16_vs_double_loop", "gpu_lists_cap128_vs_double_loop", "gpu_lists_cap16_truncates_and_cap128_does_not",
              "gpu_lists_points_vs_double_loop", "gpu_lists_count_is_the_neighbors_count"):
        assert results[k]["pass"]
