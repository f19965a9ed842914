"""The neighbour query from JavaScript without a GPU: the addon exports neighbors, the wrapper has Simulation.prototype.neighbors and
closePairs, and an uninitialised simulation answers with the usual "call init(particles) first" error.  (The GPU half runs from
tests/test_neighbors_gpu.py.)"""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_neighbors_tests.js")
JS = os.path.join(ROOT, "nbody3d-webgpu_amd", "js")
ADDON = os.path.join(JS, "addon", "nb_napi.node")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_neighbors_surface_cpu():
    src = os.path.join(JS, "addon", "nb_napi.c")
    if not os.path.exists(ADDON) or os.path.getmtime(ADDON) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", JS, "-s"])
    p = subprocess.run([NODE, SCRIPT, "cpu"], capture_output=True, text=True, timeout=300)
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert line, "node produced no result: rc=%d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(line[-1])
    failed = {k: v for k, v in res["results"].items() if not v["pass"]}
    assert res["ok"] and p.returncode == 0, failed
    for k in ("addon_exports_neighbors", "wrapper_has_neighbors", "wrapper_has_closePairs", "neighbors_before_init_throws",
              "closePairs_before_init_throws", "mutual_pairs_logic"):
        assert res["results"][k]["pass"]
