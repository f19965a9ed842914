"""The forces over neighbour rows from JavaScript.  Without a GPU: the addon exports listForce, the wrapper has
Simulation.prototype.listForce, and an uninitialised simulation answers with the usual "call init(particles) first" error.  On the GPU:
listForce() on plummer1024 -- at the bodies over neighborLists()' rows with their counts, at 300 points over knn()'s rows -- returns
the BYTES the Python binding returns for the same rows."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden32

NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_list_force_tests.js")
JS = os.path.join(ROOT, "nbody3d-webgpu_amd", "js")
ADDON = os.path.join(JS, "addon", "nb_napi.node")


def run(mode, *more):
    src = os.path.join(JS, "addon", "nb_napi.c")
    if not os.path.exists(ADDON) or os.path.getmtime(ADDON) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", JS, "-s"])
    p = subprocess.run([NODE, SCRIPT, mode] + [str(x) for x in more], capture_output=True, text=True, timeout=300)
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert line, "node produced no result: rc=%d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(line[-1])
    failed = {k: v for k, v in res["results"].items() if not v["pass"]}
    assert res["ok"] and p.returncode == 0, failed
    return res["results"]


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_list_force_surface_cpu():
    results = run("cpu")
    for k in ("addon_exports_listForce", "wrapper_has_listForce", "listForce_before_init_throws", "listForce_wants_a_handle"):
        assert results[k]["pass"]


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_list_force_returns_the_bytes_of_the_python_binding(tmp_path):
    from nbody3d_amd import Simulation
    results = run("gpu", tmp_path)
    for k in ("gpu_listForce_shapes", "gpu_listForce_defaults_to_accel", "gpu_listForce_range_error", "gpu_listForce_cap_range",
              "gpu_listForce_needs_pointVel", "gpu_listForce_jerk_needs_hermite", "gpu_listForce_leapfrog_has_the_same_bits"):
        assert results[k]["pass"]

    def js(name, dtype=np.float32):
        return np.frombuffer(open(os.path.join(str(tmp_path), name + ".bin"), "rb").read(), dtype)

    b, v = load_golden32("plummer1024_bodies0"), load_golden32("plummer1024_vel0")
    n = len(b)
    with Simulation(n, integrator="hermite4") as s:
        s.init(b, v)
        s.set_params(1e-3, 1.0)
        lists, count = s.neighbor_lists(bodies=(0, n), radius=0.25, cap=32)
        assert lists.tobytes() == js("lists", np.uint32).tobytes() and count.tobytes() == js("count", np.uint32).tobytes()
        assert 0 < count.mean() and (count > 0).sum() > n // 2            # the rows are not trivial
        a, j, phi = s.list_force(lists, bodies=(0, n), count=count, jerk=True, phi=True)
        assert a.tobytes() == js("own_accel").tobytes() and j.tobytes() == js("own_jerk").tobytes() and phi.tobytes() == js("own_phi").tobytes()
        pts, pv = js("points").reshape(-1, 4), js("point_vel").reshape(-1, 4)
        assert pts.shape == (300, 4)
        index, _ = s.knn(pts, k=16, dist2=False)
        assert index.tobytes() == js("knn_index", np.uint32).tobytes()
        a, j, phi = s.list_force(index, points=pts, point_vel=pv, jerk=True, phi=True)
        assert a.tobytes() == js("at_accel").tobytes() and j.tobytes() == js("at_jerk").tobytes() and phi.tobytes() == js("at_phi").tobytes()
        assert np.abs(a[:, :3]).max() > 0 and np.abs(j[:, :3]).max() > 0 and (phi < 0).all()
