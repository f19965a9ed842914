"""The sums and the neighbour rows from one pass, from JavaScript.  Without a GPU: the addon exports splitLists and
neighborSchemeFused, the wrapper has Simulation.prototype.splitLists, and an uninitialised simulation answers with the usual "call
init(particles) first" error.  On the GPU: splitLists() on plummer1024 with a Hermite simulation -- at the bodies with one radius, at
300 points with a radius each (0 included) -- returns the BYTES the Python binding returns for the same request, and
neighborSchemeFused() answers as the Python property does."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden32

NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_split_lists_tests.js")
JS = os.path.join(ROOT, "nbody3d-webgpu_amd", "js")
ADDON = os.path.join(JS, "addon", "nb_napi.node")
NAMES = ("accel_irr", "accel_reg", "jerk_irr", "jerk_reg", "list", "count")
CAP = 24


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
def test_node_split_lists_surface_cpu():
    results = run("cpu")
    for k in ("addon_exports_splitLists", "wrapper_has_splitLists", "splitLists_before_init_throws", "splitLists_wants_a_handle"):
        assert results[k]["pass"]


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_split_lists_returns_the_bytes_of_the_python_binding(tmp_path):
    from nbody3d_amd import Simulation
    results = run("gpu", tmp_path)
    for k in ("gpu_splitLists_shapes", "gpu_splitLists_without_the_jerk", "gpu_splitLists_range_error", "gpu_splitLists_needs_a_radius",
              "gpu_splitLists_needs_pointVel", "gpu_splitLists_cap_range", "gpu_no_scheme_is_not_fused", "gpu_scheme_is_fused",
              "gpu_two_calls_flag_is_not_fused", "gpu_splitLists_jerk_needs_hermite", "gpu_splitLists_leapfrog_defaults_to_accel"):
        assert results[k]["pass"]

    def js(name, dtype=np.float32):
        return np.frombuffer(open(os.path.join(str(tmp_path), name + ".bin"), "rb").read(), dtype)

    b, v = load_golden32("plummer1024_bodies0"), load_golden32("plummer1024_vel0")
    n = len(b)
    with Simulation(n, integrator="hermite4") as s:
        s.init(b, v)
        s.set_params(1e-3, 1.0)
        own = s.split_lists(bodies=(0, n), radius=0.25, cap=CAP)
        for name in NAMES:
            assert own[name].tobytes() == js("own_" + name).tobytes(), name
        assert np.abs(own["accel_irr"][:, :3]).max() > 0 and np.abs(own["accel_reg"][:, :3]).max() > 0 and own["count"].max() > CAP > own["count"].min()
        pts, pv, radii = js("points").reshape(-1, 4), js("point_vel").reshape(-1, 4), js("radii")
        assert pts.shape == (300, 4) and radii.shape == (300,)
        at = s.split_lists(pts, point_vel=pv, radii=radii, cap=CAP)
        for name in NAMES:
            assert at[name].tobytes() == js("at_" + name).tobytes(), name
        assert not at["count"][radii == 0].any() and at["count"][radii > 0.3].any()
