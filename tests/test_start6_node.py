"""The start mode of order-6 handles from JavaScript: the surface without a GPU, and on the GPU the setter, the getter and the
crackle of a 257-body start through the wrapper, which gives the bits the Python binding gives."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import hermite6_ref as H6

NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_start6_tests.js")
JS = os.path.join(ROOT, "nbody3d-webgpu_amd", "js")
ADDON = os.path.join(JS, "addon", "nb_napi.node")


def run_node(*args):
    src = os.path.join(JS, "addon", "nb_napi.c")
    if not os.path.exists(ADDON) or os.path.getmtime(ADDON) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", JS, "-s"])
    p = subprocess.run([NODE, SCRIPT] + list(args), capture_output=True, text=True, timeout=300)
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert line, "node produced no result: rc=%d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(line[-1])
    assert res["ok"] and p.returncode == 0, {k: v for k, v in res["results"].items() if not v["pass"]}
    return res


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_surface():
    res = run_node("cpu")
    for k in ("addon_exports_setStart6", "wrapper_has_setStart6", "setStart6_before_init_throws", "setStart6_wants_a_handle"):
        assert res["results"][k]["pass"], k


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_start6_matches_the_python_binding_bit_for_bit(tmp_path):
    from nbody3d_amd import Simulation
    n = 257
    b0, v0 = H6.system(n)
    b0.tofile(str(tmp_path / "bodies0.f32"))
    v0.tofile(str(tmp_path / "vel0.f32"))
    res = run_node("gpu", str(tmp_path))
    for k in ("default_mode_is_0", "default_crackle_is_0", "bad_mode_is_an_argument_error", "setter_returns_the_simulation", "snap_is_shared",
              "order_4_returns_the_mode_to_0", "setStart6_at_order_4_is_a_state_error", "setStart6_on_leapfrog_is_a_state_error"):
        assert res["results"][k]["pass"], k
    with Simulation(n, eps2=1e-4, integrator="hermite6") as sim:       # the wrapper's default softening
        sim.init(b0, v0)
        sim.set_params(2.0 ** -6, 1.0)
        sim.set_start6(1)
        s, c = sim.read_snap()
    assert c[:, :3].any()
    for name, arr in (("snap", s), ("crackle", c)):
        got = np.fromfile(str(tmp_path / (name + ".f32")), "<f4").reshape(-1, 4)
        assert got.tobytes() == arr.tobytes(), name
