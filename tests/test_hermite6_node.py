"""The 6th-order Hermite scheme from JavaScript.  Without a GPU: the addon exports setHermiteOrder / hermiteOrder / downloadSnap /
uploadDerivs6 and the wrapper has setHermiteOrder, hermiteOrder, readSnap and uploadDerivs6.  On the GPU: 5 steps of 2^-6 at N = 257
at order 6 through the wrapper give the bits the Python binding gives, a checkpoint of six arrays continues bit for bit, and the
calls that do not apply are NB_ERR_STATE."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import hermite6_ref as R

NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_hermite6_tests.js")
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
    failed = {k: v for k, v in res["results"].items() if not v["pass"]}
    assert res["ok"] and p.returncode == 0, failed
    return res["results"]


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_hermite6_surface_cpu():
    res = run_node("cpu")
    for k in ("addon_exports_setHermiteOrder", "addon_exports_hermiteOrder", "addon_exports_downloadSnap", "addon_exports_uploadDerivs6",
              "wrapper_has_setHermiteOrder", "wrapper_has_hermiteOrder", "wrapper_has_readSnap", "wrapper_has_uploadDerivs6"):
        assert res[k]["pass"]


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_hermite6_matches_the_python_binding_bit_for_bit(tmp_path):
    from nbody3d_amd import Simulation
    b0, v0 = R.system(257)
    b0.tofile(str(tmp_path / "bodies0.f32"))
    v0.tofile(str(tmp_path / "vel0.f32"))
    res = run_node("gpu", str(tmp_path))
    for k in ("restore_with_derivs6_continues_bit_identically", "variant_is_hermite6", "crackle_is_zero_after_the_start",
              "readSnap_at_order_4_is_a_state_error", "setHermiteOrder_on_leapfrog_is_a_state_error", "uploadDerivs_at_order_6_is_a_state_error"):
        assert res[k]["pass"], k
    with Simulation(257, eps2=1e-4, integrator="hermite6") as sim:       # the wrapper's default softening (nbody3d.js:234)
        sim.init(b0, v0)
        sim.simulate(5, R.H, 1.0)
        b, v, a = sim.read()
        j = sim.read_jerk()
        s, c = sim.read_snap()
    for name, arr in (("bodies", b), ("vel", v), ("accel", a), ("jerk", j), ("snap", s), ("crackle", c)):
        got = np.fromfile(str(tmp_path / (name + ".f32")), "<f4").reshape(-1, 4)
        assert got.tobytes() == arr.tobytes(), name
