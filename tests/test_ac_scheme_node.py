"""The Ahmad-Cohen neighbour scheme from JavaScript: the surface without a GPU, and on the GPU one recorded fixture through the wrapper --
the start equals splitForce(), the trajectory holds the bound of tests/test_ac_scheme_gpu.py and equals the Python binding bit for
bit, an overflow is an NB_4 error."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import ac_ref as R

NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_ac_scheme_tests.js")
JS = os.path.join(ROOT, "nbody3d-webgpu_amd", "js")
ADDON = os.path.join(JS, "addon", "nb_napi.node")
NAME, NS = "plummer256", 8


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
def test_node_surface_without_a_gpu():
    run_node("cpu")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_neighbor_scheme_matches_the_restatement_and_the_python_binding(tmp_path):
    from nbody3d_amd import Simulation
    e = R.record()["fixtures"][NAME]
    b0, v0 = R.fixture(NAME)
    b0.tofile(str(tmp_path / "bodies0.f32"))
    v0.tofile(str(tmp_path / "vel0.f32"))
    params = dict(dt=e["dt"], G=e["G"], radius=e["radius"], cap=e["cap"], substeps=NS, steps=R.STEPS)
    run_node("gpu", str(tmp_path), json.dumps(params))
    with Simulation(e["n"], eps2=1e-4, integrator="hermite4") as sim:       # the wrapper's default softening
        sim.init(b0, v0)
        sim.set_params(e["dt"], e["G"])
        sim.set_neighbor_scheme(radius=e["radius"], cap=e["cap"], substeps=NS)
        sim.simulate(R.STEPS)
        b, v, a = sim.read()
        j, st = sim.read_jerk(), sim.neighbor_scheme_stats()
    js = json.load(open(str(tmp_path / "stats.json")))
    run = e["runs"][str(NS)]
    assert (js["entries"], js["builds"], js["maxCount"]) == (st["entries"], st["builds"], st["max_count"]) == (run["entries"], run["builds"], run["last_max_count"])
    ref = R.recorded_state(NAME, NS)
    for name, arr, q, want in zip(("bodies", "vel", "accel", "jerk"), (b, v, a, j), R.QUANTITIES, ref):
        got = np.fromfile(str(tmp_path / (name + ".f32")), "<f4").reshape(-1, 4)
        assert R.norm_err(got[:, :3], want) <= 8 * run["f32_err"][q], name
        assert got.tobytes() == arr.tobytes(), name
