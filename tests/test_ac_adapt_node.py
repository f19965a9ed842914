"""The neighbour scheme's radii that follow a target count and its checkpoint from JavaScript: the surface without a GPU, and on the GPU
the recorded recovery case through the wrapper -- the four calls, the stats, a checkpoint round trip that continues bit for bit, and the
first steps equal to the Python binding's bit for bit."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import ac_adapt_ref as A

NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_ac_adapt_tests.js")
JS = os.path.join(ROOT, "nbody3d-webgpu_amd", "js")
ADDON = os.path.join(JS, "addon", "nb_napi.node")
NAME = "recover256"


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
def test_node_adaptation_and_checkpoint_match_the_python_binding(tmp_path):
    from nbody3d_amd import Simulation
    e = A.record()["cases"][NAME]
    b0, v0 = A.fixture(e["fixture"])
    b0.tofile(str(tmp_path / "bodies0.f32"))
    v0.tofile(str(tmp_path / "vel0.f32"))
    params = dict(dt=e["dt"], G=e["G"], radius=e["radius"], cap=e["cap"], target=e["target"], substeps=A.SUBSTEPS, steps=A.STEPS)
    run_node("gpu", str(tmp_path), json.dumps(params))
    with Simulation(e["n"], eps2=1e-4, integrator="hermite4") as sim:       # the wrapper's default softening
        sim.init(b0, v0)
        sim.set_params(e["dt"], e["G"])
        sim.set_neighbor_scheme(radius=e["radius"], cap=e["cap"], substeps=A.SUBSTEPS)
        sim.set_neighbor_adapt(e["target"])
        sim.simulate(A.STEPS)
        b, v, a = sim.read()
        j, st, ad = sim.read_jerk(), sim.neighbor_scheme_stats(), sim.neighbor_adapt_stats()
        nxt = sim.download_neighbor_radii()[1]
    js = json.load(open(str(tmp_path / "stats.json")))
    assert (js["entries"], js["builds"], js["maxCount"], js["rebuilds"], js["rowsShrunk"], js["lastRebuilds"]) == \
        (st["entries"], st["builds"], st["max_count"], ad["rebuilds"], ad["rows_shrunk"], ad["last_rebuilds"])
    for name, want in (("bodies", b), ("vel", v), ("accel", a), ("jerk", j), ("next", nxt)):
        got = np.fromfile(str(tmp_path / (name + ".f32")), "<f4")
        assert got.tobytes() == want.tobytes(), name
