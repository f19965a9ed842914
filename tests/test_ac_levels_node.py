"""The neighbour scheme's block individual irregular steps from JavaScript: the surface without a GPU, and on the GPU a recorded
fixture with dynamic levels through the wrapper -- the four calls, the stats, the errors, a checkpoint round trip that continues
bit for bit, and the first steps equal to the Python binding's bit for bit."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import ac_ref as R

NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_ac_levels_tests.js")
JS = os.path.join(ROOT, "nbody3d-webgpu_amd", "js")
ADDON = os.path.join(JS, "addon", "nb_napi.node")
NAME, SUBSTEPS, MIN_LEVEL, ETA, STEPS = "plummer256", 8, 1, 0.02, 3


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
def test_node_levels_and_checkpoint_match_the_python_binding(tmp_path):
    from nbody3d_amd import Simulation
    e = R.record()["fixtures"][NAME]
    b0, v0 = R.fixture(NAME)
    b0.tofile(str(tmp_path / "bodies0.f32"))
    v0.tofile(str(tmp_path / "vel0.f32"))
    params = dict(dt=e["dt"], G=e["G"], radius=e["radius"], cap=e["cap"], substeps=SUBSTEPS, minLevel=MIN_LEVEL, eta=ETA, steps=STEPS)
    run_node("gpu", str(tmp_path), json.dumps(params))
    with Simulation(e["n"], eps2=1e-4, integrator="hermite4") as sim:       # the wrapper's default softening
        sim.init(b0, v0)
        sim.set_params(e["dt"], e["G"])
        sim.set_neighbor_scheme(radius=e["radius"], cap=e["cap"], substeps=SUBSTEPS)
        sim.set_neighbor_levels(min_level=MIN_LEVEL, eta=ETA)
        sim.download_neighbor_levels()                                    # (the script asks for the start's levels too: the same calls)
        sim.simulate(STEPS)
        b, v, a = sim.read()
        j, ls, lev = sim.read_jerk(), sim.neighbor_level_stats(), sim.download_neighbor_levels()
    js = json.load(open(str(tmp_path / "stats.json")))
    assert (js["regularSteps"], js["ticks"], js["blockSteps"], js["bodySteps"], js["entries"], js["clamped"], js["finestLevel"]) == \
        (ls["regular_steps"], ls["ticks"], ls["block_steps"], ls["body_steps"], ls["entries"], ls["clamped"], ls["finest_level"])
    for name, want in (("bodies", b), ("vel", v), ("accel", a), ("jerk", j)):
        got = np.fromfile(str(tmp_path / (name + ".f32")), "<f4")
        assert got.tobytes() == want.tobytes(), name
    assert np.fromfile(str(tmp_path / "levels.u8"), np.uint8).tobytes() == lev.tobytes()
