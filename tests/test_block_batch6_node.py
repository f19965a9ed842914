"""Batched block steps on order-6 handles from JavaScript, on the GPU: one frozen outer step at N = 77 through the wrapper's
setBlockBatch6 / blockBatchStats gives the bits and the counters the Python binding gives with the same configuration (depth 8,
small_max 64)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import block6_ref as R

NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_block_batch6_tests.js")
JS = os.path.join(ROOT, "nbody3d-webgpu_amd", "js")
ADDON = os.path.join(JS, "addon", "nb_napi.node")
CAMEL = dict(host_waits="hostWaits", slots="slots", small_steps="smallSteps", host_steps="hostSteps", idle_slots="idleSlots")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_block_batch6_matches_the_python_binding_bit_for_bit(tmp_path):
    from nbody3d_amd import Simulation
    src = os.path.join(JS, "addon", "nb_napi.c")
    if not os.path.exists(ADDON) or os.path.getmtime(ADDON) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", JS, "-s"])
    n = 77
    b0, v0, lev0, _ = R.frozen_ref(n)
    b0.tofile(str(tmp_path / "bodies0.f32"))
    v0.tofile(str(tmp_path / "vel0.f32"))
    lev0.tofile(str(tmp_path / "levels0.u8"))
    p = subprocess.run([NODE, SCRIPT, str(tmp_path)], capture_output=True, text=True, timeout=300)
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert line, "node produced no result: rc=%d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(line[-1])
    assert res["ok"] and p.returncode == 0, {k: v for k, v in res["results"].items() if not v["pass"]}
    with Simulation(n, eps2=1e-4, integrator="hermite4") as sim:       # the wrapper's default softening
        sim.set_hermite_order(6)
        sim.init(b0, v0)
        sim.set_block_steps6(max_level=R.L_FROZEN, frozen=True)
        sim.set_block_batch6(depth=8, small_max=64)
        sim.upload_levels(lev0)
        sim.simulate(1, R.DT_FROZEN, 1.0)
        b, v, a = sim.read()
        j, (s, c), lev, st, bs = sim.read_jerk(), sim.read_snap(), sim.read_levels(), sim.block_stats(), sim.block_batch_stats()
    js = json.load(open(str(tmp_path / "stats.json")))
    jb = json.load(open(str(tmp_path / "batch.json")))
    assert js["bodySteps"] == st["body_steps"] and js["blockSteps"] == st["block_steps"] == 8 and js["finestLevel"] == st["finest_level"], (js, st)
    assert js["clamped"] == st["clamped"] == 0 and js["outerSteps"] == 1
    assert jb["enabled"] is True and all(jb[c_] == bs[k] for k, c_ in CAMEL.items()), (jb, bs)
    assert bs["small_steps"] > 0 and bs["host_steps"] >= 1, bs
    assert np.fromfile(str(tmp_path / "levels.u8"), np.uint8).tobytes() == lev.tobytes() == lev0.tobytes()
    for name, arr in (("bodies", b), ("vel", v), ("accel", a), ("jerk", j), ("snap", s), ("crackle", c)):
        got = np.fromfile(str(tmp_path / (name + ".f32")), "<f4").reshape(-1, 4)
        assert got.tobytes() == arr.tobytes(), name
