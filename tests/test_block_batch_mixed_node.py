"""Batched block steps on mixed-precision handles from JavaScript, on the GPU: one frozen outer step at N = 77 of an f64 'hermite4'
simulation with setPassPrecision('mixed') through the wrapper's setBlockBatchMixed / blockBatchStats, on and off, gives the bits
and the counters the Python binding gives with the same configuration (depth 8, small_max 64)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from block6_ref import frozen_levels

NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_block_batch_mixed_tests.js")
JS = os.path.join(ROOT, "nbody3d-webgpu_amd", "js")
ADDON = os.path.join(JS, "addon", "nb_napi.node")
CAMEL = dict(host_waits="hostWaits", slots="slots", small_steps="smallSteps", host_steps="hostSteps", idle_slots="idleSlots")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_block_batch_mixed_matches_the_python_binding_bit_for_bit(tmp_path):
    from nbody3d_amd import Simulation, ic
    src = os.path.join(JS, "addon", "nb_napi.c")
    if not os.path.exists(ADDON) or os.path.getmtime(ADDON) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", JS, "-s"])
    n = 77
    b0, v0 = [np.array(z, np.float64) for z in ic.plummer(n, seed=21)]
    b0[:, :3] += 1e-9                                           # float64 rows that binary32 does not hold: the lo words are in play
    lev0 = frozen_levels(n)
    b0.tofile(str(tmp_path / "bodies0.f64"))
    v0.tofile(str(tmp_path / "vel0.f64"))
    lev0.tofile(str(tmp_path / "levels0.u8"))
    p = subprocess.run([NODE, SCRIPT, str(tmp_path)], capture_output=True, text=True, timeout=300)
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert line, "node produced no result: rc=%d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(line[-1])
    assert res["ok"] and p.returncode == 0, {k: v for k, v in res["results"].items() if not v["pass"]}
    with Simulation(n, precision="f64", eps2=1e-4, integrator="hermite4") as sim:       # the wrapper's default softening
        sim.init(b0, v0)
        sim.set_block_steps(max_level=3, frozen=True)
        sim.set_pass_precision("mixed")
        sim.set_block_batch_mixed(depth=8, small_max=64)
        sim.upload_levels(lev0)
        sim.simulate(1, 2.0 ** -4, 1.0)
        b, v, a = sim.read()
        j, lev, st, bs = sim.read_jerk(), sim.read_levels(), sim.block_stats(), sim.block_batch_stats()
    js = json.load(open(str(tmp_path / "stats.json")))
    jb = json.load(open(str(tmp_path / "batch.json")))
    assert js["bodySteps"] == st["body_steps"] and js["blockSteps"] == st["block_steps"] == 8 and js["finestLevel"] == st["finest_level"], (js, st)
    assert js["clamped"] == st["clamped"] == 0 and js["outerSteps"] == 1
    assert jb["enabled"] is True and all(jb[c_] == bs[k] for k, c_ in CAMEL.items()), (jb, bs)
    assert bs["small_steps"] > 0 and bs["host_steps"] >= 1, bs
    assert np.fromfile(str(tmp_path / "levels.u8"), np.uint8).tobytes() == lev.tobytes() == lev0.tobytes()
    for name, arr in (("bodies", b), ("vel", v), ("accel", a), ("jerk", j)):
        got = np.fromfile(str(tmp_path / (name + ".f64")), "<f8").reshape(-1, 4)
        assert got.tobytes() == arr.tobytes(), name
