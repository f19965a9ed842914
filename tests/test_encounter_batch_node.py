"""The encounter watch inside batched block steps from JavaScript, on the GPU: one frozen outer step on a small census lattice
(N = 261: two tiles, the last of five rows; l = i mod 4, so |A| = 65, 130, 65, 195, 65, 130, 65 run in small slots) of an f32
'hermite4' simulation through the wrapper's setBlockBatchWatch gives the records and the counters of the int64 brute force
(tests/encounter_ref.py); without the watch the setter is refused."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import encounter_ref as E
import encounter_batch_ref as B

NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_encounter_batch_tests.js")
JS = os.path.join(ROOT, "nbody3d-webgpu_amd", "js")
ADDON = os.path.join(JS, "addon", "nb_napi.node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_batched_encounter_watch_equals_the_brute_force(tmp_path):
    src = os.path.join(JS, "addon", "nb_napi.c")
    if not os.path.exists(ADDON) or os.path.getmtime(ADDON) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", JS, "-s"])
    n = 261
    b0 = E.lattice(1025)[0][:n].astype(np.float32)                 # the first rows of the census lattice: body 0 at the origin, body 1 beside it
    v0 = np.zeros((n, 4), np.float32)
    b0[n - 1, :3] = b0[5, :3]                                      # a coincident pair across the two tiles
    b0[200, :3] = b0[10, :3]                                       # ... and one inside the first
    lev0, rad = E.lattice_levels(n), E.lattice_radii(n, "per_body").astype(np.float32)
    want, hits, passes = E.lattice_brute(b0, lev0, rad)
    assert hits > 0 and B.expected_path(lev0, 256) == (7, 1)
    b0.tofile(str(tmp_path / "bodies0.f32"))
    v0.tofile(str(tmp_path / "vel0.f32"))
    lev0.tofile(str(tmp_path / "levels0.u8"))
    rad.tofile(str(tmp_path / "radii.f32"))
    p = subprocess.run([NODE, SCRIPT, str(tmp_path)], capture_output=True, text=True, timeout=300)
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert line, "node produced no result: rc=%d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(line[-1])
    assert res["ok"] and p.returncode == 0, {k: v for k, v in res["results"].items() if not v["pass"]}
    st, bst = json.load(open(str(tmp_path / "stats.json"))), json.load(open(str(tmp_path / "batch.json")))
    assert st["hits"] == hits and st["passes"] == passes == 8 and st["firstTime"] == want["time"].min(), (st, hits)
    assert bst["smallSteps"] == 7 and bst["hostSteps"] == 1, bst
    got = dict(rho2=np.fromfile(str(tmp_path / "rho2.f32"), "<f4"), partner=np.fromfile(str(tmp_path / "partner.u32"), "<u4"),
               time=np.fromfile(str(tmp_path / "time.f64"), "<f8"), count=np.fromfile(str(tmp_path / "count.u32"), "<u4"))
    for k in got:
        assert np.array_equal(got[k].astype(want[k].dtype), want[k]), (k, np.nonzero(got[k] != want[k])[0][:8])
