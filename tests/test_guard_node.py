"""The guarded sums of the mixed pass from JavaScript.  Without a GPU: the addon exports setPassGuard / passGuard, the wrapper has
the methods and a radius that is no number throws TypeError before any device call.  On the GPU: the calls, their errors, and the
start of hard_shifted at N = 1,025 with setPassGuard(0.01) held to the barycentre bounds of tests/golden/guard.json."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import guard_ref as Gd
import mixed_ref as M

NODE = shutil.which("node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_guard_tests.js")
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
def test_node_guard_surface_cpu():
    res = run_node("cpu")
    for k in ("addon_exports_setPassGuard", "addon_exports_passGuard", "wrapper_has_setPassGuard", "wrapper_has_passGuard",
              "a_string_throws_TypeError"):
        assert res[k]["pass"]


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_guard_keeps_the_barycentre_rows(tmp_path):
    kind, n = "hard_shifted", 1025
    b0, v0, ra, rj = M.pass_ref(kind, n)
    b0.tofile(str(tmp_path / "bodies0.f64"))
    v0.tofile(str(tmp_path / "vel0.f64"))
    res = run_node("gpu", str(tmp_path))
    for k in ("off_by_default", "native_handle_is_a_state_error", "negative_is_invalid", "nan_is_invalid", "getter_returns_what_was_set",
              "variant_is_hermite4_f64mxg", "native_again_drops_the_guard"):
        assert res[k]["pass"]
    a, j = [np.fromfile(str(tmp_path / (name + ".f64")), "<f8").reshape(-1, 4) for name in ("accel", "jerk")]
    got, rec = Gd.four(a, j, ra, rj, b0), Gd.pass_record(kind, n)[Gd.key(Gd.R_NEARS[0])]
    print("node, guarded pass %s N=%d: %s; restatement %s" % (kind, n, got, rec))
    for q in Gd.QUANTITIES:
        assert got[q] <= M.FACTOR * rec[q], (q, got, rec)
