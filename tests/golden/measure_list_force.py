#!/usr/bin/env python3
"""Measures the tolerances of the nb_list_force census (tests/list_force_ref.py) -> tests/golden/list_force_census.json.  CPU only, a
few seconds.

Inputs: census_ref.bodies(n, 5) / velocities(n, 5) for n = 77, 1025, 4099, G = 0.37, eps2 = 1e-4; rows = the bodies inside 1.6 and 2.4
lattice spacings of every body and of 300 arbitrary points (numpy).  Every input goes through a binary32 restatement of the sums (the
pair arithmetic of census_ref._f32_terms, one ordered ascending sum per row); recorded per input and per output (a, jerk, phi; at
the bodies and, pt_*, at the points): the worst row error of that arithmetic against numpy fp64, min_share (the smallest share one
entry has of its row) and tol = 8 x that error.  The kernels are held to `tol`; it is never derived from a device's output.

    python tests/golden/measure_list_force.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "nbody3d-webgpu_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import list_force_ref  # noqa: E402

out = list_force_ref.measure_all()
with open(list_force_ref.JSON_PATH, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
for e in out["inputs"]:
    for pre in ("", "pt_"):
        print("n=%-5d %.1f spacings %-6s mean count %5.1f  " % (e["n"], e["spacings"], pre or "bodies", e["points_mean_count" if pre else "mean_count"])
              + "  ".join("%s: fp32 %.3g share %.3g (%.0f x tol)" % (k, e[pre + k + "_ref_f32_err"], e[pre + k + "_min_share"],
                                                                   e[pre + k + "_min_share"] / e[pre + k + "_tol"] if e[pre + k + "_tol"] else float("inf"))
                          for k in ("a", "jerk", "phi")))
