#!/usr/bin/env python3
"""Measures the tolerances of the pair census (tests/census_ref.py) -> tests/golden/pair_census.json.  CPU only, ~30 s.

Every census input -- the jittered-lattice systems with one residue class of K carrying mass -- goes through the reference's own
binary32 arithmetic: oracle.accel_f32 for the accelerations (at the bodies and at the field points), numpy float32 restatements
with an ordered sum for the jerk (the formula of include/nbody3d_hip.h) and the potential, and nb_diag's stated arithmetic
(binary32 per pair, fp64 sum) for the potential energy.  Recorded per input: n, K, seeds, the worst err_i of that arithmetic against
numpy fp64 on the row metric, min_share (the smallest share a single pair has of its row), and tol = factor x that error.  The
kernels are held to `tol`; it is never derived from a device's output.  A `factor` other than 8 carries the observed device value
and the reason next to it (`device_err`, `why`), and min_share >= 4 tol still holds.

    python tests/golden/measure_pair_census.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "nbody3d-webgpu_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import census_ref  # noqa: E402

out = census_ref.measure_all()
with open(census_ref.JSON_PATH, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
for kind in ("accel", "field_points", "diag"):
    for e in out[kind]:
        share = e["min_share"] if e["min_share"] is not None else float("inf")
        print("%-12s n=%-6d K=%-4d fp32 reference %.3g  tol %.3g  min_share %.3g (%.0f x tol)" % (
            kind, e["n"], e["K"], e["ref_f32_err"], e["tol"], share, share / e["tol"] if e["tol"] else float("inf")))
