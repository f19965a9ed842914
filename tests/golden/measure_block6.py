#!/usr/bin/env python3
"""Measures what binary32 costs block steps on order-6 handles with frozen levels, and what noise at the project's fp64 bound moves
the 300-body dynamic run by (tests/block6_ref.py) -> tests/golden/block6.json.  CPU only, a few minutes.

Recorded: the fixtures; for every frozen-schedule and census case the binary32-storing restatement's distance from the fp64 one
(hermite6_ref.distances, the crackle's scale at the finest step) after the one outer step; for the 300-body system with the tight
pair the restatement's counts, |dE/E|, smallest margin, and the largest position deviation of three runs with noise of 1e-12 on
every (a1, j1, s1).  The f32 handles and the 300-body position bound are held to 8 x these figures; none of them comes from a
device.

    python tests/golden/measure_block6.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "nbody3d-webgpu_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import block6_ref  # noqa: E402

out = block6_ref.measure_all()
with open(block6_ref.JSON_PATH, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
