#!/usr/bin/env python3
"""Measures what binary32 costs the 6th-order Hermite scheme (tests/hermite6_ref.py) -> tests/golden/hermite6.json.  CPU only, about
two minutes.

Recorded: the fixtures (sizes, step, G, the census rows, the Kepler pair); for every pass case the worst row error |got - ref|_2 /
sum |term|_2 of the binary32 restatement's (a, j, s) against the fp64 one; for every stepping case the binary32-storing
restatement's distance from the fp64 one after 1, 2 and 5 steps; the restatement's Kepler errors and their ratios per halving of
dt.  The f32 handles are held to 8 x these figures; none of them comes from a device.

    python tests/golden/measure_hermite6.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "nbody3d-webgpu_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import hermite6_ref  # noqa: E402

out = hermite6_ref.measure_all()
with open(hermite6_ref.JSON_PATH, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
