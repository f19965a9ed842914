#!/usr/bin/env python3
"""Measures what binary32 costs the crackle sum of an order-6 start and the steps that follow it, and records the payoff of the
two-rule start on the hard-pair fixture (tests/start6_ref.py) -> tests/golden/start6.json.  CPU only, a few minutes.

Recorded: the fixtures; for every pass and census case of hermite6_ref the binary32-storing restatement's row error of the crackle
against the fp64 direct sum; for every stepping case its distance from the fp64 restatement after 1, 2 and 5 steps from the
NB_START6_CRACKLE start; for the 1,024-body hard-pair system the first outer step's |dE/E0|, counts, start-level histogram and
smallest start margin under both starts; the smallest start margins of the small exact cases.  The f32 handles are held to 8 x
these figures; none of them comes from a device.

    python tests/golden/measure_start6.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "nbody3d-webgpu_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import start6_ref  # noqa: E402

out = start6_ref.measure_all()
with open(start6_ref.JSON_PATH, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
