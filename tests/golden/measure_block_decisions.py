#!/usr/bin/env python3
"""Measures the inputs and tolerances of the block-step decision audit (tests/block_ref.py, tests/test_block_decisions_gpu.py)
-> tests/golden/block_decisions.json and the fixtures block_decisions_n<N>_{levels,state}.npy.  CPU only, about two minutes.

Part A, per input (tight_pair(plummer(n, seed)), one outer step of dt with eta = 0.02; three at N = 1025): the parameters, the
restatement's stats after every outer step, the histogram of the final levels, the sizes of the active sets by bucket, the counts
of the decisions by kind, the smallest decision margin, and the noise experiment: every (a1, j1) of the restatement moved by 1e-12
of the system's max |a| and max |j| (the project's fp64 bound on them), three seeds -- the number of bodies whose final level
changed, the flip-safe margin (the largest reference margin among them; 0: none changed) and the largest position deviation
(norm_err).  For the sizes in block_ref.STORED the final levels and the state of 256 sampled rows are written as fixtures.

Part B, per (n, precision): the evaluation spread of tau -- fp64 as decide() evaluates it against np.longdouble and against fp64
with a2e as one expression -- on one emulated block step per dt, and of the start rule's tau.  `exclusion_margin` is 8 x the
largest of them; `excluded_cap` is the largest share of one run's decisions that may sit inside it.

    python tests/golden/measure_block_decisions.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "nbody3d-webgpu_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import block_ref as R  # noqa: E402

out = {"generator": "tests/golden/measure_block_decisions.py", "metric": "norm_err: max |delta|_inf / max |ref|_inf", "G": 1.0,
       "eps2": R.EPS2, "factor": R.FACTOR, "excluded_cap": R.EXCLUDED_CAP, "schedules": [], "steps": []}
for n in R.SCHEDULES:
    rec, lev, state = R.measure_schedule(n)
    R.schedule_conditions(rec)
    out["schedules"].append(rec)
    if n in R.STORED:
        for path, arr in zip(R.fixture_paths(n), (lev, state)):
            np.save(path, arr)
    print("N=%d: %s\n  levels %s\n  |A| %s\n  kinds %s\n  smallest margin %.3g, flip-safe margin %.3g (%d flipped), noise moves positions by %.3g"
          % (n, rec["stats"][-1], rec["levels"], rec["active_sizes"], rec["kinds"], rec["min_margin"], rec["flip_safe_margin"],
             rec["noise_flipped"], rec["noise_position_dev"]))
for n in R.STEP_SIZES:
    for prec in ("f32", "f64"):
        rec = R.measure_step(n, prec)
        out["steps"].append(rec)
        print("one block step N=%d %s: start tau spread %.3g; %s" % (n, prec, rec["start_tau_spread"], "; ".join(
            "dt 2^%d L %d: tau spread %.3g, smallest margin %.3g, clamped %d" % (s["dt_log2"], s["max_level"], s["tau_spread"], s["min_margin"], s["clamped"]) for s in rec["steps"])))
out["exclusion_margin"] = R.exclusion_margin(out["steps"])
print("exclusion margin %.3g" % out["exclusion_margin"])
with open(R.DECISIONS_JSON, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
