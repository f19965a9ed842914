"""Measures tests/golden/mixed.json on the CPU (numpy only; about five minutes): the restatement of the mixed-precision force+jerk
pass (tests/mixed_ref.py) against the fp64 direct sum on every pass case, with and without the lo word, and the block-step run BLOCK
with every force sum of the comparison.  test_mixed_cpu.py recomputes a part of it; test_mixed_gpu.py takes its bounds from it.

    python tests/golden/measure_mixed.py            # rewrites tests/golden/mixed.json
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "nbody3d-webgpu_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mixed_ref as M      # noqa: E402


def main():
    rec = dict(factor=M.FACTOR, pairs=M.PAIRS, halves=M.HALVES, shift=list(M.SHIFT), seed=M.SEED, block_config=M.BLOCK, **{"pass": []})
    for kind in M.KINDS:
        for n in M.SIZES:
            r = M.measure_pass(kind, n)
            print(r, flush=True)
            rec["pass"].append(r)
    rows = dict(fp64=M.measure_block())
    print("fp64", rows["fp64"], flush=True)
    for acc in M.ACCS:
        rows["mixed_" + acc] = M.measure_block(M.with_acc(acc))
        print(acc, rows["mixed_" + acc], flush=True)
    rows["hi_only"] = M.measure_block(M.with_acc("fp64", lo=False))
    print("hi_only", rows["hi_only"], flush=True)
    rows["f32_handle"] = M.measure_block(store=np.float32)
    print("f32_handle", rows["f32_handle"], flush=True)
    rec["block"] = rows
    with open(M.MIXED_JSON, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
