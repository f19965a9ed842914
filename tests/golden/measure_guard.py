"""Measures tests/golden/guard.json on the CPU (numpy only; several minutes): the restatement of the guarded sums of the mixed pass
(tests/guard_ref.py) against the fp64 direct sum on every hard pass case -- the pair members' rows and the pairs' barycentre rows,
at every radius of guard_ref.R_NEARS and with mixed_ref.fj_mixed's binary32 and fp64 sums beside them -- the Plummer cases, five
shared steps, and the block-step run BLOCK with the guarded sum.  test_guard_cpu.py recomputes a part of it; test_guard_gpu.py
takes its bounds from it.

    python tests/golden/measure_guard.py            # rewrites tests/golden/guard.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "nbody3d-webgpu_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import guard_ref as Gd     # noqa: E402
import mixed_ref as M      # noqa: E402


def main():
    rec = dict(factor=M.FACTOR, r_nears=list(Gd.R_NEARS), pairs=M.PAIRS, halves=M.HALVES, block_config=M.BLOCK,
               **{"pass": [], "plummer": [], "steps": []})
    for kind in M.HARD_KINDS:
        for n in M.SIZES:
            r = Gd.measure_pass(kind, n)
            print(r, flush=True)
            rec["pass"].append(r)
    for n in M.SIZES:
        rec["plummer"].append(Gd.measure_plummer(n))
        print(rec["plummer"][-1], flush=True)
    for n in Gd.STEPS_SIZES:
        rec["steps"].append(Gd.measure_steps(n))
        print(rec["steps"][-1], flush=True)
    rec["block"] = {Gd.key(Gd.R_NEARS[0]): M.measure_block(Gd.with_guard(Gd.R_NEARS[0]))}
    print(rec["block"], flush=True)
    with open(Gd.GUARD_JSON, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
