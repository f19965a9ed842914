#!/usr/bin/env python3
"""Times the crackle pass of an order-6 start (set_start6(1): nb_h6_crk_pk / nb_h6_crk64 + nb_h6_reduce1) against the
force+jerk+snap pass on the same handle, and prints ONE JSON line.

The crackle pass has no entry point of its own: it runs inside the start.  set_start6() drops a start no step has consumed while
(a, j) stay current, so the next force_pass(1) makes the start again -- the snap pass and, at mode 1, the crackle pass (at mode 0 a
memset in its place) -- and then runs one force+jerk+snap pass.  Per size of --sizes, f32 and f64, in turns, --rounds times, wall time
with the device idle before and after:
  t1 = set_start6(1) + force_pass(1)      snap pass + crackle pass + one pass
  t0 = set_start6(0) + force_pass(1)      snap pass + memset       + one pass
  pass_ms                                 nb_force_pass's own figure for the force+jerk+snap pass (kernel + reduce), --min-seconds of it
  ratio = (t1 - t0) / pass_ms             the crackle pass (less a memset of N rows) over the force+jerk+snap pass

Needs a GPU (no fallback)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
from nbody3d_amd import Simulation, capi, ic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[65536, 262144])
    ap.add_argument("--precisions", nargs="*", default=["f32", "f64"])
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if capi.device_count() < 1:
        sys.exit("start6_pass: no GPU")
    out = {"tool": "start6_pass", "min_seconds": args.min_seconds, "rounds": args.rounds, "sizes": {}}
    for prec in args.precisions:
        for n in args.sizes:
            b, v = ic.plummer(n, seed=1)
            with Simulation(n, precision=prec, integrator="hermite6") as s:
                s.init(b, v)
                s.set_params(1e-3, 1.0)
                est = s.force_pass(2)
                reps = max(2, int(np.ceil(args.min_seconds * 1e3 / est)))

                def start(mode):
                    s.set_start6(mode)
                    s.sync()
                    t = time.perf_counter()
                    s.force_pass(1)
                    s.sync()
                    return 1e3 * (time.perf_counter() - t)

                got = {"t1_ms": [], "t0_ms": [], "pass_ms": []}
                start(1)
                start(0)
                for _ in range(args.rounds):
                    s.force_pass(reps)                  # warm: at least min_seconds of the same work
                    got["pass_ms"].append(s.force_pass(reps))
                    got["t1_ms"].append(start(1))
                    got["t0_ms"].append(start(0))
                r = {k: {"best": min(x), "median": float(np.median(x)), "all": x} for k, x in got.items()}
                r["variant"], r["shape"] = s.variant, s.shape_info()
                r["crackle_ms"] = r["t1_ms"]["median"] - r["t0_ms"]["median"]
                r["ratio"] = r["crackle_ms"] / r["pass_ms"]["median"]
                r["ratio_best"] = (r["t1_ms"]["best"] - r["t0_ms"]["best"]) / r["pass_ms"]["best"]
                out["sizes"]["%s_%d" % (prec, n)] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
