#!/usr/bin/env python3
"""Records tests/golden/hermite_parent.json: what nb_step did on Hermite handles of orders 4 and 6, with and without block steps,
at the commit BEFORE the two orders were given one host path (tests/hermite_parent.py says what is recorded;
tests/test_hermite_parent_gpu.py holds every later build to it).  Needs the GPU, well under a minute.

Only the public Python API is used, so the script runs unchanged on a checkout of that commit (0a1aa00, "Block individual time
steps on order-6 Hermite handles (f64)") with this script and tests/hermite_parent.py copied in -- or here, with NB_ENGINE_LIB
naming the libnbody3d_hip.so built from that commit.

    python tests/golden/measure_hermite_parent.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "nbody3d-webgpu_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402,F401  (first: one HIP runtime for the process, as tests/conftest.py says)
import hermite_parent as P  # noqa: E402
from nbody3d_amd import capi  # noqa: E402


def main():
    out = {"library": os.path.basename(capi.library_path()), "compute_units": P.compute_units(),
           "messages": P.all_messages(), "bits": P.all_bits()}
    split, whole = out["bits"][P.case_id(P.SPLIT)], out["bits"][P.case_id(P.SPLIT_OF)]
    assert split == whole, "two calls of simulate(1) and one of simulate(2) disagree:\n%s\n%s" % (split, whole)
    path = sys.argv[1] if len(sys.argv) > 1 else P.JSON_PATH
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d compute units, %d cases, %d segments, %d messages" % (
        path, out["compute_units"], len(out["bits"]), sum(len(v) for v in out["bits"].values()), len(out["messages"])))
    for k, segs in sorted(out["bits"].items()):
        for seg in segs:
            print("  %-44s %-28s %s %s" % (k, seg["variant"], seg["shape"], seg["stats"]))
    for k, (rc, text) in sorted(out["messages"].items()):
        print("  %-36s %d  %s" % (k, rc, text))


if __name__ == "__main__":
    main()
