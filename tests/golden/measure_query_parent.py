#!/usr/bin/env python3
"""Records tests/golden/query_parent.json: what the six queries, their *_shape getters and the nb_multi_* wrappers answered at the
commit BEFORE they were given one prologue, one staging path and one batch rule (tests/query_parent.py says what is recorded;
tests/test_query_parent_gpu.py holds every later build to it).  Needs the GPU, a few seconds.

Run it on a checkout of that commit (f7b0afc, "Add nb_set_neighbor_scheme") with this script and tests/query_parent.py copied in --
or here, with NB_ENGINE_LIB naming the libnbody3d_hip.so built from that commit: the bindings build the same requests.

    python tests/golden/measure_query_parent.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "nbody3d-webgpu_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402,F401  (first: one HIP runtime for the process, as tests/conftest.py says)
import query_parent as P  # noqa: E402
from nbody3d_amd import capi  # noqa: E402


def main():
    out = {"library": os.path.basename(capi.library_path()), "compute_units": P.compute_units(),
           "shapes": P.all_shapes(), "messages": P.all_messages(), "bits": P.all_bits()}
    path = sys.argv[1] if len(sys.argv) > 1 else P.JSON_PATH
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d compute units, %d handles x %d shapes, %d messages, %d digests" % (
        path, out["compute_units"], len(out["shapes"]), len(next(iter(out["shapes"].values()))), len(out["messages"]),
        sum(len(v) for v in out["bits"].values())))
    for k, (rc, text) in sorted(out["messages"].items()):
        print("  %-48s %d  %s" % (k, rc, text))


if __name__ == "__main__":
    main()
