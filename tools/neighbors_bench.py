#!/usr/bin/env python3
"""Times nb_neighbors (Simulation.neighbors_device: NB_NBR_DEVICE, so no host copy is in the number) with device events around
warmed calls on the handle's own stream, and prints ONE JSON line.

  per precision (f32, f64) and per M = N in --sizes (default 65,536 and 262,144), the bodies' own positions (AT_BODIES), in ONE
  process on ONE handle, in turns:
      nearest          index + dist2
      nearest_count    index + dist2 + count (one radius for all)
      field_phi        nb_field_eval, potential only -- the yardstick: existing code, the same launch shape, the same tile stream
  `ratio_*` = neighbour time / field_phi time (of the best times; the medians are in the line too)

The bar for the ratios is computed, not guessed: `loops` in the line holds the VALU instructions of the built plain (unmasked) inner
loops of nb_nbr_pk<false>, nb_nbr_pk<true> and nb_field_pk<false, true> from csrc/nb_engine.gfx950.s (`make asm`), their issue
cycles by DESIGN.md section 7.1's convention (packed and plain VALU 4 cycles, a transcendental 8) and bar = cycle ratio x 1.20.
`--loops-only` prints just that and needs no GPU.

Every figure: at least --min-seconds of the same work before the timed run and in it; --rounds timed runs per figure, interleaved
across the three arms; the JSON holds the best, the median and the spread (max - min) / min.  Needs a GPU (no fallback)."""
import argparse
import json
import os
import re
import sys

import numpy as np

try:
    import torch          # first: one HIP runtime for torch and the engine (tests/conftest.py has the story)
except Exception as e:    # pragma: no cover
    sys.exit("neighbors_bench: torch is required for the device buffers and events: %s" % e)

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
from nbody3d_amd import Simulation, capi, ic  # noqa: E402


def plain_loop(text, kernel):
    """VALU instruction mix of the innermost loop without a v_cmp_*_u32 / v_cmp_eq (the unmasked one) of `kernel`, the longest such."""
    m = re.search(r"^(_ZN2nb\d+%s\w*):.*?$(.*?)^\.Lfunc_end" % re.escape(kernel), text, re.S | re.M)
    lines = [l.split(";")[0].strip() for l in m.group(2).splitlines()]
    lines = [l for l in lines if l and (not l.startswith(".") or l.startswith(".LBB"))]
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    loops = []
    for i, l in enumerate(lines):
        b = re.match(r"s_cbranch_\w+\s+(\S+)", l)
        if b and b.group(1) in labels and labels[b.group(1)] < i:
            loops.append(lines[labels[b.group(1)]:i + 1])
    inner = [lp for lp in loops if not any(o is not lp and len(o) < len(lp) and o[0] in lp for o in loops)]
    plain = [lp for lp in inner if any(o.startswith("v_pk_fma_f32") for o in lp) and not any(re.match(r"v_cmp_(ne|eq)_u32", o) for o in lp)]
    lp = max(plain, key=len)
    valu = [re.sub(r"_e(32|64)$", "", l.split()[0]) for l in lp if l.startswith("v_")]
    mix = {}
    for o in valu:
        mix[o] = mix.get(o, 0) + 1
    trans = sum(v for k, v in mix.items() if k.startswith(("v_rsq", "v_sqrt", "v_rcp", "v_exp", "v_log")))
    return {"mix": mix, "valu": len(valu), "transcendental": trans, "cycles": 4 * (len(valu) - trans) + 8 * trans}


def loop_counts():
    path = os.path.join(ROOT, "nbody3d-webgpu_amd", "csrc", "nb_engine.gfx950.s")
    if not os.path.exists(path):
        return None
    text = open(path).read()
    out = {"nearest": plain_loop(text, "nb_nbr_pkILb0E"), "nearest_count": plain_loop(text, "nb_nbr_pkILb1E"),
           "field_phi": plain_loop(text, "nb_field_pkILb0ELb1E")}
    for k in ("nearest", "nearest_count"):
        out["cycle_ratio_" + k] = out[k]["cycles"] / out["field_phi"]["cycles"]
        out["bar_" + k] = 1.20 * out["cycle_ratio_" + k]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops-only", action="store_true", help="print the loop counts and the bar from csrc/nb_engine.gfx950.s; no GPU")
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 262144])
    ap.add_argument("--precisions", nargs="+", default=["f32", "f64"])
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.loops_only:
        print(json.dumps({"tool": "neighbors_bench", "loops": loop_counts()}))
        return
    if capi.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("neighbors_bench: no GPU")
    stream = torch.cuda.Stream()
    out = {"tool": "neighbors_bench", "device": torch.cuda.get_device_name(0), "min_seconds": args.min_seconds, "rounds": args.rounds, "loops": loop_counts(), "cases": []}

    def timed(fn):
        """ms per call of fn (enqueues on `stream`): estimate, warm for min_seconds, then one timed run of min_seconds."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn(); stream.synchronize()
        e0.record(stream); fn(); e1.record(stream); stream.synchronize()
        reps = max(2, int(np.ceil(args.min_seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
        for _ in range(reps):
            fn()
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream); stream.synchronize()
        return e0.elapsed_time(e1) / reps

    for precision in args.precisions:
        dt, tt = (np.float64, torch.float64) if precision == "f64" else (np.float32, torch.float32)
        for n in args.sizes:
            b, v = ic.plummer(n, seed=7)
            with Simulation(n, precision=precision, stream=stream.cuda_stream) as s:
                s.init(b.astype(dt), v.astype(dt))
                s.set_params(1e-3, 1.0)
                with torch.cuda.stream(stream):
                    idx = torch.zeros(n, device="cuda", dtype=torch.int32)
                    cnt = torch.zeros(n, device="cuda", dtype=torch.int32)
                    d2 = torch.zeros(n, device="cuda", dtype=tt)
                    phi = torch.zeros(n, device="cuda", dtype=tt)
                arms = {
                    "nearest": lambda: s.neighbors_device(None, 0, idx.data_ptr(), d2.data_ptr(), None, bodies=(0, n)),
                    "nearest_count": lambda: s.neighbors_device(None, 0, idx.data_ptr(), d2.data_ptr(), cnt.data_ptr(), bodies=(0, n), radius=0.05),
                    "field_phi": lambda: s.field_device(None, 0, None, phi.data_ptr(), bodies=(0, n)),
                }
                ms = {k: [] for k in arms}
                for _ in range(args.rounds):
                    for k, fn in arms.items():
                        ms[k].append(timed(fn))
                case = {"precision": precision, "n": n, "shape": s.neighbors_shape(n)}
                for k, xs in ms.items():
                    case[k + "_ms"] = {"best": min(xs), "median": float(np.median(xs)), "spread": (max(xs) - min(xs)) / min(xs)}
                for k in ("nearest", "nearest_count"):
                    case["ratio_" + k] = min(ms[k]) / min(ms["field_phi"])
                    case["ratio_" + k + "_median"] = float(np.median(ms[k]) / np.median(ms["field_phi"]))
                    case["gpairs_per_s_" + k] = (n * (n - 1.0)) / (min(ms[k]) * 1e-3) / 1e9
                out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
