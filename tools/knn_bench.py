#!/usr/bin/env python3
"""Times nb_knn (Simulation.knn_device: NB_NBR_DEVICE, so no host copy is in the number) with device events around warmed calls on
the handle's own stream, and prints ONE JSON line.

  per precision (f32, f64) and per M = N in --sizes (default 65,536 and 262,144), a Plummer sphere ic.plummer(N, seed=7), the
  bodies' own positions (AT_BODIES), in ONE process on ONE handle, in turns:
      knn_k6, knn_k32, knn_k64     index + dist2 for k = 6, 32, 64
      nearest                      nb_neighbors index + dist2 (no count) -- the yardstick: existing code this call does not touch
  `ratio_k*` = knn / nearest (of the best times; the medians are in the line too).

`loops` (also alone with `--loops-only`, which needs no GPU) holds the VALU instructions of the built plain (unmasked) inner loops
from csrc/nb_engine.gfx950.s (`make asm`): nb_knn_pk's fast path, nb_nbl_pk's fast path (the condition: the first carries no more
VALU per 16 pairs than the second) and the yardstick's loop nb_nbr_pk<false>, each also per 16 pairs since the loops are unrolled
over different numbers of rows.

`--stats` runs each arm ONCE on the calibration build (libnbody3d_hip_tuning.so, `make tuning`) with its counters on and prints,
per arm: the share of (wave, 4-row group) pairs that left the fast path, the candidates appended per (point, chunk) against the
estimate k (1 + ln(rows per chunk / k)), and the compactions per (point, chunk) before the closing one.  No timing in that mode.

Every timed figure: at least --min-seconds of the same work before the timed run and in it; --rounds timed runs per figure,
interleaved across the arms; the JSON holds the best, the median and the spread (max - min) / min.  Needs a GPU (no fallback)."""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
STATS = "--stats" in sys.argv
if STATS:       # before the bindings pick their library
    os.environ["NB_ENGINE_LIB"] = os.path.join(ROOT, "nbody3d-webgpu_amd", "csrc", "libnbody3d_hip_tuning.so")
    os.environ["NB_KNN_STATS"] = "1"

import numpy as np  # noqa: E402

try:
    import torch          # first: one HIP runtime for torch and the engine (tests/conftest.py has the story)
except Exception as e:    # pragma: no cover
    torch = None
    _torch_error = e

sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nbody3d_amd import Simulation, capi, ic  # noqa: E402
from neighbor_lists_bench import _tally, plain_loop  # noqa: E402

KS = (6, 32, 64)


def loop_counts():
    path = os.path.join(ROOT, "nbody3d-webgpu_amd", "csrc", "nb_engine.gfx950.s")
    if not os.path.exists(path):
        return None
    text = open(path).read()
    out = {}
    for name, kernel in (("knn_fast_path", "nb_knn_pk"), ("lists_fast_path", "nb_nbl_pk"), ("nearest", "nb_nbr_pkILb0E")):
        t = _tally(plain_loop(text, kernel))
        t["valu_per_16_pairs"] = 16.0 * t["valu"] / max(1, t["pairs"])
        out[name] = t
    out["knn_no_more_valu_than_lists"] = out["knn_fast_path"]["valu_per_16_pairs"] <= out["lists_fast_path"]["valu_per_16_pairs"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops-only", action="store_true", help="print the loop counts from csrc/nb_engine.gfx950.s; no GPU")
    ap.add_argument("--stats", action="store_true", help="the calibration build's counters instead of timings")
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 262144])
    ap.add_argument("--precisions", nargs="+", default=["f32", "f64"])
    ap.add_argument("--ks", type=int, nargs="+", default=list(KS))
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.loops_only:
        print(json.dumps({"tool": "knn_bench", "loops": loop_counts()}))
        return
    if torch is None:
        sys.exit("knn_bench: torch is required for the device buffers and events: %s" % _torch_error)
    if capi.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("knn_bench: no GPU")
    stream = torch.cuda.Stream()
    out = {"tool": "knn_bench", "mode": "stats" if args.stats else "timing", "device": torch.cuda.get_device_name(0)}
    if not args.stats:
        out.update({"min_seconds": args.min_seconds, "rounds": args.rounds})
    out.update({"loops": loop_counts(), "cases": []})
    L = capi.load_library()
    if args.stats and not hasattr(L, "nb_tuning_knn_stats"):
        sys.exit("knn_bench --stats: %s has no counters (make -C nbody3d-webgpu_amd/csrc tuning)" % capi.library_path())
    if args.stats:
        L.nb_tuning_knn_stats.argtypes = [C.c_void_p, C.c_int]
        L.nb_tuning_knn_stats.restype = None

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
                kmax = max(args.ks)
                with torch.cuda.stream(stream):
                    idx = torch.zeros(n * kmax, device="cuda", dtype=torch.int32)
                    d2 = torch.zeros(n * kmax, device="cuda", dtype=tt)
                case = {"precision": precision, "n": n, "nearest_shape": s.neighbors_shape(n)}
                arms = {"nearest": (lambda: s.neighbors_device(None, 0, idx.data_ptr(), d2.data_ptr(), None, bodies=(0, n)))}
                for k in args.ks:
                    case["shape_k%d" % k] = s.knn_shape(n, k)
                    arms["knn_k%d" % k] = (lambda k=k: s.knn_device(None, 0, k, idx.data_ptr(), d2.data_ptr(), bodies=(0, n)))
                if args.stats:
                    for k in args.ks:
                        L.nb_tuning_knn_stats(None, 1)
                        arms["knn_k%d" % k]()
                        stream.synchronize()
                        c = (C.c_uint64 * 5)()
                        L.nb_tuning_knn_stats(c, 1)
                        rows, cand, comp, slow, groups = (int(x) for x in c)
                        per = case["shape_k%d" % k]["j_per_chunk"]
                        assert rows == case["shape_k%d" % k]["chunks"] * n, (rows, case["shape_k%d" % k])      # every batch ran the request's chunks
                        case["stats_k%d" % k] = {"point_chunk_rows": rows, "candidates_per_row": cand / rows, "compactions_per_row": comp / rows,
                                                 "estimate_k_1_plus_ln": k * (1.0 + math.log(max(1.0, min(per, n) / k))),
                                                 "slow_group_share": slow / groups, "candidate_share_of_pairs": cand / (float(n) * n)}
                else:
                    ms = {name: [] for name in arms}
                    for _ in range(args.rounds):
                        for name, fn in arms.items():
                            ms[name].append(timed(fn))
                    for name, xs in ms.items():
                        case[name + "_ms"] = {"best": min(xs), "median": float(np.median(xs)), "spread": (max(xs) - min(xs)) / min(xs)}
                    for k in args.ks:
                        case["ratio_k%d" % k] = min(ms["knn_k%d" % k]) / min(ms["nearest"])
                        case["ratio_k%d_median" % k] = float(np.median(ms["knn_k%d" % k]) / np.median(ms["nearest"]))
                out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
