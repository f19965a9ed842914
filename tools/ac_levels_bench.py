#!/usr/bin/env python3
"""Measures the block individual irregular steps of the neighbour scheme (Simulation.set_neighbor_levels) on one GPU and prints
ONE JSON line.

  (1) tick     per precision and N in --sizes: ic.plummer(N, seed=7) on a Hermite handle, the radius chosen (bisection on
               nb_neighbors' count) for a mean count of ~32, cap 256 or what the largest count needs.  In ONE process on ONE
               handle, in turns, --rounds times, one regular step (wall time with its host wait) at N_sub = --sub-lo and --sub-hi of
                   shared   the shared substeps (nb_ac_sub*, the code of a handle without levels)
                   all      dynamic levels with min_level = L: every body due at every tick, every decision evaluated
                   due64    uploaded frozen levels, 64 bodies at L and the rest at 0: 64 bodies due at every tick but the last
                   empty    levels frozen at 0: no body due at any tick but the last
               and per arm (step_hi - step_lo) / (sub_hi - sub_lo): what ONE tick of that kind (two launches) or ONE shared substep
               launch adds to a regular step, launch gaps included.  `all_ratio` = all / shared, bar 1.5 (f32).
  (2) step     one regular step at L = 6 with uploaded frozen levels, 1 % of the bodies at level 6 and the rest at 3 (8 full and 56
               sparse ticks), against the shared scheme at N_sub = 64 and at N_sub = 8.  Bar: below the N_sub = 64 arm.
  (3) accuracy block_bench's workload (ic.plummer with 1 % of the bodies as tight pairs at +-0.02), N = --acc-n, one time unit at
               dt = 2^-6, radius 0.1, cap 128: |dE/E0| and wall time with dynamic levels (L = 6, min_level 2 and 3) beside the shared
               scheme at N_sub = 8 and 64.  Recorded only.

Every figure of (1) and (2): at least --min-seconds of the same work before the timed run and in it.  Every GPU step runs under its
own time limit (--step-limit seconds): when one runs out the process ends with status 124 and starts nothing more.  Needs a GPU."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


class step_limit:
    """A time limit for one GPU step: a step that outlives it ends the process (status 124); nothing more is started."""

    def __init__(self, seconds, what):
        self.t = threading.Timer(seconds, self._expire, (what, seconds))
        self.t.daemon = True

    @staticmethod
    def _expire(what, seconds):
        sys.stderr.write("ac_levels_bench: step '%s' exceeded its limit of %g s; ending\n" % (what, seconds))
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        self.t.start()

    def __exit__(self, *a):
        self.t.cancel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 262144])
    ap.add_argument("--precisions", nargs="+", default=["f32", "f64"])
    ap.add_argument("--sub-lo", type=int, default=8)
    ap.add_argument("--sub-hi", type=int, default=32)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-limit", type=float, default=60.0)
    ap.add_argument("--acc-n", type=int, default=16384)
    ap.add_argument("--only", choices=["timing", "accuracy"], default=None)
    args = ap.parse_args()
    try:
        import torch          # first: one HIP runtime for torch and the engine (tests/conftest.py has the story)
    except Exception as e:    # pragma: no cover
        sys.exit("ac_levels_bench: torch is required for the device buffers: %s" % e)
    sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
    from nbody3d_amd import Simulation, capi, ic
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from block_bench import energy, with_tight_pairs      # tools/block_bench.py: the workload of profiles/r08/block_steps.md
    if capi.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("ac_levels_bench: no GPU")
    stream = torch.cuda.Stream()
    out = {"tool": "ac_levels_bench", "device": torch.cuda.get_device_name(0), "min_seconds": args.min_seconds, "rounds": args.rounds,
           "sub_lo": args.sub_lo, "sub_hi": args.sub_hi, "cases": [], "accuracy": None}

    def walled(s):
        """ms per step of s.simulate (wall clock: a regular step ends with a host wait), warmed and timed for min_seconds each."""
        s.simulate(1); s.sync()
        t = time.perf_counter(); s.simulate(1); s.sync()
        reps = max(2, int(np.ceil(args.min_seconds / max(time.perf_counter() - t, 1e-6))))
        s.simulate(reps); s.sync()
        t = time.perf_counter(); s.simulate(reps); s.sync()
        return 1e3 * (time.perf_counter() - t) / reps

    for precision in ([] if args.only == "accuracy" else args.precisions):
        dt = np.float64 if precision == "f64" else np.float32
        for n in args.sizes:
            b, v = ic.plummer(n, seed=7)
            with Simulation(n, precision=precision, stream=stream.cuda_stream, integrator="hermite4") as s:
                s.init(b.astype(dt), v.astype(dt))
                s.set_params(2.0 ** -10, 1.0)        # short steps: the lists stay what they are over the measurement
                with torch.cuda.stream(stream):
                    cnt = torch.zeros(n, device="cuda", dtype=torch.int32)

                def mean_count(h):
                    s.neighbors_device(None, 0, None, None, cnt.data_ptr(), bodies=(0, n), radius=h)
                    stream.synchronize()
                    return float(cnt.double().mean().item()), int(cnt.max().item())

                with step_limit(args.step_limit, "radius"):
                    lo, hi = 0.0, 4.0
                    for _ in range(24):          # bisection: the mean count grows with the radius
                        mid = 0.5 * (lo + hi)
                        lo, hi = (mid, hi) if mean_count(mid)[0] < 32.0 else (lo, mid)
                    h = 0.5 * (lo + hi)
                    mc, mx = mean_count(h)
                cap = max(256, (mx + 32 + 63) // 64 * 64)
                case = {"precision": precision, "n": n, "radius": h, "mean_count": mc, "max_count": mx, "cap": cap}

                def shared(k):
                    s.set_neighbor_scheme(radius=h, substeps=k, cap=cap)
                    return walled(s)

                def floor(k, m, frozen):
                    s.set_neighbor_scheme(radius=h, substeps=k, cap=cap)
                    s.set_neighbor_levels(min_level=m, frozen=frozen)
                    return walled(s)

                def uploaded(k, lev, m=0):
                    s.set_neighbor_scheme(radius=h, substeps=k, cap=cap)
                    s.set_neighbor_levels(min_level=m, frozen=True)
                    s.simulate(1)                # the scheme is current behind a step
                    s.upload_neighbor_levels(lev)
                    return walled(s)

                def due64(k):
                    L = k.bit_length() - 1
                    lev = np.zeros(n, np.uint8)
                    lev[np.linspace(0, n - 1, 64).astype(np.int64)] = L
                    return uploaded(k, lev)

                one_percent = np.full(n, 3, np.uint8)
                one_percent[::100] = 6
                lo_, hi_ = args.sub_lo, args.sub_hi
                arms = {
                    "shared_lo": lambda: shared(lo_), "shared_hi": lambda: shared(hi_),
                    "all_lo": lambda: floor(lo_, lo_.bit_length() - 1, False), "all_hi": lambda: floor(hi_, hi_.bit_length() - 1, False),
                    "due64_lo": lambda: due64(lo_), "due64_hi": lambda: due64(hi_),
                    "empty_lo": lambda: floor(lo_, 0, True), "empty_hi": lambda: floor(hi_, 0, True),
                    "levels_1pc": lambda: uploaded(64, one_percent, 3), "shared_64": lambda: shared(64), "shared_8": lambda: shared(8),
                }
                ms = {k: [] for k in arms}
                for _ in range(args.rounds):
                    for k, fn in arms.items():
                        with step_limit(args.step_limit, "%s %s n=%d" % (k, precision, n)):
                            ms[k].append(fn())
                for k, xs in ms.items():
                    case[k + "_ms"] = {"best": min(xs), "median": float(np.median(xs)), "spread": (max(xs) - min(xs)) / min(xs)}
                med = lambda k: float(np.median(ms[k]))
                per = lambda arm: (med(arm + "_hi") - med(arm + "_lo")) / (hi_ - lo_)
                case["substep_ms"] = per("shared")
                case["tick_all_ms"], case["tick_due64_ms"], case["tick_empty_ms"] = per("all"), per("due64"), per("empty")
                case["all_ratio"] = case["tick_all_ms"] / case["substep_ms"]
                case["due64_ratio"] = case["tick_due64_ms"] / case["substep_ms"]
                case["empty_ratio"] = case["tick_empty_ms"] / case["substep_ms"]
                case["step_ratio_64"] = med("levels_1pc") / med("shared_64")
                case["step_ratio_8"] = med("levels_1pc") / med("shared_8")
                if precision == "f32":
                    case["tick_inside_bar"] = bool(case["all_ratio"] <= 1.5)
                case["step_inside_bar"] = bool(case["step_ratio_64"] < 1.0)
                out["cases"].append(case)

    if args.only != "timing":
        n = args.acc_n
        b, v = with_tight_pairs(n)
        acc = {"n": n, "pairs": int(0.01 * n) // 2, "precision": "f32", "time": 1.0, "dt": 2.0 ** -6, "runs": []}

        def run(name, substeps, levels):
            with Simulation(n, precision="f32", integrator="hermite4") as s:
                s.init(b, v)
                s.set_params(2.0 ** -6, 1.0)
                s.set_neighbor_scheme(radius=0.1, substeps=substeps, cap=128)
                if levels is not None:
                    s.set_neighbor_levels(**levels)
                e0 = energy(s)
                s.sync()
                t = time.perf_counter()
                try:
                    s.simulate(64)
                except capi.NBodyError as e:
                    return {"arm": name, "error": str(e), "stats": s.neighbor_scheme_stats()}
                s.sync()
                row = {"arm": name, "substeps": substeps, "levels": levels, "wall_s": time.perf_counter() - t, "dE": abs((energy(s) - e0) / e0),
                       "stats": s.neighbor_scheme_stats()}
                if levels is not None:
                    row["level_stats"] = s.neighbor_level_stats()
                    row["final_levels"] = np.bincount(s.download_neighbor_levels(), minlength=7).tolist()
                return row
        for name, substeps, levels in (("shared_8", 8, None), ("shared_64", 64, None), ("levels_min2", 64, dict(min_level=2)),
                                       ("levels_min3", 64, dict(min_level=3)), ("levels_min0", 64, dict(min_level=0))):
            with step_limit(4 * args.step_limit, "accuracy: " + name):
                acc["runs"].append(run(name, substeps, levels))
        out["accuracy"] = acc
    print(json.dumps(out))


if __name__ == "__main__":
    main()
