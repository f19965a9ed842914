#!/usr/bin/env python3
"""Measures the Ahmad-Cohen neighbour scheme (Simulation.set_neighbor_scheme) on one GPU and prints ONE JSON line.

  (a) substep  per precision and N in --sizes: ic.plummer(N, seed=7) on a Hermite handle, the radius chosen (bisection on
               nb_neighbors' count) for a mean count of ~32, cap 128 or what the largest count needs.  In ONE process on ONE handle, in turns, --rounds times:
                   list_force   nb_list_force, accel + jerk, device pointers, the rows nb_neighbor_lists wrote for that radius
                   step_lo / step_hi   one regular step with N_sub = --sub-lo (8) / --sub-hi (32), wall time with the host wait
                   hermite      one plain shared Hermite step of the same handle with the scheme switched off
                   split, lists nb_split_force (four outputs) and nb_neighbor_lists at the bodies, device pointers
               `substep_ms` = (step_hi - step_lo) / (sub_hi - sub_lo): what ONE substep launch adds to a regular step, launch gaps
               included (the scheme has no entry point that runs a substep alone).  `substep_ratio` = substep_ms / list_force, bar 1.5
               (f32).  `step_ratio_<k>` = step_k / (k x hermite), bar 0.5 for k = 8 at N = 65,536.  `parts`: split, lists, the substep
               launches (k x substep_ms) and `rest` (the first prediction, the old-list sums, the regular correction, the header copy
               and the host wait) of step_lo.
  (b) accuracy block_bench's workload (ic.plummer with 1 % of the bodies as tight pairs at +-0.02), N = --acc-n, one time unit: |dE/E0|
               and wall time of the scheme (dt = 2^-6, N_sub = 8, radius 0.1, cap 128) and of the shared step at dt = 2^-k, k = 6 .. 10.
               Recorded only.

Every figure of (a): at least --min-seconds of the same work before the timed run and in it.  Every GPU step runs under its own time
limit (--step-limit seconds): when one runs out the process ends with status 124 and starts nothing more.  Needs a GPU (no fallback)."""
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
        sys.stderr.write("ac_scheme_bench: step '%s' exceeded its limit of %g s; ending\n" % (what, seconds))
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-limit", type=float, default=60.0)
    ap.add_argument("--acc-n", type=int, default=16384)
    ap.add_argument("--only", choices=["a", "b"], default=None)
    args = ap.parse_args()
    try:
        import torch          # first: one HIP runtime for torch and the engine (tests/conftest.py has the story)
    except Exception as e:    # pragma: no cover
        sys.exit("ac_scheme_bench: torch is required for the device buffers and events: %s" % e)
    sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
    from nbody3d_amd import Simulation, capi, ic
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from block_bench import energy, with_tight_pairs      # tools/block_bench.py: the workload of profiles/r08/block_steps.md
    if capi.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("ac_scheme_bench: no GPU")
    stream = torch.cuda.Stream()
    out = {"tool": "ac_scheme_bench", "device": torch.cuda.get_device_name(0), "min_seconds": args.min_seconds, "rounds": args.rounds,
           "sub_lo": args.sub_lo, "sub_hi": args.sub_hi, "cases": [], "accuracy": None}

    def timed(fn):
        """ms per call of fn (enqueues on `stream`), by events: estimate, warm for min_seconds, then one timed run of min_seconds."""
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

    def walled(s):
        """ms per step of s.simulate (wall clock: a regular step ends with a host wait), warmed and timed for min_seconds each."""
        s.simulate(1); s.sync()
        t = time.perf_counter(); s.simulate(1); s.sync()
        reps = max(2, int(np.ceil(args.min_seconds / max(time.perf_counter() - t, 1e-6))))
        s.simulate(reps); s.sync()
        t = time.perf_counter(); s.simulate(reps); s.sync()
        return 1e3 * (time.perf_counter() - t) / reps

    for precision in ([] if args.only == "b" else args.precisions):
        dt, tt = (np.float64, torch.float64) if precision == "f64" else (np.float32, torch.float32)
        for n in args.sizes:
            b, v = ic.plummer(n, seed=7)
            with Simulation(n, precision=precision, stream=stream.cuda_stream, integrator="hermite4") as s:
                s.init(b.astype(dt), v.astype(dt))
                s.set_params(2.0 ** -10, 1.0)        # short steps: the lists stay what they are over the measurement
                with torch.cuda.stream(stream):
                    cnt = torch.zeros(n, device="cuda", dtype=torch.int32)
                    o = [torch.zeros((n, 4), device="cuda", dtype=tt) for _ in range(4)]

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
                # one radius for a Plummer sphere: the core's rows are several times the mean.  cap: 128, or the largest count and
                # room for it to move while the handle steps, in whole 64s; both arms read rows of that cap
                cap = max(128, (mx + 32 + 63) // 64 * 64)
                case = {"precision": precision, "n": n, "radius": h, "mean_count": mc, "max_count": mx, "cap": cap}
                with torch.cuda.stream(stream):
                    lst = torch.zeros((n, cap), device="cuda", dtype=torch.int32)

                def scheme(k):
                    s.set_neighbor_scheme(radius=h, substeps=k, cap=cap)
                    return walled(s)

                def plain():
                    s.set_neighbor_scheme(None)
                    return walled(s)

                def lists():
                    s.neighbor_lists_device(None, 0, lst.data_ptr(), cap, cnt.data_ptr(), bodies=(0, n), radius=h)

                arms = {
                    "list_force": lambda: timed(lambda: s.list_force_device(lst.data_ptr(), 0, cap, bodies=(0, n), count_ptr=cnt.data_ptr(),
                                                                            accel_ptr=o[0].data_ptr(), jerk_ptr=o[2].data_ptr())),
                    "step_lo": lambda: scheme(args.sub_lo),
                    "step_hi": lambda: scheme(args.sub_hi),
                    "hermite": plain,
                    "split": lambda: timed(lambda: s.split_force_device(0, bodies=(0, n), radius=h, accel_irr_ptr=o[0].data_ptr(), accel_reg_ptr=o[1].data_ptr(),
                                                                        jerk_irr_ptr=o[2].data_ptr(), jerk_reg_ptr=o[3].data_ptr())),
                    "lists": lambda: timed(lists),
                }
                ms = {k: [] for k in arms}
                for _ in range(args.rounds):
                    for k, fn in arms.items():
                        with step_limit(args.step_limit, "%s %s n=%d" % (k, precision, n)):
                            if k == "list_force":
                                lists(); stream.synchronize()        # the rows of the state as it stands
                            ms[k].append(fn())
                s.set_neighbor_scheme(radius=h, substeps=args.sub_lo, cap=cap)
                s.simulate(1)
                case["stats"] = s.neighbor_scheme_stats()
                for k, xs in ms.items():
                    case[k + "_ms"] = {"best": min(xs), "median": float(np.median(xs)), "spread": (max(xs) - min(xs)) / min(xs)}
                med = lambda k: float(np.median(ms[k]))
                sub = (med("step_hi") - med("step_lo")) / (args.sub_hi - args.sub_lo)
                case["substep_ms"] = sub
                case["substep_ratio"] = sub / med("list_force")
                for k, key in ((args.sub_lo, "step_lo"), (args.sub_hi, "step_hi")):
                    case["step_ratio_%d" % k] = med(key) / (k * med("hermite"))
                case["parts"] = {"split": med("split"), "lists": med("lists"), "substeps": args.sub_lo * sub,
                                 "rest": med("step_lo") - med("split") - med("lists") - args.sub_lo * sub}
                if precision == "f32":
                    case["substep_inside_bar"] = bool(case["substep_ratio"] <= 1.5)
                    if n == 65536:
                        case["step_inside_bar"] = bool(case["step_ratio_%d" % args.sub_lo] <= 0.5)
                out["cases"].append(case)

    if args.only != "a":
        n = args.acc_n
        b, v = with_tight_pairs(n)
        acc = {"n": n, "pairs": int(0.01 * n) // 2, "precision": "f32", "time": 1.0, "scheme": None, "shared": []}

        def run(k, scheme):
            with Simulation(n, precision="f32", integrator="hermite4") as s:
                s.init(b, v)
                s.set_params(2.0 ** -k, 1.0)
                if scheme:
                    s.set_neighbor_scheme(**scheme)
                e0 = energy(s)
                s.sync()
                t = time.perf_counter()
                try:
                    s.simulate(2 ** k)
                except capi.NBodyError as e:
                    return {"level": k, "error": str(e), "stats": s.neighbor_scheme_stats()}
                s.sync()
                row = {"level": k, "wall_s": time.perf_counter() - t, "dE": abs((energy(s) - e0) / e0)}
                if scheme:
                    row["stats"] = s.neighbor_scheme_stats()
                    row["scheme"] = scheme
                return row
        with step_limit(4 * args.step_limit, "accuracy: scheme"):
            acc["scheme"] = run(6, dict(radius=0.1, substeps=8, cap=128))
        for k in range(6, 11):
            with step_limit(4 * args.step_limit, "accuracy: shared 2^-%d" % k):
                acc["shared"].append(run(k, None))
        out["accuracy"] = acc
    print(json.dumps(out))


if __name__ == "__main__":
    main()
