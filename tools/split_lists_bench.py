#!/usr/bin/env python3
"""Times nb_split_lists (Simulation.split_lists_device: NB_SPLIT_DEVICE, so no host copy is in the number) against the calls it stands
for on the SAME Hermite handle, and prints ONE JSON line.

  The bar of (a) comes from the built loops (`make asm` -> csrc/nb_engine.gfx950.s): the VALU and transcendental instructions on the
  FAST path of one trip of the inner loop of nb_spl_pk<.., true> (the blocks a forward branch skips when no lane has a member are left
  out) and of the plain inner loop of nb_split_pk<.., true>, their issue cycles by DESIGN.md section 7.1's convention (every VALU
  instruction 4 cycles, a transcendental 8) per 16 pairs, and bar = (nb_spl_pk cycles / nb_split_pk cycles) x 1.20.  The scalar
  instructions of either loop are reported beside them.  `--loops-only` prints just that and needs no GPU.

  per precision (f32, f64) and per M = N in --sizes (default 65,536 and 262,144): ic.plummer(N, seed=7) on a Hermite handle, AT_BODIES,
  device pointers, the radius chosen (bisection on nb_neighbors' count) for a mean count of ~32, cap 128.  In ONE process on ONE
  handle, in turns, --rounds times:
      split_lists   nb_split_lists, all four sums, the rows and the counts             -- the main figure
      split         nb_split_force, the same four sums                                 -- (a)
      two_calls     nb_split_force, then nb_neighbor_lists (rows and counts)           -- (b): the route the call replaces
      lists         nb_neighbor_lists alone
      empty_lists / empty_split   the first two with a radius that leaves every row empty: the slow path's share of (a)
  Reported per arm: ms best / median / spread; `ratio` = split_lists / split of the best times and of the medians, `ratio_worse`,
  `inside_bar` (f32 only: the bar is the f32 loops'); `ratio_empty`; `ratio_route` = split_lists / two_calls (best and median),
  `route_spread` the two_calls arm's own run-to-run spread and `beats_route` = 1 - ratio_route_worse > route_spread.
  (c) with --steps: one regular step of the neighbour scheme (N_sub = 8, the same radius, cap 128 or what the largest count needs)
  on a default handle and on an
  NB_FLAG_AC_TWO_CALLS handle, alternating, ms per step from events round nb_step(k).
  `clock`: what the runtime and a read-only rocm-smi --showclocks report when the tool starts.

Every figure: at least --min-seconds of the same work before the timed run and in it.  Every GPU step runs under its own time limit
(--step-limit seconds): when one runs out the process ends with status 124 and starts nothing more.  Needs a GPU (no fallback)."""
import argparse
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from split_force_bench import ASM, ROOT, TRANS, _loops, device_clock, plain_loop, step_limit  # noqa: E402


def fast_path_loop(text, kernel):
    """Tally of the fast path through the innermost loop of `kernel` that holds the pair arithmetic: the loop's instructions in
    order, every stretch that a forward branch inside the loop jumps over and that holds a store left out."""
    loops = _loops(text, kernel)
    inner = [lp for lp in loops if not any(o is not lp and len(o) < len(lp) and o[0] in lp for o in loops)]
    # (the compiler may rotate the loop: of two candidates with the pair arithmetic, the one that also holds the tile reads is the trip)
    lp = max(inner, key=lambda q: (len([o for o in q if o.startswith("v_rsq")]), len([o for o in q if o.startswith("ds_read")])))
    labels = {l[:-1]: i for i, l in enumerate(lp) if l.endswith(":")}
    path, i, skipped = [], 0, 0
    while i < len(lp):
        l = lp[i]
        b = re.match(r"s_cbranch\w*\s+(\S+)", l)
        if b and labels.get(b.group(1), -1) > i and any(o.startswith("global_store") for o in lp[i + 1:labels[b.group(1)]]):
            path.append(l)
            skipped += labels[b.group(1)] - i - 1
            i = labels[b.group(1)]
            continue
        path.append(l)
        i += 1
    valu = [re.sub(r"_e(32|64)$", "", l.split()[0]) for l in path if l.startswith("v_")]
    mix = {}
    for o in valu:
        mix[o] = mix.get(o, 0) + 1
    trans = sum(mix.get(t, 0) for t in TRANS)
    pairs = mix.get("v_rsq_f32", 0)
    cycles = 4 * len(valu) + 4 * trans
    return {"valu": len(valu), "transcendental": trans, "pairs": pairs, "salu": len([l for l in path if l.startswith("s_")]),
            "branches": len([l for l in path if l.startswith("s_cbranch")]), "lds_reads": len([l for l in path if l.startswith("ds_read")]),
            "slow_path_instructions_left_out": skipped, "cycles": cycles, "cycles_per_16_pairs": 16.0 * cycles / max(1, pairs), "mix": mix}


def loop_counts():
    if not os.path.exists(ASM):
        return None
    text = open(ASM).read()
    ng = int(re.search(r"^_ZN2nb\d+nb_split_pkILi(\d)ELb1E", text, re.M).group(1))
    sp = plain_loop(text, "nb_split_pkILi%dELb1E" % ng)
    sp["salu"] = None
    out = {"split_ng": ng, "split_lists_jerk": fast_path_loop(text, "nb_spl_pkILi%dELb1E" % ng), "split_jerk": sp,
           "split_lists_accel": fast_path_loop(text, "nb_spl_pkILi%dELb0E" % ng), "split_accel": plain_loop(text, "nb_split_pkILi%dELb0E" % ng)}
    out["split_jerk"]["cycles_per_16_pairs"] = 16.0 * sp["cycles_per_pair"]
    out["cycle_ratio"] = out["split_lists_jerk"]["cycles_per_16_pairs"] / out["split_jerk"]["cycles_per_16_pairs"]
    out["bar"] = 1.20 * out["cycle_ratio"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops-only", action="store_true", help="print the loop counts and the bar from csrc/nb_engine.gfx950.s; no GPU")
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 262144])
    ap.add_argument("--precisions", nargs="+", default=["f32", "f64"])
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cap", type=int, default=128)
    ap.add_argument("--steps", type=int, default=0, help="(c): regular steps of the neighbour scheme per timed run (0: skip)")
    ap.add_argument("--step-limit", type=float, default=120.0)
    args = ap.parse_args()
    if args.loops_only:
        print(json.dumps({"tool": "split_lists_bench", "loops": loop_counts()}))
        return
    try:
        import torch          # first: one HIP runtime for torch and the engine (tests/conftest.py has the story)
    except Exception as e:    # pragma: no cover
        sys.exit("split_lists_bench: torch is required for the device buffers and events: %s" % e)
    sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
    from nbody3d_amd import Simulation, capi, ic
    if capi.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("split_lists_bench: no GPU")
    stream = torch.cuda.Stream()
    loops = loop_counts()
    cap = args.cap
    out = {"tool": "split_lists_bench", "device": torch.cuda.get_device_name(0), "clock": device_clock(torch), "min_seconds": args.min_seconds,
           "rounds": args.rounds, "cap": cap, "loops": loops, "cases": []}

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

    def stat(xs):
        return {"best": min(xs), "median": float(np.median(xs)), "spread": (max(xs) - min(xs)) / min(xs)}

    for precision in args.precisions:
        dt, tt = (np.float64, torch.float64) if precision == "f64" else (np.float32, torch.float32)
        for n in args.sizes:
            b, v = ic.plummer(n, seed=7)
            with Simulation(n, precision=precision, stream=stream.cuda_stream, integrator="hermite4") as s:
                s.init(b.astype(dt), v.astype(dt))
                s.set_params(1e-3, 1.0)
                with torch.cuda.stream(stream):
                    cnt = torch.zeros(n, device="cuda", dtype=torch.int32)
                    o = [torch.zeros((n, 4), device="cuda", dtype=tt) for _ in range(4)]
                    lst = torch.zeros((n, cap), device="cuda", dtype=torch.int32)

                def mean_count(h):
                    s.neighbors_device(None, 0, None, None, cnt.data_ptr(), bodies=(0, n), radius=h)
                    stream.synchronize()
                    return float(cnt.double().mean().item())

                with step_limit(args.step_limit, "radius"):
                    lo, hi = 0.0, 4.0
                    for _ in range(24):          # bisection: the mean count grows with the radius
                        mid = 0.5 * (lo + hi)
                        lo, hi = (mid, hi) if mean_count(mid) < 32.0 else (lo, mid)
                    h = 0.5 * (lo + hi)
                    mc = mean_count(h)
                    over, mx = int((cnt > cap).sum().item()), int(cnt.max().item())
                sums = dict(accel_irr_ptr=o[0].data_ptr(), accel_reg_ptr=o[1].data_ptr(), jerk_irr_ptr=o[2].data_ptr(), jerk_reg_ptr=o[3].data_ptr())
                tiny = 1e-9
                case = {"precision": precision, "n": n, "radius": h, "mean_count": mc, "max_count": mx, "rows_over_cap": over, "shape": s.split_lists_shape(n, cap),
                        "split_force_shape": s.split_force_shape(n)}

                def two_calls(r=h):
                    s.split_force_device(0, bodies=(0, n), radius=r, **sums)
                    s.neighbor_lists_device(None, 0, lst.data_ptr(), cap, cnt.data_ptr(), bodies=(0, n), radius=r)
                arms = {
                    "split_lists": lambda: s.split_lists_device(0, lst.data_ptr(), cap, cnt.data_ptr(), bodies=(0, n), radius=h, **sums),
                    "split": lambda: s.split_force_device(0, bodies=(0, n), radius=h, **sums),
                    "two_calls": two_calls,
                    "lists": lambda: s.neighbor_lists_device(None, 0, lst.data_ptr(), cap, cnt.data_ptr(), bodies=(0, n), radius=h),
                    "empty_lists": lambda: s.split_lists_device(0, lst.data_ptr(), cap, cnt.data_ptr(), bodies=(0, n), radius=tiny, **sums),
                    "empty_split": lambda: s.split_force_device(0, bodies=(0, n), radius=tiny, **sums),
                }
                ms = {k: [] for k in arms}
                for _ in range(args.rounds):
                    for k, fn in arms.items():
                        with step_limit(args.step_limit, "%s %s n=%d" % (k, precision, n)):
                            ms[k].append(timed(fn))
                for k, xs in ms.items():
                    case[k + "_ms"] = stat(xs)
                med = lambda k: float(np.median(ms[k]))
                case["ratio"] = min(ms["split_lists"]) / min(ms["split"])
                case["ratio_median"] = med("split_lists") / med("split")
                case["ratio_worse"] = max(case["ratio"], case["ratio_median"])
                case["ratio_empty"] = min(ms["empty_lists"]) / min(ms["empty_split"])
                case["ratio_route"] = min(ms["split_lists"]) / min(ms["two_calls"])
                case["ratio_route_median"] = med("split_lists") / med("two_calls")
                case["route_spread"] = case["two_calls_ms"]["spread"]
                case["beats_route"] = bool(1.0 - max(case["ratio_route"], case["ratio_route_median"]) > case["route_spread"])
                if precision == "f32" and loops:
                    case["bar"] = loops["bar"]
                    case["inside_bar"] = bool(case["ratio_worse"] <= loops["bar"])
            if args.steps:
                step = {}
                sims = {}
                for name, flags in (("fused", 0), ("two_calls", capi.NB_FLAG_AC_TWO_CALLS)):
                    sim = Simulation(n, precision=precision, stream=stream.cuda_stream, integrator="hermite4", flags=flags)
                    sim.init(b.astype(dt), v.astype(dt))
                    sim.set_params(1e-4, 1.0)
                    # one radius for a Plummer sphere: the core's rows are several times the mean.  cap, or the largest count and room for
                    # it to move while the handle steps, in whole 64s (tools/ac_scheme_bench.py's rule)
                    step["cap"] = max(cap, (mx + 32 + 63) // 64 * 64)
                    sim.set_neighbor_scheme(radius=h, substeps=8, cap=step["cap"])
                    step[name + "_route"] = int(sim.neighbor_scheme_fused)
                    sims[name] = sim
                ts = {k: [] for k in sims}
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for r in range(args.rounds + 1):
                    for name, sim in sims.items():
                        with step_limit(args.step_limit, "scheme %s %s n=%d" % (name, precision, n)):
                            sim.sync()
                            e0.record(stream)
                            sim.simulate(args.steps)
                            e1.record(stream); stream.synchronize()
                            if r:                      # (the first round holds the start)
                                ts[name].append(e0.elapsed_time(e1) / args.steps)
                for name, sim in sims.items():
                    step[name + "_ms"] = stat(ts[name])
                    step[name + "_stats"] = sim.neighbor_scheme_stats()
                    sim.close()
                step["ratio"] = step["fused_ms"]["best"] / step["two_calls_ms"]["best"]
                case["regular_step"] = step
            out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
