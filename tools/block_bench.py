#!/usr/bin/env python3
"""Measures block individual time steps (Simulation.set_block_steps; with --order 6 Simulation.set_block_steps6 on order-6 handles,
every counterpart below then an order-6 handle too) on one GPU and prints ONE JSON line.

  (a) full     one outer step with every body pinned at level 0 (ONE block step with |A| = N: nb_blk_sched, the host's wait,
               nb_blk_predict, nb_blk_fj_pk / nb_blk_fj64 over the full gathered set, nb_blk_correct) against nb_force_pass of a plain
               Hermite handle (nb_fj_pk / nb_fj64 + nb_fj_reduce) and against its whole shared step, in turns, --rounds times; N = --full-n,
               f32 and f64.  The kernels alone: run this part under `rocprofv3 --kernel-trace --stats -- python tools/block_bench.py --only a`.
  (b) end2end  ic.plummer at each N of --sizes with 1 % of the bodies re-placed as tight pairs (the two bodies at +-0.02 about the pair's
               centre, on the circular orbit of their masses): wall time of one time unit with block steps (eta 0.02, outer step
               --outer-dt), |dE/E0| from nb_diagnostics, body_steps, block_steps and the level histogram; then shared-step Hermite at
               dt = 2^-k, k rising from --shared-from until its |dE/E0| is no worse (at most --shared-to: past that the run is recorded as
               not reached), with each run's wall time (--shared-to below --shared-from: no shared runs).  --eta sets the block steps' accuracy
               parameter, --start-deeper K uploads the start rule's levels K deeper before the run, --start6 (order 6) switches the block handle
               to set_start6(1): the exact crackle and the two-rule start levels; dE_first is |dE/E0| after the first outer step.  --pair-half / --eps2 make the pairs hard (e.g. 0.001 and 1e-8: a period of ~0.1
               time units at N = 16,384 instead of ~4.5), the case the step hierarchy is for
  (c) small    microseconds per block step with |A| = 64 at N = --full-n: frozen levels, 64 bodies at level 6 and the rest at level 0
               (64 block steps per outer step, 63 of them with |A| = 64) minus the same outer step with every body at level 0, over 63
  (i) idle     with --batch: what an idle slot costs.  N = --full-n, frozen, 64 bodies at level 6, 2,000 at level 5 (every even tick has
               2,064 active bodies and parks) and the rest at level 0.  The first outer step after set_block_batch() enqueues one slot,
               then a batch of min(depth, 63) slots whose first slot parks: with depth 32 that leaves 30 idle slots, with depth 3 one,
               and every later batch is the same in both.  (first outer step at depth 32 - at depth 3) / 29, the arms in turns.

--batch DEPTH,SMALL_MAX switches set_block_batch(depth, small_max) on (with --order 6: set_block_batch6): (a) and (c) then run a handle with the mode on in
turns with the one without, (b) runs with the mode on and records the five batch counters (run it without --batch for the other arm).

--pass-precision mixed (order 4, f64 only: (a), (c) and (i) run their f64 case alone, (b) needs --precision f64) calls
set_pass_precision("mixed") on every handle with block steps -- the plain Hermite handles of (a) and the shared runs of (b) stay
native -- and --batch then goes through set_block_batch_mixed.

--watch RADIUS (order 4, native pass) switches set_encounter_watch(radius=RADIUS) on: (a) and (c) run a handle with
the watch on in turns with the one without (the keys --batch names batch_* are then watch_*; watch_stats holds the counters and
the hits per body and pass), (b) runs with the watch on and records the counters, how many bodies carry a record against the pair
members, and the distribution of the recorded rho2 - eps2 of the pair members (run it without --watch for the other arm).
--watch R --batch D,S together switch the watch on and then set_block_batch_watch(depth, small_max): the second arm is the watched
batched mode, the keys are --batch's batch_*, and watch_stats is recorded beside them.

Needs a GPU (no fallback)."""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
from nbody3d_amd import Simulation, capi, ic  # noqa: E402


ORDER = 4      # --order: 6 makes every handle an order-6 one (set_hermite_order(6)) and switches block steps on with set_block_steps6


def hermite(n, prec, eps2=None):
    sim = Simulation(n, precision=prec, integrator="hermite4", eps2=eps2)
    if ORDER == 6:
        sim.set_hermite_order(6)
    return sim


MIXED = False      # --pass-precision mixed: the block handles (f64 only) run the double-single pass


def precisions():
    return ("f64",) if MIXED else ("f32", "f64")


def block_steps(sim, **kw):
    if MIXED:
        sim.set_pass_precision("mixed")
    return sim.set_block_steps6(**kw) if ORDER == 6 else sim.set_block_steps(**kw)


BATCH = None      # --batch: (depth, small_max)


WATCH = None      # --watch: the radius


def second_arm():
    """The name of the second arm of (a) and (c), or None."""
    return "batch" if BATCH else "watch" if WATCH is not None else None


def watch_stats(sim):
    st = sim.encounter_stats()
    rec = sim.download_encounters()
    st["bodies_with_record"] = int((rec["partner"] != capi.ENC_NONE).sum())
    st["hits_per_body_and_pass"] = float(st["hits"]) / max(1, st["passes"]) / sim.n      # (a hit is a body step with at least one candidate)
    return st


def second_arm_on(sim, depth=None):
    if WATCH is not None:
        sim.set_encounter_watch(radius=WATCH)
        if not BATCH:
            return sim
    setter = sim.set_block_batch_watch if WATCH is not None else sim.set_block_batch6 if ORDER == 6 else sim.set_block_batch_mixed if MIXED else sim.set_block_batch
    return setter(depth=BATCH[0] if depth is None else depth, small_max=BATCH[1])


def spread(x):
    return {"median": float(np.median(x)), "min": float(min(x)), "max": float(max(x)), "all": [float(y) for y in x]}


def with_tight_pairs(n, seed=1, frac=0.01, half=0.02):
    """ic.plummer with frac * n bodies (consecutive pairs from body 0) re-placed: +-half along x about the pair's centre, velocities
    +-w along y about the pair's mean velocity, w m_other / (m0 + m1) each with w = sqrt((m0 + m1) / (2 half)) (G = 1)."""
    b, v = ic.plummer(n, seed=seed)
    b, v = b.astype(np.float64), v.astype(np.float64)
    for p in range(int(frac * n) // 2):
        i, k = 2 * p, 2 * p + 1
        m0, m1 = b[i, 3], b[k, 3]
        c = (m0 * b[i, :3] + m1 * b[k, :3]) / (m0 + m1)
        u = (m0 * v[i, :3] + m1 * v[k, :3]) / (m0 + m1)
        w = np.sqrt((m0 + m1) / (2 * half))
        b[i, :3], b[k, :3] = c + (half, 0, 0), c - (half, 0, 0)
        v[i, :3], v[k, :3] = u + (0, w * m1 / (m0 + m1), 0), u - (0, w * m0 / (m0 + m1), 0)
    return b.astype(np.float32), v.astype(np.float32)


def wall(sim, steps):
    sim.sync()
    t = time.perf_counter()
    sim.simulate(steps)
    sim.sync()
    return time.perf_counter() - t


def energy(sim):
    ke, pe, _ = sim.diagnostics()
    return ke + pe


def part_a(args, out):
    n = args.full_n
    b, v = ic.plummer(n, seed=1)
    for prec in precisions():
        with contextlib.ExitStack() as stack:
            blk, plain = stack.enter_context(hermite(n, prec)), stack.enter_context(hermite(n, prec))
            bat = stack.enter_context(hermite(n, prec)) if second_arm() else None      # the handle of the second arm: the batched mode or the watch on
            for s in (blk, plain) + ((bat,) if second_arm() else ()):
                s.init(b, v)
                s.set_params(1e-3, 1.0)
            block_steps(blk, max_level=0, frozen=True)
            if second_arm():
                block_steps(bat, max_level=0, frozen=True)
                second_arm_on(bat)
            est = plain.force_pass(2)
            reps = max(4, int(np.ceil(args.min_seconds * 1e3 / est)))
            got = {"force_pass_ms": [], "shared_step_ms": [], "block_step_ms": []}
            if second_arm():
                got[second_arm() + "_block_step_ms"] = []
            for _ in range(args.rounds):
                plain.force_pass(reps)
                got["force_pass_ms"].append(plain.force_pass(reps))
                wall(plain, reps)
                got["shared_step_ms"].append(1e3 * wall(plain, reps) / reps)
                wall(blk, reps)
                got["block_step_ms"].append(1e3 * wall(blk, reps) / reps)
                if second_arm():
                    wall(bat, reps)
                    got[second_arm() + "_block_step_ms"].append(1e3 * wall(bat, reps) / reps)
            r = {k: {"median": float(np.median(x)), "best": min(x), "all": x} for k, x in got.items()}
            r["variant"] = plain.variant
            r["block_over_force_pass"] = r["block_step_ms"]["median"] / r["force_pass_ms"]["median"]
            r["block_over_shared_step"] = r["block_step_ms"]["median"] / r["shared_step_ms"]["median"]
            if second_arm():
                r[second_arm() + "_over_block"] = r[second_arm() + "_block_step_ms"]["median"] / r["block_step_ms"]["median"]
                r[second_arm() + "_over_block_rounds"] = [x / y for x, y in zip(got[second_arm() + "_block_step_ms"], got["block_step_ms"])]
                r[second_arm() + "_stats"] = bat.block_batch_stats() if BATCH else watch_stats(bat)
                if BATCH and WATCH is not None:
                    r["watch_stats"] = watch_stats(bat)
            out["full"]["%s_%d" % (prec, n)] = r


def part_b(args, out):
    for n in args.sizes:
        b, v = with_tight_pairs(n, half=args.pair_half)
        outer = int(round(1.0 / args.outer_dt))
        r = {"n": n, "pairs": int(0.01 * n) // 2, "precision": args.precision, "outer_dt": args.outer_dt, "eta": args.eta, "order": ORDER,
             "start_deeper": args.start_deeper, "start6": int(args.start6), "pair_half": args.pair_half, "eps2": args.eps2,
             "batch": list(BATCH) if BATCH else None, "watch": WATCH, "pass_precision": "mixed" if MIXED else "native"}
        with hermite(n, args.precision, args.eps2) as sim:
            sim.init(b, v)
            if args.start6:      # the engine's own start: exact crackle, two-rule levels
                sim.set_start6(1)
            sim.set_params(args.outer_dt, 1.0)
            block_steps(sim, eta=args.eta, max_level=args.max_level)
            if second_arm():
                second_arm_on(sim)
            e0 = energy(sim)
            lev0 = sim.read_levels()
            if args.start_deeper:      # the start rule's levels made deeper through nb_upload_levels: every body's first step shorter
                lev0 = np.minimum(lev0 + args.start_deeper, args.max_level).astype(np.uint8)
                sim.upload_levels(lev0)
            sim.block_stats(reset=True)
            if BATCH:
                sim.block_batch_stats(reset=True)
            t = wall(sim, 1)
            de_first = abs((energy(sim) - e0) / e0)
            t += wall(sim, outer - 1)
            r["block"] = {"wall_s": t, "dE_first": de_first, "dE": abs((energy(sim) - e0) / e0), "stats": sim.block_stats(),
                          "levels_start": np.bincount(lev0).tolist(), "levels_end": np.bincount(sim.read_levels()).tolist()}
            if BATCH:
                r["block"]["batch_stats"] = sim.block_batch_stats()
            if WATCH is not None:      # who carries a record, and the pair members' closest approaches (the pairs are bodies 0 .. 2 pairs - 1)
                rec, members = sim.download_encounters(), 2 * r["pairs"]
                have = rec["partner"] != capi.ENC_NONE
                peri = np.sqrt(np.maximum(rec["rho2"][:members][have[:members]].astype(np.float64) - (1e-4 if args.eps2 is None else args.eps2), 0.0))
                r["block"]["watch_stats"] = dict(watch_stats(sim), pair_members=members, pair_members_with_record=int(have[:members].sum()),
                                                 partner_is_the_mate=int((rec["partner"][:members][have[:members]] == (np.arange(members) ^ 1)[have[:members]]).sum()),
                                                 pericentre_quantiles=dict(zip(("min", "p10", "p50", "p90", "max"), np.quantile(peri, [0, 0.1, 0.5, 0.9, 1]).tolist())) if len(peri) else None)
        r["block"]["full_force_equivalents"] = r["block"]["stats"]["body_steps"] / n
        r["shared"] = []
        for k in range(args.shared_from, args.shared_to + 1):
            with hermite(n, args.precision, args.eps2) as sim:
                sim.init(b, v)
                sim.set_params(2.0 ** -k, 1.0)
                e0 = energy(sim)
                t = wall(sim, 2 ** k)
                row = {"level": k, "wall_s": t, "dE": abs((energy(sim) - e0) / e0)}
            r["shared"].append(row)
            if row["dE"] <= r["block"]["dE"]:
                r["shared_match"] = row
                r["speedup"] = row["wall_s"] / r["block"]["wall_s"]
                break
        else:
            r["shared_match"] = None      # not reached by 2^-shared_to: the speedup over the LAST run is a lower bound
            if r["shared"]:
                r["speedup_at_least"] = r["shared"][-1]["wall_s"] / r["block"]["wall_s"]
        out["end2end"].append(r)


def part_c(args, out):
    n, L, k = args.full_n, 6, 64
    b, v = ic.plummer(n, seed=1)
    lev = np.zeros(n, np.uint8)
    lev[np.random.default_rng(5).choice(n, k, replace=False)] = L
    sets = (("all_level0", np.zeros(n, np.uint8)), ("64_at_level6", lev))
    second = second_arm()
    arms = ["off"] + (["on"] if second else [])
    for prec in precisions():
        sims = {}
        try:
            for arm in arms:      # one handle per (arm, set of levels): the arms run in turns
                for name, levels in sets:
                    sim = sims[arm, name] = hermite(n, prec)
                    sim.init(b, v)
                    sim.set_params(1e-3, 1.0)
                    block_steps(sim, max_level=L, frozen=True)
                    if arm == "on":
                        second_arm_on(sim)
                    sim.upload_levels(levels)
                    wall(sim, 4)
                    sim.block_stats(reset=True)
                    if arm == "on" and BATCH:
                        sim.block_batch_stats(reset=True)
            runs = {key: [] for key in sims}
            for _ in range(args.rounds):
                for arm in arms:
                    for name, levels in sets:
                        sim = sims[arm, name]
                        sim.upload_levels(levels)      # the same state of the levels' clock before every timed run
                        runs[arm, name].append(wall(sim, args.small_outer) / args.small_outer)
            res = {}
            for arm in arms:
                t = {}
                for name, _ in sets:
                    st = sims[arm, name].block_stats(reset=True)
                    t[name] = {"outer_step_us": 1e6 * float(np.median(runs[arm, name])), "outer_step_us_rounds": [1e6 * x for x in runs[arm, name]],
                               "block_steps_per_outer": st["block_steps"] / st["outer_steps"], "body_steps_per_outer": st["body_steps"] / st["outer_steps"]}
                    if arm == "on":
                        t[name][second + "_stats"] = sims[arm, name].block_batch_stats() if BATCH else watch_stats(sims[arm, name])
                        if BATCH and WATCH is not None:
                            t[name]["watch_stats"] = watch_stats(sims[arm, name])
                per = [1e6 * (x - y) / (2 ** L - 1) for x, y in zip(runs[arm, "64_at_level6"], runs[arm, "all_level0"])]
                t["us_per_small_block_step"] = (t["64_at_level6"]["outer_step_us"] - t["all_level0"]["outer_step_us"]) / (2 ** L - 1)
                t["us_per_small_block_step_rounds"] = per
                res[arm] = t
            r = res["off"]
            if second:
                r[second] = res["on"]
                r[second]["config"] = list(BATCH) if BATCH else WATCH
                r[second + "_over_off"] = res["on"]["us_per_small_block_step"] / res["off"]["us_per_small_block_step"]
                r["full_set_" + second + "_over_off"] = res["on"]["all_level0"]["outer_step_us"] / res["off"]["all_level0"]["outer_step_us"]
            out["small"]["%s_%d" % (prec, n)] = r
        finally:
            for sim in sims.values():
                sim.close()


def part_i(args, out):
    n, L = args.full_n, 6
    b, v = ic.plummer(n, seed=1)
    pick = np.random.default_rng(5).choice(n, 2064, replace=False)
    lev = np.zeros(n, np.uint8)
    lev[pick[:64]] = L
    lev[pick[64:]] = L - 1
    for prec in precisions():
        with hermite(n, prec) as sim:
            sim.init(b, v)
            sim.set_params(1e-3, 1.0)
            block_steps(sim, max_level=L, frozen=True)
            runs, idle = {3: [], 32: []}, {}
            for r in range(args.rounds + 1):      # the first round warms up
                for depth in (3, 32):
                    second_arm_on(sim, depth)      # the policy starts over: one slot, then min(depth, 63)
                    sim.upload_levels(lev)
                    sim.block_batch_stats(reset=True)
                    t = wall(sim, 1)
                    idle[depth] = sim.block_batch_stats()
                    if r:
                        runs[depth].append(1e6 * t)
            d = idle[32]["idle_slots"] - idle[3]["idle_slots"]
            out["idle"]["%s_%d" % (prec, n)] = {"first_outer_step_us": {str(k): spread(x) for k, x in runs.items()}, "stats": {str(k): s for k, s in idle.items()},
                                                "us_per_idle_slot": (float(np.median(runs[32])) - float(np.median(runs[3]))) / d if d else None,
                                                "us_per_idle_slot_rounds": [(x - y) / d for x, y in zip(runs[32], runs[3])] if d else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["a", "b", "c", "i"], nargs="*", default=["a", "b", "c"])
    ap.add_argument("--batch", default=None, metavar="DEPTH,SMALL_MAX", help="set_block_batch(depth, small_max) on the block handles (with --order 6: set_block_batch6)")
    ap.add_argument("--watch", type=float, default=None, metavar="RADIUS", help="set_encounter_watch(radius=RADIUS) on the block handles (order 4, native pass); with --batch: set_block_batch_watch")
    ap.add_argument("--pass-precision", default="native", choices=["native", "mixed"], help="mixed: set_pass_precision('mixed') on the block handles (f64 only); --batch then uses set_block_batch_mixed")
    ap.add_argument("--full-n", type=int, default=65536)
    ap.add_argument("--sizes", type=int, nargs="*", default=[16384, 65536])
    ap.add_argument("--precision", default="f32", choices=["f32", "f64"])
    ap.add_argument("--pair-half", type=float, default=0.02, help="(b): half the separation of a pair (the issue's workload: 0.02)")
    ap.add_argument("--eps2", type=float, default=None, help="(b): softening (default: the engine's 1e-4)")
    ap.add_argument("--order", type=int, default=4, choices=[4, 6], help="the Hermite order of every handle (6: set_hermite_order(6) + set_block_steps6)")
    ap.add_argument("--eta", type=float, default=0.02, help="(b): the accuracy parameter of the block steps")
    ap.add_argument("--start-deeper", type=int, default=0, help="(b): upload the start rule's levels this many levels deeper before the run")
    ap.add_argument("--start6", action="store_true", help="(b): with --order 6, set_start6(1) on the block handle: exact crackle and two-rule start levels")
    ap.add_argument("--outer-dt", type=float, default=2.0 ** -4)
    ap.add_argument("--max-level", type=int, default=16)
    ap.add_argument("--shared-from", type=int, default=6)
    ap.add_argument("--shared-to", type=int, default=12)
    ap.add_argument("--small-outer", type=int, default=20)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    global ORDER, BATCH, MIXED, WATCH
    WATCH = args.watch
    if WATCH is not None and (args.order != 4 or args.pass_precision != "native" or not WATCH >= 0):
        ap.error("--watch takes a radius >= 0 and needs --order 4 and the native pass")
    ORDER = args.order
    MIXED = args.pass_precision == "mixed"
    if MIXED and ORDER != 4:
        ap.error("--pass-precision mixed needs --order 4")
    if MIXED and "b" in args.only and args.precision != "f64":
        ap.error("--pass-precision mixed with (b) needs --precision f64")
    if args.batch:
        BATCH = tuple(int(x) for x in args.batch.split(","))
        if len(BATCH) != 2:
            ap.error("--batch takes DEPTH,SMALL_MAX")
    if "i" in args.only and not BATCH:
        ap.error("--only i needs --batch")
    if args.start6 and ORDER != 6:
        ap.error("--start6 needs --order 6")
    if capi.device_count() < 1:
        sys.exit("block_bench: no GPU")
    out = {"tool": "block_bench", "order": ORDER, "batch": list(BATCH) if BATCH else None, "watch": args.watch, "pass_precision": args.pass_precision, "full": {}, "end2end": [], "small": {}, "idle": {}}
    if "a" in args.only:
        part_a(args, out)
    if "b" in args.only:
        part_b(args, out)
    if "c" in args.only:
        part_c(args, out)
    if "i" in args.only:
        part_i(args, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
