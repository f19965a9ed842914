#!/usr/bin/env python3
"""Measures the mixed-precision force+jerk pass of f64 Hermite handles (Simulation.set_pass_precision("mixed"): nb_mx_fj +
nb_fj_reduce<float, double>) on one GPU and prints ONE JSON line.

  (a) pass     nb_force_pass at each N of --sizes on three handles holding the same system: the mixed handle, the native f64 handle
               (nb_fj64) and an f32 Hermite handle (nb_fj_pk); the arms are timed in turns in one process, --rounds times, at least
               --min-seconds of the same work before every timed run; best, median and every figure, the ratios mixed / f32 and
               mixed / f64
  (b) small    microseconds per block step with |A| = 64 at N = --full-n, by tools/block_bench.py's method (frozen levels: 64 bodies
               at level 6 against every body at level 0), on a mixed and on a native f64 handle, in turns
  (c) payoff   tools/block_bench.py's hard-pair workload (ic.plummer(--payoff-n), 1 % of the bodies as pairs at +-0.001, eps2 1e-8,
               dynamic levels, eta 0.02, outer step 2^-4, max_level 16, one time unit) on a mixed handle, a native f64 handle and an
               f32 handle: wall time, block and body steps, |dE/E0| from nb_diagnostics

Needs a GPU (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from nbody3d_amd import Simulation, capi, ic  # noqa: E402
from block_bench import energy, wall, with_tight_pairs  # noqa: E402

ARMS = ("mixed", "f64", "f32")


def handle(arm, n, eps2=None):
    sim = Simulation(n, precision="f32" if arm == "f32" else "f64", integrator="hermite4", eps2=eps2)
    if arm == "mixed":
        sim.set_pass_precision("mixed")
    return sim


def stats(x):
    return {"best": min(x), "median": float(np.median(x)), "all": x}


def part_a(args, out):
    def force_pass(s):
        est = s.force_pass(2)
        reps = max(2, int(np.ceil(args.min_seconds * 1e3 / est)))
        s.force_pass(reps)                      # warm: at least min_seconds of the same work
        return s.force_pass(reps)

    for n in args.sizes:
        b, v = ic.plummer(n, seed=1)
        sims = {arm: handle(arm, n) for arm in ARMS}
        try:
            for s in sims.values():
                s.init(b, v)
                s.set_params(1e-3, 1.0)
            got = {arm: [] for arm in ARMS}
            for _ in range(args.rounds):
                for arm in ARMS:
                    got[arm].append(force_pass(sims[arm]))
            r = {arm + "_ms": stats(x) for arm, x in got.items()}
            r["variants"] = {arm: s.variant for arm, s in sims.items()}
            r["shapes"] = {arm: s.shape_info() for arm, s in sims.items()}
            r["mixed_over_f32"] = r["mixed_ms"]["median"] / r["f32_ms"]["median"]
            r["mixed_over_f64"] = r["mixed_ms"]["median"] / r["f64_ms"]["median"]
            r["mixed_pairs_per_s"] = float(n) * n / (r["mixed_ms"]["median"] * 1e-3)
            out["pass"][str(n)] = r
        finally:
            for s in sims.values():
                s.close()


def part_b(args, out):
    n, L, k = args.full_n, 6, 64
    b, v = ic.plummer(n, seed=1)
    lev = np.zeros(n, np.uint8)
    lev[np.random.default_rng(5).choice(n, k, replace=False)] = L
    cases = (("all_level0", np.zeros(n, np.uint8)), ("64_at_level6", lev))
    arms = ("mixed", "f64")
    sims = {arm: handle(arm, n) for arm in arms}
    try:
        for s in sims.values():
            s.init(b, v)
            s.set_params(1e-3, 1.0)
            s.set_block_steps(max_level=L, frozen=True)
        runs = {arm: {name: [] for name, _ in cases} for arm in arms}
        for rnd in range(args.rounds + 1):      # the first round warms every shape
            for arm in arms:
                for name, levels in cases:
                    sims[arm].upload_levels(levels)      # the same state of the levels' clock before every timed run
                    t = wall(sims[arm], args.small_outer) / args.small_outer
                    if rnd:
                        runs[arm][name].append(1e6 * t)
        for arm in arms:
            t = {name: stats(x) for name, x in runs[arm].items()}
            t["us_per_small_block_step"] = (t["64_at_level6"]["median"] - t["all_level0"]["median"]) / (2 ** L - 1)
            out["small"][arm] = t
    finally:
        for s in sims.values():
            s.close()


def part_c(args, out):
    n = args.payoff_n
    b, v = with_tight_pairs(n, half=0.001)
    dt = 2.0 ** -4
    outer = int(round(args.payoff_time / dt))
    out["payoff"] = {"n": n, "pairs": int(0.01 * n) // 2, "pair_half": 0.001, "eps2": 1e-8, "eta": 0.02, "outer_dt": dt, "max_level": 16,
                     "time": args.payoff_time, "runs": {}}
    for arm in ARMS:
        with handle(arm, n, 1e-8) as sim:
            sim.init(b, v)
            sim.set_params(dt, 1.0)
            sim.set_block_steps(eta=0.02, max_level=16)
            e0 = energy(sim)
            sim.read_levels()                       # the start is not part of the timed steps
            sim.block_stats(reset=True)
            t = wall(sim, outer)
            out["payoff"]["runs"][arm] = {"wall_s": t, "dE": abs((energy(sim) - e0) / e0), "stats": sim.block_stats(), "variant": sim.variant}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["a", "b", "c"], nargs="*", default=["a", "b", "c"])
    ap.add_argument("--sizes", type=int, nargs="*", default=[65536, 262144])
    ap.add_argument("--full-n", type=int, default=65536)
    ap.add_argument("--payoff-n", type=int, default=16384)
    ap.add_argument("--payoff-time", type=float, default=1.0)
    ap.add_argument("--small-outer", type=int, default=20)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if capi.device_count() < 1:
        sys.exit("mixed_bench: no GPU")
    out = {"tool": "mixed_bench", "min_seconds": args.min_seconds, "rounds": args.rounds, "pass": {}, "small": {}}
    if "a" in args.only:
        part_a(args, out)
    if "b" in args.only:
        part_b(args, out)
    if "c" in args.only:
        part_c(args, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
