#!/usr/bin/env python3
"""Measures the guarded sums of the mixed-precision force+jerk pass (Simulation.set_pass_guard(r_near): nb_mxg_fj +
nb_fj_reduce<double, double>) on one GPU and prints ONE JSON line.  The arms -- plain mixed, guarded, native f64 -- hold the same
system and are timed in turns in one process, as tools/mixed_bench.py does.  Every handle has eps2 = 1e-8; r_near is a quarter of
the mean interparticle distance inside the half-mass radius r_h, 0.25 r_h (8 pi / (3 N))^(1/3).

  (a) pass     nb_force_pass at each N of --sizes on ic.plummer and on the same with 1 % of the bodies as pairs at +-0.001; --rounds
               times, at least --min-seconds of the same work before every timed run; the ratios guarded / mixed and guarded / f64,
               and the share of (wave, stage) slots that take the slow sums, counted on the CPU from the fixture
  (b) small    microseconds per block step with |A| = 64 at N = --full-n by tools/block_bench.py's method (frozen levels)
  (c) payoff   ic.plummer(--payoff-n) with 1 % of the bodies as pairs at +-0.0001, dynamic levels, eta 0.02, outer step 2^-4,
               max_level 16, one time unit: wall time, block and body steps, |dE/E0|, and the largest distance of a pair's
               barycentre from the native run's at the end

  --loops      no GPU: the fast and the slow path of the built stage loops (csrc/nb_engine.gfx950.s from `make asm`), issue cycles
               by DESIGN 4.1's accounting, and the factors of the bar

Parts (a) to (c) need a GPU (no fallback)."""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARMS = ("mixed", "guarded", "f64")
EPS2 = 1e-8
ROWS, WAVE_ROWS, STAGE = 1024, 64, 2      # nb_mxg_fj<2>: i-rows per workgroup; consecutive rows per wave and packed half; j-bodies per stage


def quarter_spacing(b):
    x, m = np.asarray(b, np.float64)[:, :3], np.asarray(b, np.float64)[:, 3]
    r = np.sqrt(((x - (m[:, None] * x).sum(0) / m.sum()) ** 2).sum(1))
    return float(0.25 * np.median(r) * (8 * np.pi / (3 * len(x))) ** (1.0 / 3.0))


def slow_share(b, r_near, eps2=EPS2):
    """The share of (wave, stage) slots of the full pass in which some lane has a near pair: d^2 + eps2 < r_near^2, the self pair
    included.  Row i belongs to wave (i // 1024, (i % 256) // 64) -- a lane holds rows tid, tid + 256, tid + 512, tid + 768 of its
    workgroup --, body j to stage j // 2."""
    from scipy.spatial import cKDTree
    x = np.asarray(b, np.float64)[:, :3]
    n = len(x)
    if r_near * r_near <= eps2:
        return 0.0
    p = cKDTree(x).query_pairs(np.sqrt(r_near * r_near - eps2), output_type="ndarray")
    i = np.concatenate([p[:, 0], p[:, 1], np.arange(n)])
    j = np.concatenate([p[:, 1], p[:, 0], np.arange(n)])
    wave = (i // ROWS) * (256 // WAVE_ROWS) + (i % 256) // WAVE_ROWS
    slots = np.unique(wave * (n // STAGE + 1) + j // STAGE)
    waves = -(-n // ROWS) * (256 // WAVE_ROWS)
    return float(len(slots)) / (waves * -(-n // STAGE))


def handle(arm, n, r_near):
    from nbody3d_amd import Simulation
    sim = Simulation(n, precision="f64", integrator="hermite4", eps2=EPS2)
    if arm != "f64":
        sim.set_pass_precision("mixed")
    if arm == "guarded":
        sim.set_pass_guard(r_near)
    return sim


def stats(x):
    return {"best": min(x), "median": float(np.median(x)), "all": x}


def part_a(args, out):
    from nbody3d_amd import ic
    from block_bench import with_tight_pairs

    def force_pass(s):
        est = s.force_pass(2)
        reps = max(2, int(np.ceil(args.min_seconds * 1e3 / est)))
        s.force_pass(reps)                      # warm: at least min_seconds of the same work
        return s.force_pass(reps)

    for n in args.sizes:
        for system in ("plummer", "pairs"):
            b, v = ic.plummer(n, seed=1) if system == "plummer" else with_tight_pairs(n, half=0.001)
            r_near = quarter_spacing(b)
            sims = {arm: handle(arm, n, r_near) for arm in ARMS}
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
                r["r_near"] = r_near
                r["slow_share"] = slow_share(b, r_near)
                r["guarded_over_mixed"] = r["guarded_ms"]["median"] / r["mixed_ms"]["median"]
                r["guarded_over_f64"] = r["guarded_ms"]["median"] / r["f64_ms"]["median"]
                out["pass"]["%d_%s" % (n, system)] = r
            finally:
                for s in sims.values():
                    s.close()


def part_b(args, out):
    from nbody3d_amd import ic
    from block_bench import wall
    n, L, k = args.full_n, 6, 64
    b, v = ic.plummer(n, seed=1)
    r_near = quarter_spacing(b)
    lev = np.zeros(n, np.uint8)
    lev[np.random.default_rng(5).choice(n, k, replace=False)] = L
    cases = (("all_level0", np.zeros(n, np.uint8)), ("64_at_level6", lev))
    sims = {arm: handle(arm, n, r_near) for arm in ARMS}
    try:
        for s in sims.values():
            s.init(b, v)
            s.set_params(1e-3, 1.0)
            s.set_block_steps(max_level=L, frozen=True)
        runs = {arm: {name: [] for name, _ in cases} for arm in ARMS}
        for rnd in range(args.rounds + 1):      # the first round warms every shape
            for arm in ARMS:
                for name, levels in cases:
                    sims[arm].upload_levels(levels)      # the same state of the levels' clock before every timed run
                    t = wall(sims[arm], args.small_outer) / args.small_outer
                    if rnd:
                        runs[arm][name].append(1e6 * t)
        out["small"]["r_near"] = r_near
        for arm in ARMS:
            t = {name: stats(x) for name, x in runs[arm].items()}
            t["us_per_small_block_step"] = (t["64_at_level6"]["median"] - t["all_level0"]["median"]) / (2 ** L - 1)
            out["small"][arm] = t
    finally:
        for s in sims.values():
            s.close()


def part_c(args, out):
    from block_bench import energy, wall, with_tight_pairs
    n = args.payoff_n
    b, v = with_tight_pairs(n, half=0.0001)
    pairs = int(0.01 * n) // 2
    r_near = quarter_spacing(b)
    dt = 2.0 ** -4
    outer = int(round(args.payoff_time / dt))
    out["payoff"] = {"n": n, "pairs": pairs, "pair_half": 0.0001, "eps2": EPS2, "eta": 0.02, "outer_dt": dt, "max_level": 16,
                     "time": args.payoff_time, "r_near": r_near, "runs": {}}
    centres = {}
    for arm in ("f64", "mixed", "guarded"):
        with handle(arm, n, r_near) as sim:
            sim.init(b, v)
            sim.set_params(dt, 1.0)
            sim.set_block_steps(eta=0.02, max_level=16)
            e0 = energy(sim)
            sim.read_levels()                       # the start is not part of the timed steps
            sim.block_stats(reset=True)
            t = wall(sim, outer)
            x = np.asarray(sim.read()[0], np.float64)
            m0, m1 = x[0:2 * pairs:2, 3:4], x[1:2 * pairs:2, 3:4]
            centres[arm] = (m0 * x[0:2 * pairs:2, :3] + m1 * x[1:2 * pairs:2, :3]) / (m0 + m1)
            out["payoff"]["runs"][arm] = {"wall_s": t, "dE": abs((energy(sim) - e0) / e0), "stats": sim.block_stats(), "variant": sim.variant,
                                          "max_barycentre_distance_from_f64": float(np.sqrt(((centres[arm] - centres["f64"]) ** 2).sum(1)).max())}


def loop_paths(body):
    """The stage loop's instructions along its fast path (every mask branch taken) and its slow path (none taken; the branch on a
    non-empty exec behind the slow sums always is): tests/test_guard_cpu.py's walk."""
    lines = [l.split(";")[0].strip() for l in body.splitlines()]
    lines = [l for l in lines if l and (not l.startswith(".") or l.startswith(".LBB"))]
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    first = next(i for i, l in enumerate(lines) if l.startswith("v_rsq_f32"))
    start = max(i for i in labels.values() if i < first)
    paths = {}
    for fast in (True, False):
        i, ops = start + 1, []
        while len(ops) < 10000:
            l = lines[i]
            if l.endswith(":"):
                if i == start:
                    break
                i += 1
                continue
            op = l.split()[0]
            ops.append(op)
            if op == "s_cbranch_vccz" and lines[i - 1].startswith("s_or_b64 vcc"):
                i = labels[l.split()[1]] if fast else i + 1
            elif op == "s_branch" or (op == "s_cbranch_execnz" and not fast):
                i = labels[l.split()[1]]
            elif op.startswith("s_cbranch") and labels[l.split()[1]] <= i:
                break
            else:
                i += 1
        valu = [o for o in ops if o.startswith("v_")]
        rsq = sum(o.startswith("v_rsq_f32") for o in valu)
        paths["fast" if fast else "slow"] = {
            "instructions": len(ops), "valu": len(valu), "v_pk": sum(o.startswith("v_pk_") for o in valu), "v_rsq_f32": rsq,
            "v_cmp": sum(o.startswith("v_cmp_") for o in valu), "v_cndmask": sum(o.startswith("v_cndmask") for o in valu),
            "ds": sum(o.startswith("ds_") for o in ops), "salu": sum(o.startswith("s_") for o in ops),
            "issue_cycles_per_two_pairs": ((len(valu) - rsq) * 4 + rsq * 8) / (rsq / 2.0)}
    return paths


def loops():
    text = open(os.path.join(ROOT, "nbody3d-webgpu_amd", "csrc", "nb_engine.gfx950.s")).read()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN2nb\d+nb_\w+):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M)}
    out = {}
    for name in ("nb_mx_fjILi2E", "nb_mxg_fjILi2E", "nb_mx_blk_fjILi1E", "nb_mxg_blk_fjILi1E"):
        p = loop_paths(next(v for k, v in bodies.items() if name in k))
        out[name] = p if "mxg" in name else {"fast": p["fast"]}
    cyc = lambda k, path: out[k][path]["issue_cycles_per_two_pairs"]
    out["fast_ratio"] = cyc("nb_mxg_fjILi2E", "fast") / cyc("nb_mx_fjILi2E", "fast")
    out["slow_ratio"] = cyc("nb_mxg_fjILi2E", "slow") / cyc("nb_mxg_fjILi2E", "fast")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", action="store_true")
    ap.add_argument("--only", choices=["a", "b", "c"], nargs="*", default=["a", "b", "c"])
    ap.add_argument("--sizes", type=int, nargs="*", default=[65536, 262144])
    ap.add_argument("--full-n", type=int, default=65536)
    ap.add_argument("--payoff-n", type=int, default=16384)
    ap.add_argument("--payoff-time", type=float, default=1.0)
    ap.add_argument("--small-outer", type=int, default=20)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.loops:
        print(json.dumps({"tool": "guard_bench", "loops": loops()}))
        return
    from nbody3d_amd import capi
    if capi.device_count() < 1:
        sys.exit("guard_bench: no GPU")
    out = {"tool": "guard_bench", "min_seconds": args.min_seconds, "rounds": args.rounds, "pass": {}, "small": {}}
    if "a" in args.only:
        part_a(args, out)
    if "b" in args.only:
        part_b(args, out)
    if "c" in args.only:
        part_c(args, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
