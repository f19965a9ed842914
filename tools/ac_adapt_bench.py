#!/usr/bin/env python3
"""Measures what radii that follow a target count (Simulation.set_neighbor_adapt) cost the Ahmad-Cohen neighbour scheme on one GPU, and
prints ONE JSON line.  Workload: ic.plummer(N, seed=7) on a Hermite handle, the radius chosen (bisection on nb_neighbors' count) for a
mean count of ~32, rows of 256 or what the largest count needs, N_sub = 8, dt = 2^-10 (the lists stay what they are over the measurement).

  (a) step     one regular step, wall time with its host wait(s), per arm, the arms in turns (--rounds times), EVERY figure from a
               process of its own (a process loads one library):
                   parent      the library --parent-lib (the commit this change is based on), fixed radii
                   tree_fixed  this tree's library, fixed radii: the code the parent runs -- the spread between two libraries
                   tree_adapt  this tree's library, adaptation on, target 32, grow_max = 1 (the rule runs, no radius moves: the same
                               lists, so the same work in every other launch), no rebuild
               `ratio` = median(tree_adapt) / median(parent), bar 1.03.  Without --parent-lib the parent arm is left out and the ratio
               is against tree_fixed.
  (b) rebuild  this tree's library: the start (wall time) with rows that fit (0 rebuilds) and with rows of 64 (the core's rows overflow:
               r rebuilds, from nb_neighbor_adapt_stats), and ONE nb_split_lists pass with the same outputs by device events.
               `rebuild_ms` = (start_r - start_0) / r, `rebuild_over_pass` = rebuild_ms / pass_ms.

Every figure: at least --min-seconds of the same work before the timed run and in it.  Every child runs under its own time limit
(--step-limit seconds) and the driver starts nothing more after a child that failed.  Needs a GPU (no fallback)."""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
TARGET, NSUB, DT = 32, 8, 2.0 ** -10


def expire(what, seconds):
    sys.stderr.write("ac_adapt_bench: '%s' exceeded its limit of %g s; ending\n" % (what, seconds))
    sys.stderr.flush()
    os._exit(124)


def child(args):
    """One arm in this process; prints its JSON line."""
    guard = threading.Timer(args.step_limit, expire, (args.arm, args.step_limit))
    guard.daemon = True
    guard.start()
    import torch          # first: one HIP runtime for torch and the engine
    sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
    from nbody3d_amd import Simulation, capi, ic
    if capi.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("ac_adapt_bench: no GPU")
    n, precision = args.n, args.precision
    dt, tt = (np.float64, torch.float64) if precision == "f64" else (np.float32, torch.float32)
    stream = torch.cuda.Stream()
    b, v = ic.plummer(n, seed=7)
    out = {"arm": args.arm, "n": n, "precision": precision, "lib": capi.library_path()}
    with Simulation(n, precision=precision, stream=stream.cuda_stream, integrator="hermite4") as s:
        s.init(b.astype(dt), v.astype(dt))
        s.set_params(DT, 1.0)
        with torch.cuda.stream(stream):
            cnt = torch.zeros(n, device="cuda", dtype=torch.int32)

        def mean_count(h):
            s.neighbors_device(None, 0, None, None, cnt.data_ptr(), bodies=(0, n), radius=h)
            stream.synchronize()
            return float(cnt.double().mean().item()), int(cnt.max().item())

        def walled_steps():
            s.simulate(1); s.sync()
            t = time.perf_counter(); s.simulate(1); s.sync()
            reps = max(2, int(np.ceil(args.min_seconds / max(time.perf_counter() - t, 1e-6))))
            s.simulate(reps); s.sync()
            t = time.perf_counter(); s.simulate(reps); s.sync()
            return 1e3 * (time.perf_counter() - t) / reps

        if args.arm == "radius":
            lo, hi = 0.0, 4.0
            for _ in range(24):          # bisection: the mean count grows with the radius
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if mean_count(mid)[0] < float(TARGET) else (lo, mid)
            h = float(dt(0.5 * (lo + hi)))
            mc, mx = mean_count(h)
            out.update(radius=h, mean_count=mc, max_count=mx, cap=max(256, (mx + 32 + 63) // 64 * 64))
        elif args.arm in ("parent", "tree_fixed", "tree_adapt"):
            s.set_neighbor_scheme(radius=args.radius, substeps=NSUB, cap=args.cap)
            if args.arm == "tree_adapt":
                s.set_neighbor_adapt(TARGET, grow_max=1.0)
            out["step_ms"] = walled_steps()
            out["stats"] = s.neighbor_scheme_stats()
            if args.arm == "tree_adapt":
                out["adapt"] = s.neighbor_adapt_stats()
        elif args.arm == "rebuild":
            def start(cap):
                """ms per start (wall), and the rebuilds of one: set_neighbor_adapt stales the scheme, the download runs the start."""
                s.set_neighbor_scheme(radius=args.radius, substeps=NSUB, cap=cap)

                def once():
                    s.set_neighbor_adapt(TARGET, grow_max=1.0, max_rebuilds=16)
                    t = time.perf_counter()
                    s.neighbor_adapt_stats()                     # (no device call)
                    s.download_neighbor_radii(); s.sync()
                    return time.perf_counter() - t
                once()
                reps = max(2, int(np.ceil(args.min_seconds / max(once(), 1e-6))))
                for _ in range(reps):
                    once()
                total = sum(once() for _ in range(reps))
                return 1e3 * total / reps, s.neighbor_adapt_stats()["last_rebuilds"], s.neighbor_scheme_stats()
            small = 2 * TARGET
            out["start_0_ms"], r0, out["stats_0"] = start(args.cap)
            out["start_r_ms"], out["rebuilds"], out["stats_r"] = start(small)
            assert r0 == 0 and out["rebuilds"] >= 1, (r0, out["rebuilds"])
            with torch.cuda.stream(stream):
                lst = torch.zeros((n, args.cap), device="cuda", dtype=torch.int32)
                o = [torch.zeros((n, 4), device="cuda", dtype=tt) for _ in range(4)]
            s.set_neighbor_scheme(None)

            def one_pass():
                s.split_lists_device(0, lst.data_ptr(), args.cap, cnt.data_ptr(), bodies=(0, n), radius=args.radius, accel_irr_ptr=o[0].data_ptr(),
                                     accel_reg_ptr=o[1].data_ptr(), jerk_irr_ptr=o[2].data_ptr(), jerk_reg_ptr=o[3].data_ptr())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            one_pass(); stream.synchronize()
            e0.record(stream); one_pass(); e1.record(stream); stream.synchronize()
            reps = max(2, int(np.ceil(args.min_seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
            for _ in range(reps):
                one_pass()
            e0.record(stream)
            for _ in range(reps):
                one_pass()
            e1.record(stream); stream.synchronize()
            out["pass_ms"] = e0.elapsed_time(e1) / reps
            out["rebuild_ms"] = (out["start_r_ms"] - out["start_0_ms"]) / out["rebuilds"]
            out["rebuild_over_pass"] = out["rebuild_ms"] / out["pass_ms"]
    guard.cancel()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 262144])
    ap.add_argument("--precisions", nargs="+", default=["f32"])
    ap.add_argument("--parent-lib", default=None, help="libnbody3d_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--step-limit", type=float, default=120.0)
    ap.add_argument("--arm", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--n", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--precision", default="f32", help=argparse.SUPPRESS)
    ap.add_argument("--radius", type=float, default=0.0, help=argparse.SUPPRESS)
    ap.add_argument("--cap", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.arm:
        return child(args)

    def run(arm, n, precision, lib=None, **kw):
        env = dict(os.environ)
        env.pop("NB_ENGINE_LIB", None)
        if lib:
            env["NB_ENGINE_LIB"] = lib
        cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--n", str(n), "--precision", precision, "--min-seconds", str(args.min_seconds),
               "--step-limit", str(args.step_limit)] + [x for k, v in kw.items() for x in ("--" + k, repr(v))]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.step_limit + 60)
        line = [l for l in p.stdout.splitlines() if l.startswith("{")]
        if p.returncode != 0 or not line:      # a child that failed: nothing more is started
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit("ac_adapt_bench: arm %s n=%d ended with status %d" % (arm, n, p.returncode))
        return json.loads(line[-1])

    out = {"tool": "ac_adapt_bench", "min_seconds": args.min_seconds, "rounds": args.rounds, "target": TARGET, "substeps": NSUB, "cases": []}
    arms = (["parent"] if args.parent_lib else []) + ["tree_fixed", "tree_adapt"]
    for precision in args.precisions:
        for n in args.sizes:
            shape = run("radius", n, precision)
            kw = dict(radius=shape["radius"], cap=shape["cap"])
            case = {"precision": precision, "n": n, "radius": shape["radius"], "mean_count": shape["mean_count"], "max_count": shape["max_count"], "cap": shape["cap"]}
            ms = {a: [] for a in arms}
            for _ in range(args.rounds):
                for a in arms:
                    r = run(a, n, precision, lib=args.parent_lib if a == "parent" else None, **kw)
                    ms[a].append(r["step_ms"])
                    if a == "tree_adapt":
                        case["adapt"] = r["adapt"]
                        assert r["adapt"]["rebuilds"] == 0, r
            for a, xs in ms.items():
                case[a + "_ms"] = {"all": xs, "best": min(xs), "median": float(np.median(xs)), "spread": (max(xs) - min(xs)) / min(xs)}
            base = "parent" if args.parent_lib else "tree_fixed"
            case["ratio"] = case["tree_adapt_ms"]["median"] / case[base + "_ms"]["median"]
            case["ratio_against"] = base
            case["inside_bar"] = bool(case["ratio"] <= 1.03)
            case["rebuild"] = {k: v for k, v in run("rebuild", n, precision, **kw).items() if k not in ("arm", "n", "precision", "lib")}
            out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
