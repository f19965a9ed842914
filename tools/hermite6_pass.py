#!/usr/bin/env python3
"""Times the force+jerk+snap pass of an order-6 Hermite handle (nb_set_hermite_order(6): nb_h6_fjs_pk / nb_h6_fjs64 + nb_h6_reduce)
against the force+jerk pass of an order-4 handle on the same system and device, and prints ONE JSON line.

  ratio         nb_force_pass of the order-6 handle / nb_force_pass of the order-4 handle, per size of --sizes, f32 and f64; the two
                handles are timed in turns, --rounds times, at least --min-seconds of the same work before every timed run; best,
                median and every figure
  step parts    force_ms (kernel + reduce) and integrate_ms (predictor + corrector) of timed steps of both handles (nb_step_times2)
  --payoff N    a Plummer sphere of N bodies over --payoff-time time units, f64: |dE/E0| (KE + PE of one nb_diagnostics call, the
                state is at one instant) and the wall time of order 4 at dt = 1e-3 and of order 6 at every step of --payoff-dts

Needs a GPU (no fallback)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
from nbody3d_amd import Simulation, capi, ic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[65536, 262144])
    ap.add_argument("--precisions", nargs="*", default=["f32", "f64"])
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--payoff", type=int, default=0)
    ap.add_argument("--payoff-time", type=float, default=1.0)
    ap.add_argument("--payoff-dts", type=float, nargs="*", default=[2.0 ** -6, 2.0 ** -7, 2.0 ** -8, 2.0 ** -9])
    args = ap.parse_args()
    if capi.device_count() < 1:
        sys.exit("hermite6_pass: no GPU")
    out = {"tool": "hermite6_pass", "min_seconds": args.min_seconds, "rounds": args.rounds, "sizes": {}}

    def force_pass(s):
        est = s.force_pass(2)
        reps = max(2, int(np.ceil(args.min_seconds * 1e3 / est)))
        s.force_pass(reps)                      # warm: at least min_seconds of the same work
        return s.force_pass(reps)

    for prec in args.precisions:
        for n in args.sizes:
            b, v = ic.plummer(n, seed=1)
            with Simulation(n, precision=prec, integrator="hermite4") as h4, Simulation(n, precision=prec, integrator="hermite6") as h6:
                for s in (h4, h6):
                    s.init(b, v)
                    s.set_params(1e-3, 1.0)
                got = {"order4": [], "order6": []}
                for _ in range(args.rounds):
                    got["order4"].append(force_pass(h4))
                    got["order6"].append(force_pass(h6))
                r = {"order4_variant": h4.variant, "order6_variant": h6.variant, "order4_shape": h4.shape_info(), "order6_shape": h6.shape_info()}
                for k, x in got.items():
                    r[k] = {"best_ms": min(x), "median_ms": float(np.median(x)), "all_ms": x}
                r["ratio"] = r["order6"]["median_ms"] / r["order4"]["median_ms"]
                r["ratio_best"] = r["order6"]["best_ms"] / r["order4"]["best_ms"]
                r["pairs_per_s"] = float(n) * n / (r["order6"]["median_ms"] * 1e-3)
                for name, s in (("order4_step", h4), ("order6_step", h6)):
                    s.enable_timing(True)
                    s.simulate(6)
                    t = s.step_breakdown()
                    r[name] = {k: t[k] for k in ("launches", "force_ms", "integrate_ms", "span_ms")}
                out["sizes"]["%s_%d" % (prec, n)] = r

    if args.payoff:
        n = args.payoff
        b, v = ic.plummer(n, seed=1)
        out["payoff"] = {"n": n, "time": args.payoff_time, "precision": "f64", "runs": []}
        for order, dt in [(4, 1e-3)] + [(6, d) for d in args.payoff_dts]:
            steps = int(round(args.payoff_time / dt))
            with Simulation(n, precision="f64", integrator="hermite%d" % order) as s:
                s.init(b, v)
                s.set_params(dt, 1.0)
                ke, pe, _ = s.diagnostics()
                e0 = ke + pe
                s.read_jerk()                   # the start is not part of the timed steps
                if order == 6:
                    s.read_snap()
                s.sync()
                t0 = time.perf_counter()
                s.simulate(steps)
                s.sync()
                wall = time.perf_counter() - t0
                ke, pe, _ = s.diagnostics()
                out["payoff"]["runs"].append({"order": order, "dt": dt, "steps": steps, "wall_s": wall, "dE_over_E0": abs((ke + pe - e0) / e0)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
