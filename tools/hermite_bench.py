#!/usr/bin/env python3
"""Times the force+jerk pass of a Hermite handle (integrator="hermite4") against the ordered-pair force pass of a leapfrog handle
(NB_FLAG_NO_SYM) on the same system and device, and prints ONE JSON line.

  ratio         nb_force_pass of the Hermite handle (nb_fj_pk / nb_fj64 + nb_fj_reduce) / nb_force_pass of the leapfrog handle,
                per size of --sizes (f32) and --sizes-f64 (information only); the two handles are timed in turns, --rounds times,
                at least --min-seconds of the same work before every timed run; best and median
  step parts    force_ms (kernel + reduce) and integrate_ms (predictor + corrector) of timed Hermite steps (nb_step_times2)
  --energy N    |dE/E0| over --energy-steps steps of dt = 1e-3 at N bodies, sampled every 50 steps with nb_diagnostics: Hermite (state
                at one instant: KE + PE of the same call) and leapfrog (Simulation.energy_drift's lagged bookkeeping), f32 and f64

Needs a GPU (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))
from nbody3d_amd import Simulation, capi, ic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[65536, 262144])
    ap.add_argument("--sizes-f64", type=int, nargs="*", default=[65536])
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--energy", type=int, default=0)
    ap.add_argument("--energy-steps", type=int, default=400)
    args = ap.parse_args()
    if capi.device_count() < 1:
        sys.exit("hermite_bench: no GPU")
    out = {"tool": "hermite_bench", "min_seconds": args.min_seconds, "rounds": args.rounds, "sizes": {}}

    def force_pass(s):
        est = s.force_pass(2)
        reps = max(2, int(np.ceil(args.min_seconds * 1e3 / est)))
        s.force_pass(reps)
        return s.force_pass(reps)

    for prec, sizes in (("f32", args.sizes), ("f64", args.sizes_f64)):
        for n in sizes:
            b, v = ic.plummer(n, seed=1)
            with Simulation(n, precision=prec, integrator="hermite4") as h, Simulation(n, precision=prec, flags=capi.NB_FLAG_NO_SYM) as l:
                for s in (h, l):
                    s.init(b, v)
                    s.set_params(1e-3, 1.0)
                got = {"hermite": [], "leapfrog": []}
                for _ in range(args.rounds):
                    got["leapfrog"].append(force_pass(l))
                    got["hermite"].append(force_pass(h))
                r = {"hermite_variant": h.variant, "leapfrog_variant": l.variant, "shape": h.shape_info()}
                for k, x in got.items():
                    r[k] = {"best_ms": min(x), "median_ms": float(np.median(x)), "all_ms": x}
                r["ratio"] = r["hermite"]["median_ms"] / r["leapfrog"]["median_ms"]
                r["ratio_best"] = r["hermite"]["best_ms"] / r["leapfrog"]["best_ms"]
                r["pairs_per_s"] = float(n) * n / (r["hermite"]["median_ms"] * 1e-3)
                h.enable_timing(True)
                h.simulate(8)
                t = h.step_breakdown()
                r["step"] = {k: t[k] for k in ("launches", "force_ms", "integrate_ms", "span_ms")}
                out["sizes"]["%s_%d" % (prec, n)] = r

    if args.energy:
        n, every = args.energy, 50
        b, v = ic.plummer(n, seed=1)
        out["energy"] = {"n": n, "steps": args.energy_steps, "dt": 1e-3, "every": every}
        for prec in ("f32", "f64"):
            with Simulation(n, precision=prec, integrator="hermite4") as h:
                h.init(b, v)
                h.set_params(1e-3, 1.0)
                ke, pe, _ = h.diagnostics()
                e0, drift = ke + pe, []
                for _ in range(args.energy_steps // every):
                    h.simulate(every)
                    ke, pe, _ = h.diagnostics()
                    drift.append(abs((ke + pe - e0) / e0))
                out["energy"]["hermite4_" + prec] = drift
            with Simulation(n, precision=prec) as l:
                l.init(b, v)
                l.set_params(1e-3, 1.0)
                out["energy"]["leapfrog_" + prec] = l.energy_drift(args.energy_steps, every)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
