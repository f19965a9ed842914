#!/usr/bin/env python3
"""Measures the record of the tests of the neighbour scheme's block individual irregular steps (tests/ac_levels_ref.py) ->
tests/golden/ac_levels.json and the restatement's final states tests/golden/ac_levels_<fixture>_m<min_level>.npy.  CPU only, a
few minutes.

For the three fixtures of ac_ref.SETUP with their recorded radii (tests/golden/ac_scheme.json), L = 6, eta = 0.02, min_level 0
and 2, 4 regular steps with dynamic levels, it records the final levels, both stats, the smallest decision margin (the relative
distance of any finite tau from a level boundary) and the smallest membership margin of the fp64 run and of the binary32-storing
one, the error of the binary32-storing restatement against the fp64 one, the number of final levels in which the two differ, and
the position error against the shared scheme at N_sub = 64 next to that of the shared scheme at N_sub = 2^min_level.  It ASSERTS
what the GPU comparison of every final level and counter rests on: noise of 1e-12 of max |a|, max |j| on every list sum, three
seeds, changes no level and no counter; the membership margin is >= 1e-3; no row is over cap.

    python tests/golden/measure_ac_levels.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "nbody3d-webgpu_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ac_levels_ref as LR  # noqa: E402
import ac_ref as R  # noqa: E402
from block_ref import norm_err  # noqa: E402

NOISE, SEEDS = 1e-12, (1, 2, 3)


def main():
    rec = R.record()
    out = {"L": LR.L_REC, "eta": LR.ETA_REC, "steps": LR.STEPS_REC, "eps2": R.EPS2, "noise": NOISE, "seeds": list(SEEDS), "runs": {}}
    for name in R.FIXTURES:
        e = rec["fixtures"][name]
        b, v = R.fixture(name)
        kw = R.radius_args(len(b), e["per_body"], e["radius"])
        run = lambda **k: LR.ac_levels_ref(b, v, e["G"], R.EPS2, e["dt"], LR.STEPS_REC, L=LR.L_REC, cap=e["cap"], eta=LR.ETA_REC, **kw, **k)
        fine = R.ac_ref(b, v, e["G"], R.EPS2, e["dt"], LR.STEPS_REC, substeps=2 ** LR.L_REC, cap=e["cap"], **kw)[0][:, :3]
        for m in LR.MIN_LEVELS_REC:
            mm, dm, mm32, dm32 = [], [], [], []
            o64 = run(min_level=m, margins=mm, dmargins=dm)
            o32 = run(min_level=m, margins=mm32, dmargins=dm32, store=np.float32)
            t64, t32 = R.totals(o64), R.totals(o32, np.float32)
            np.save(LR.state_path(name, m), np.concatenate(t64, axis=1))
            shared = R.ac_ref(b, v, e["G"], R.EPS2, e["dt"], LR.STEPS_REC, substeps=2 ** m, cap=e["cap"], **kw)[0][:, :3]
            ent = {"n": len(b), "min_level": m, "levels": [int(z) for z in o64[8]], "scheme_stats": o64[9], "level_stats": o64[10],
                   "decision_margin": float(min(dm)), "membership_margin": float(min(mm + mm32)), "max_count": int(o64[9]["max_count"]),
                   "f32_err": {q: norm_err(t32[i], t64[i]) for i, q in enumerate(R.QUANTITIES)},
                   "f32_levels_differ": int((o64[8] != o32[8]).sum()),
                   "err_vs_fine": norm_err(o64[0][:, :3], fine), "shared_err_vs_fine": norm_err(shared, fine), "noise_flips": 0}
            for seed in SEEDS:
                on = run(min_level=m, noise=(NOISE, np.random.default_rng(seed)))
                flips = int((on[8] != o64[8]).sum()) + int(on[10] != o64[10])
                ent["noise_flips"] += flips
                assert flips == 0, (name, m, seed, "noise of %g changed a level or a counter: choose another eta or dt" % NOISE)
            assert ent["membership_margin"] >= 1e-3, (name, m, ent["membership_margin"])
            assert ent["max_count"] <= e["cap"] and o64[9]["overflowed"] == 0, (name, m)
            out["runs"]["%s_m%d" % (name, m)] = ent
            ls = o64[10]
            print("%-12s min_level %d: block steps %d of %d ticks, body-steps %d, entries %d, clamped %d, finest %d; margins: decision %.3g "
                  "membership %.3g; err vs N_sub=64 %.3g (shared N_sub=%d: %.3g); f32 err x %.3g, levels differ %d"
                  % (name, m, ls["block_steps"], ls["ticks"], ls["body_steps"], ls["entries"], ls["clamped"], ls["finest_level"],
                     ent["decision_margin"], ent["membership_margin"], ent["err_vs_fine"], 2 ** m, ent["shared_err_vs_fine"],
                     ent["f32_err"]["x"], ent["f32_levels_differ"]))
    with open(LR.JSON_PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
