#!/usr/bin/env python3
"""Measures the tolerances of the nb_split_force census (tests/split_force_ref.py) -> tests/golden/split_force_census.json.  CPU only,
about a minute.

Inputs: census_ref.bodies(n, 5) / velocities(n, 5) for n = 77, 1025, 4099, G = 0.37, eps2 = 1e-4; radii of 1.6 and 2.4 lattice
spacings, at the bodies and at 300 arbitrary points with list_force_ref.point_velocities.  Every input goes through a binary32
restatement of the kernel's sums (plain d2, rho^2 = d2 + eps2, one ordered ascending sum per side); recorded per input and per
output (accel_irr, accel_reg, jerk_irr, jerk_reg; at the bodies and, pt_*, at the points): the worst row error of that arithmetic
against numpy fp64, tol = 8 x that error, and boundary_share, the smallest share of its row's scale held by any of the 8 pairs nearest
the radius on either side.  The kernels are held to `tol`; it is never derived from a device's output.  Also recorded: the
cancellation figure (split_force_ref.measure_cancellation) -- the regular sums of a Plummer sphere taken as binary32 (full -
irregular) and by the split restatement, both against fp64.

    python tests/golden/measure_split_force.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "nbody3d-webgpu_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import split_force_ref  # noqa: E402

out = split_force_ref.measure_all()
with open(split_force_ref.JSON_PATH, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
for e in out["inputs"]:
    for pre in ("", "pt_"):
        print("n=%-5d %.1f spacings %-6s mean count %5.1f  " % (e["n"], e["spacings"], pre or "bodies", e["points_mean_count" if pre else "mean_count"])
              + "  ".join("%s: fp32 %.3g share %.3g (%.0f x tol)" % (k, e[pre + k + "_ref_f32_err"], e[pre + k + "_boundary_share"],
                                                                   e[pre + k + "_boundary_share"] / e[pre + k + "_tol"])
                          for k in split_force_ref.OUTPUTS))
c = out["cancellation"]
print("cancellation: plummer(%d, seed=%d), radius %.6g (mean count %.1f)" % (c["n"], c["seed"], c["radius"], c["mean_count"]))
for kind in ("accel", "jerk"):
    print("  regular %-5s  full - irregular: worst %.3g median %.3g    split: worst %.3g median %.3g"
          % (kind, c[kind]["subtract"]["worst"], c[kind]["subtract"]["median"], c[kind]["split"]["worst"], c[kind]["split"]["median"]))
