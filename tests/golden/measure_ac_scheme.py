#!/usr/bin/env python3
"""Measures the record of the Ahmad-Cohen neighbour scheme's tests (tests/ac_ref.py) -> tests/golden/ac_scheme.json and the
restatement's final states tests/golden/ac_scheme_<fixture>_s<substeps>.npy.  CPU only, a few minutes.

Fixtures: the first 256 and all 1,024 rows of plummer1024_* (G = 1, dt = 1/64) and disk771_* (its manifest's G, dt = 1/256, one
radius per body: base x (1, 1.25, 0.75, 0) by index mod 4), 4 regular steps, N_sub = 1, 2, 8, cap 24.  Per fixture the radius (or
base) is chosen by a scan: the pair distances along a fine shared-step Hermite run give, for every candidate, the smallest
|d2 / h2 - 1| at the build times; the largest candidate whose smallest margin is >= 3e-3 there is then RUN, in fp64 and storing
binary32, for every N_sub, and the script asserts on the runs themselves that the smallest margin is >= 1e-3 -- neither a
binary32 run nor another order of additions can then flip a membership -- and that the largest count is <= cap.  Recorded per run:
the error of the binary32-storing restatement against the fp64 one (norm_err of x, v, ai + ar, ji + jr), the smallest margin, the
largest count, and the stats the engine must reproduce exactly (entries, builds, max_count).

Also recorded: the all-members limit (n = 77, every other body in every row, N_sub = 4) against a plain shared step of dt / 4, in
fp64 and storing binary32; and the error ratio per halving of dt on plummer256 at N_sub = 8 (against the scheme at dt / 8).

    python tests/golden/measure_ac_scheme.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "nbody3d-webgpu_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ac_ref as R  # noqa: E402
from block_ref import block_ref, hermite_ref, norm_err  # noqa: E402

SETUP = R.SETUP


def scan(name, cfg):
    """The largest candidate radius (or base) whose smallest margin along a fine Hermite run is >= 3e-3 and whose counts fit."""
    b, v = R.fixture(name)
    states = [np.array(b, np.float64)]
    bb, vv, aj = b, v, None
    for _ in range(R.STEPS):
        bb, vv, a, j = hermite_ref(bb, vv, cfg["G"], R.EPS2, cfg["dt"] / 8, 8, aj)
        aj = (a, j)
        states.append(bb.copy())
    f = R.radii_pattern(len(b)) if cfg["per_body"] else np.ones(len(b))
    d2 = []
    for s in states:
        d = s[None, :, :3] - s[:, None, :3]
        q = (d * d).sum(2)
        np.fill_diagonal(q, np.inf)
        d2.append(q)
    best = None
    for h in np.geomspace(cfg["scan"][0], cfg["scan"][1], 600):
        h2 = ((f * h) ** 2)[:, None]
        ok = (h2 > 0) & np.ones_like(d2[0], bool)
        margin = min(float(np.abs(q[ok] / np.broadcast_to(h2, q.shape)[ok] - 1.0).min()) for q in d2)
        count = max(int((q < h2).sum(1).max()) for q in d2)
        if margin >= 3e-3 and count <= cfg["cap"]:
            best = float(np.float32(h))
    assert best is not None, "no candidate radius for " + name
    return best


def main():
    out = {"steps": R.STEPS, "substeps": list(R.SUBSTEPS), "eps2": R.EPS2, "fixtures": {}}
    for name in R.FIXTURES:
        cfg = dict(SETUP[name])
        h = scan(name, cfg)
        b, v = R.fixture(name)
        kw = R.radius_args(len(b), cfg["per_body"], h)
        ent = {"n": len(b), "G": cfg["G"], "dt": cfg["dt"], "cap": cfg["cap"], "per_body": cfg["per_body"], "radius": h, "runs": {}}
        for ns in R.SUBSTEPS:
            m64, m32, c64, c32 = [], [], [], []
            o64 = R.ac_ref(b, v, cfg["G"], R.EPS2, cfg["dt"], R.STEPS, substeps=ns, cap=cfg["cap"], margins=m64, counts=c64, **kw)
            o32 = R.ac_ref(b, v, cfg["G"], R.EPS2, cfg["dt"], R.STEPS, substeps=ns, cap=cfg["cap"], margins=m32, counts=c32,
                           store=np.float32, **kw)
            t64, t32 = R.totals(o64), R.totals(o32, np.float32)
            np.save(R.state_path(name, ns), np.concatenate(t64, axis=1))
            run = {"f32_err": {q: norm_err(t32[i], t64[i]) for i, q in enumerate(R.QUANTITIES)},
                   "margin": min(m64 + m32), "max_count": max(c64 + c32),
                   "entries": o64[8]["entries"], "builds": o64[8]["builds"], "last_max_count": o64[8]["max_count"],
                   "mean_count": float(o64[7].mean())}
            assert run["margin"] >= 1e-3, (name, ns, run["margin"])
            assert run["max_count"] <= cfg["cap"], (name, ns, run["max_count"])
            assert o64[8]["entries"] == o32[8]["entries"] and (o64[6] == o32[6]).all(), "binary32 decided a membership differently"
            ent["runs"][str(ns)] = run
            print("%-12s radius %.6g N_sub %d: margin %.3g  max count %d  mean %.2f  f32 err x %.3g v %.3g a %.3g j %.3g"
                  % (name, h, ns, run["margin"], run["max_count"], run["mean_count"], *[run["f32_err"][q] for q in R.QUANTITIES]))
        ent["margin"] = min(r["margin"] for r in ent["runs"].values())
        ent["max_count"] = max(r["max_count"] for r in ent["runs"].values())
        out["fixtures"][name] = ent

    # every other body in every row: the substeps are Hermite steps of hs
    A = R.ALL_MEMBERS
    b, v = R.fixture("plummer1024")
    b, v = b[:A["n"]].copy(), v[:A["n"]].copy()
    ent = dict(A)
    runs = {}
    for store, key in ((np.float64, "diff_f64"), (np.float32, "diff_f32")):
        o = R.ac_ref(b, v, A["G"], R.EPS2, A["dt"], R.STEPS, substeps=A["substeps"], cap=A["cap"], radius=A["radius"], store=store)
        assert int(o[7].min()) == A["n"] - 1
        hh = block_ref(b, v, A["G"], R.EPS2, A["dt"] / A["substeps"], R.STEPS * A["substeps"], max_level=0, min_level=0, frozen=True, store=store)
        ent[key] = {"x": norm_err(o[0][:, :3], hh[0][:, :3]), "v": norm_err(o[1][:, :3], hh[1][:, :3])}
        runs[key] = (o, hh)
        print("all members, %s: scheme against a shared step of dt / %d: x %.3g v %.3g" % (key, A["substeps"], ent[key]["x"], ent[key]["v"]))
    # what storing binary32 costs either integrator here (the two binary32 restatements round the same fp64 sums and agree to the
    # bit: their own difference says nothing about two kernels with different orders of additions)
    for key, k in (("scheme_f32_err", 0), ("hermite_f32_err", 1)):
        ent[key] = {q: norm_err(runs["diff_f32"][k][i][:, :3], runs["diff_f64"][k][i][:, :3]) for i, q in enumerate(("x", "v"))}
        print("all members, %s: x %.3g v %.3g" % (key, ent[key]["x"], ent[key]["v"]))
    out["all_members"] = ent

    # the error ratio per halving of dt
    out["order"] = R.measure_order(out["fixtures"]["plummer256"])
    print("order: err(dt) %.3g err(dt/2) %.3g ratio %.2f" % (out["order"]["err_dt"], out["order"]["err_half"], out["order"]["ratio"]))
    with open(R.JSON_PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
