#!/usr/bin/env python3
"""Measures the record of the tests of the neighbour scheme with radii that follow a target count (tests/ac_adapt_ref.py) ->
tests/golden/ac_adapt.json and the restatement's final states tests/golden/ac_adapt_<case>.npy.  CPU only; the scans use every core
(two minutes on eight).

Cases (ac_adapt_ref.CASES): tracking (target 6, cap 24) and recovery (target 4, cap 8, a start that rebuilds) on the first 256 and all
1,024 rows of plummer1024_* and on disk771_* (one radius per body), 4 regular steps of N_sub = 8.

A radius that moves at every build makes pairs cross the sphere far more often than under fixed radii, so the margin min |d2 / h2 - 1|
of the fixed-radii record (1e-3) cannot be had.  The binary32 cases (n = 256) are chosen by a scan instead: every one of 600 initial
radii is RUN, in fp64 and storing binary32; D is the largest shift of any pair's d2 / h2 (pairs with a ratio in (0.5, 2)) between the
two runs at the build times; the candidate with the largest smallest margin over both runs is taken, and the script asserts that this
margin is >= 32 D and that both runs choose identical rows.  The fp64-only cases (n = 771, 1,024) need no scan: their margin must be
>= 1e-9.  Recorded per case: the stats both structures must reproduce exactly, the margin, D, and the error of the binary32-storing
restatement against the fp64 one.  State files hold (x, v, ai + ar, ji + jr, next, next of the binary32 run): 14 fp64 columns;
ac_adapt_<case>_list.npy holds the final rows.

Also recorded: the cold collapse (plummer256 with velocities zero, radius 0.2, cap 24): K, the first regular step at which fixed radii
overflow; the adaptive run (target 6) to K + 8 with its |dE / E0| in fp64 and storing binary32; adaptive, fixed radii with cap 255 and
plain Hermite at K and deep in the collapse (step 100); and the error ratio per halving of dt with adaptation on (against the scheme at dt / 8).

    python tests/golden/measure_ac_adapt.py
"""
import json
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
for p in (ROOT, os.path.join(ROOT, "nbody3d-webgpu_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ac_adapt_ref as A  # noqa: E402
import ac_ref as R  # noqa: E402
from block_ref import hermite_ref, norm_err  # noqa: E402


def run_pair(ent):
    """A case in fp64 and storing binary32: (o64, o32, (margin over both, margin of the fp64 run), D, identical rows)."""
    b, v, kw = A.case_args(ent)
    m, m32, q64, q32 = [], [], [], []
    o64 = A.ac_adapt_ref(b, v, ent["G"], A.EPS2, ent["dt"], A.STEPS, margins=m, ratios=q64, **kw)
    o32 = A.ac_adapt_ref(b, v, ent["G"], A.EPS2, ent["dt"], A.STEPS, margins=m32, ratios=q32, store=np.float32, **kw)
    same = len(q64) == len(q32) and o64[8] == o32[8] and (o64[6] == o32[6]).all() and (o64[7] == o32[7]).all()
    D = float("inf")
    if len(q64) == len(q32):
        D = 0.0
        for x, y in zip(q64, q32):
            near = (x > 0.5) & (x < 2.0)
            if near.any():
                D = max(D, float(np.abs(x[near] - y[near]).max()))
    return o64, o32, (min(m + m32), min(m)), D, bool(same)


def candidate(arg):
    name, h = arg
    ent = dict(A.CASES[name], radius=h)
    try:
        _, _, (margin, _), D, same = run_pair(ent)
    except A.Overflow:
        return h, 0.0, float("inf"), False
    return h, margin, D, same


def scan(pool, name):
    lo, hi = A.CASES[name]["scan"]
    cands = [(name, float(np.float32(h))) for h in np.geomspace(lo, hi, 600)]
    res = [r for r in pool.map(candidate, cands, chunksize=5) if r[3]]
    assert res, "no candidate for " + name
    h, margin, D, _ = max(res, key=lambda r: r[1])
    print("%s: %d of 600 candidates choose identical rows in both runs; radius %.8g margin %.3g D %.3g (D over the candidates %.3g .. %.3g)"
          % (name, len(res), h, margin, D, min(r[2] for r in res), max(r[2] for r in res)))
    return h


def collapse():
    c = A.COLLAPSE
    b, v = A.fixture(c["fixture"])
    v = np.zeros_like(v)
    counts = []
    try:
        R.ac_ref(b, v, c["G"], A.EPS2, c["dt"], 400, substeps=A.SUBSTEPS, cap=c["cap"], radius=c["radius"], counts=counts)
        raise AssertionError("fixed radii never overflow")
    except R.Overflow:
        K = len(counts) - 1                               # builds = the start + one per regular step
    steps = K + c["extra"]
    e0 = A.energy(b, v, c["G"], A.EPS2)
    de = lambda o: abs(A.energy(o[0], o[1], c["G"], A.EPS2) - e0) / abs(e0)
    out = dict(c, K=K, steps=steps)
    for store, key in ((np.float64, "f64"), (np.float32, "f32")):
        o = A.ac_adapt_ref(b, v, c["G"], A.EPS2, c["dt"], steps, c["target"], cap=c["cap"], radius=c["radius"], store=store)
        out["dE_" + key] = de(o)                              # (no Overflow: every accepted list fits its rows)
        out["stats_" + key] = o[8]
        assert o[8]["overflowed"] == 0 and o[8]["rebuilds"] >= 1
    # the trade the rule makes, where fixed radii with rows of 255 (they hold every close neighbour) and plain Hermite can be run too
    out["dE_at"] = {}
    for k in (K, c["deep"]):
        o = A.ac_adapt_ref(b, v, c["G"], A.EPS2, c["dt"], k, c["target"], cap=c["cap"], radius=c["radius"])
        out["dE_at"][str(k)] = {"adaptive": de(o), "adaptive_rebuilds": o[8]["rebuilds"],
                                "fixed_cap255": de(R.ac_ref(b, v, c["G"], A.EPS2, c["dt"], k, substeps=A.SUBSTEPS, cap=255, radius=c["radius"])),
                                "hermite": de(hermite_ref(b, v, c["G"], A.EPS2, c["dt"], k))}
    print("collapse: fixed radii overflow at regular step %d; adaptive to %d: |dE/E0| f64 %.3g f32 %.3g, %s; the trade: %s"
          % (K, steps, out["dE_f64"], out["dE_f32"], out["stats_f64"], out["dE_at"]))
    return out


def order(ent):
    b, v, kw = A.case_args(ent)
    run = lambda k: A.ac_adapt_ref(b, v, ent["G"], A.EPS2, ent["dt"] / k, A.STEPS * k, **kw)[0][:, :3]
    fine = run(8)
    e1, e2 = norm_err(run(1), fine), norm_err(run(2), fine)
    return {"case": "track256", "err_dt": e1, "err_half": e2, "ratio": e1 / e2}


def main():
    out = {"steps": A.STEPS, "substeps": A.SUBSTEPS, "eps2": A.EPS2, "cases": {}}
    with multiprocessing.Pool() as pool:
        for name, cfg in A.CASES.items():
            ent = {k: v for k, v in cfg.items() if k != "scan"}
            if cfg["f32"]:
                ent["radius"] = scan(pool, name)
            o64, o32, (margin, margin64), D, same = run_pair(ent)
            t64, t32 = A.totals(o64), A.totals(o32, np.float32)
            ent.update(n=len(o64[0]), stats=o64[8], mean_count=float(o64[7].mean()))
            if cfg["f32"]:
                assert same and margin >= 32 * D, (name, margin, D, same)
                ent.update(margin=margin, D=D, f32_err={q: norm_err(t32[i], t64[i]) for i, q in enumerate(A.QUANTITIES)})
            else:
                ent.update(margin=margin64)
                assert ent["margin"] >= 1e-9, (name, ent["margin"])
            assert ent["stats"]["overflowed"] == 0 and (ent["stats"]["rebuilds"] > 0) == name.startswith("recover"), (name, ent["stats"])
            np.save(A.state_path(name), np.concatenate(t64 + (o64[10][:, None], o32[10][:, None]), axis=1))
            np.save(A.list_path(name), o64[6])                  # (an accepted list: the counts are its entries that are not padding)
            out["cases"][name] = ent
            print("%-12s radius %.8g: margin %.3g  mean count %.2f  %s%s" % (name, ent["radius"], ent["margin"], ent["mean_count"], ent["stats"],
                  "  f32 err x %.3g v %.3g a %.3g j %.3g" % tuple(ent["f32_err"][q] for q in A.QUANTITIES) if cfg["f32"] else ""))
    out["collapse"] = collapse()
    out["order"] = order(out["cases"]["track256"])
    print("order: err(dt) %.3g err(dt/2) %.3g ratio %.2f" % (out["order"]["err_dt"], out["order"]["err_half"], out["order"]["ratio"]))
    assert out["order"]["ratio"] >= 12
    with open(A.JSON_PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
