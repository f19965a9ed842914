"""The fp64 numpy restatement of the neighbour scheme with radii that follow a target count (include/nbody3d_hip.h, "the neighbour
scheme on a long run"), and what its tests share.  Imported by test_ac_adapt_cpu.py, test_ac_adapt_gpu.py and
golden/measure_ac_adapt.py; not a test module.

`ac_adapt_ref` is `ac_ref.ac_ref` with the header's build loop (the pass, the shrink of the overflowed rows, the pass again) and the
rule applied after every accepted pass; membership, rows and sums are ac_ref's own functions.  The radii are stored values: rounded
once to `store` wherever the header says so, everything else fp64 (np.cbrt)."""
import json
import os

import numpy as np

from ac_ref import EPS2, GOLDEN, NONE, Overflow, _rnd, fixture, list_sums, membership, radius_args, rows_of, split_sums  # noqa: F401
from block_ref import norm_err  # noqa: F401

JSON_PATH = os.path.join(GOLDEN, "ac_adapt.json")
DT = 1.0 / 64
STEPS = 4
SUBSTEPS = 8
QUANTITIES = ("x", "v", "a", "j")
GROW_DEFAULT = float(np.cbrt(2.0))


# What measure_ac_adapt.py runs.  Tracking: target 6 in rows of 24, started near the radius the rule settles at.  Recovery: target 4 in
# rows of 8, started so large that the start itself rebuilds.  scan: the range of initial radii the binary32 cases are chosen from
# (their margin must carry a binary32 run); the fp64-only cases (f32 False) take `radius` as it stands (disk771: the base of its
# per-body radii, ac_ref.radii_pattern).
CASES = {"track256": dict(fixture="plummer256", G=1.0, dt=DT, target=6, cap=24, per_body=False, f32=True, scan=(0.13, 0.19)),
         "recover256": dict(fixture="plummer256", G=1.0, dt=DT, target=4, cap=8, per_body=False, f32=True, scan=(0.6, 0.8)),
         "track1024": dict(fixture="plummer1024", G=1.0, dt=DT, target=6, cap=24, per_body=False, f32=False, radius=0.098),
         "recover1024": dict(fixture="plummer1024", G=1.0, dt=DT, target=4, cap=8, per_body=False, f32=False, radius=0.43),
         "track771": dict(fixture="disk771", G=1e-4, dt=1.0 / 256, target=6, cap=24, per_body=True, f32=False, radius=0.06),
         "recover771": dict(fixture="disk771", G=1e-4, dt=1.0 / 256, target=4, cap=8, per_body=True, f32=False, radius=0.25)}
COLLAPSE = dict(fixture="plummer256", G=1.0, dt=DT, radius=0.2, cap=24, target=6, extra=8, deep=100)      # velocities zero


def case_args(ent):
    """(bodies0, vel0, the keywords of ac_adapt_ref) of a case of the record (or of CASES with a radius filled in)."""
    b, v = fixture(ent["fixture"])
    kw = dict(target=ent["target"], cap=ent["cap"], substeps=SUBSTEPS)
    kw.update(radius_args(len(b), ent["per_body"], ent["radius"]))
    return b, v, kw


def shrink(h, cnt, cap, target, store=np.float64):
    """The rows with count > cap alone: h <- rnd(h cbrt(n_t / c))."""
    over = cnt > cap
    out = h.copy()
    out[over] = _rnd(store)(h[over] * np.cbrt(float(target) / cnt[over].astype(np.float64)))
    return out


def rule(h, cnt, target, grow_max=GROW_DEFAULT, radius_min=0.0, radius_max=0.0, store=np.float64):
    """next from the radii of an accepted pass and its counts: steps 1-6 of the header."""
    f = np.cbrt((target + 0.5) / (cnt.astype(np.float64) + 0.5))
    f = np.minimum(np.maximum(f, 1.0 / grow_max), grow_max)
    hn = h * f
    if radius_min > 0.0:
        hn = np.maximum(hn, radius_min)
    if radius_max > 0.0:
        hn = np.minimum(hn, radius_max)
    return np.where(h == 0.0, 0.0, _rnd(store)(hn))


def ratios_of(x, h, store):
    """(n, n) d2 / h2 with membership's own roundings (inf on the diagonal and where h = 0): how far every pair is from the sphere."""
    r = _rnd(store)
    d = r(x[None, :, :] - x[:, None, :])
    d2 = r(d[:, :, 0] * d[:, :, 0])
    d2 = r(d[:, :, 1] * d[:, :, 1] + d2)
    d2 = r(d[:, :, 2] * d[:, :, 2] + d2)
    h2 = r(h * h)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(h2 > 0, d2 / np.where(h2 > 0, h2, 1.0), np.inf)
    np.fill_diagonal(q, np.inf)
    return q


def ac_adapt_ref(b, v, G, eps2, dt, steps, target, substeps=SUBSTEPS, cap=24, radius=None, radii=None, grow_max=None, max_rebuilds=None,
                 radius_min=0.0, radius_max=0.0, store=np.float64, margins=None, counts=None, ratios=None):
    """`steps` regular steps of dt with adaptation on.  Returns (b, v, ai, ji, ar, jr, list, count, stats, built, next); stats holds
    the fields of nb_neighbor_scheme_stats and of nb_neighbor_adapt_stats.  Rows still over cap after the last allowed rebuild raise
    Overflow, at the start before anything moved, at a regular time after the state there is completed (ac_ref's policy).  margins,
    counts and ratios collect, per pass, the smallest |d2 / h2 - 1|, the largest count and ratios_of."""
    r = _rnd(store)
    g = GROW_DEFAULT if not grow_max else float(grow_max)
    maxreb = 4 if not max_rebuilds else int(max_rebuilds)
    b, v = r(np.array(b, np.float64)), r(np.array(v, np.float64))
    n = len(b)
    nxt = r(np.full(n, radius, np.float64) if radii is None else np.asarray(radii, np.float64).reshape(-1))
    built = nxt.copy()
    stats = {"enabled": 1, "regular_steps": 0, "substeps": 0, "entries": 0, "builds": 0, "max_count": 0, "overflowed": 0,
             "rebuilds": 0, "rows_shrunk": 0, "last_rebuilds": 0}

    def build(h):
        """The build loop on the state as it stands: (sums, list, count, the radii used, whether rows are still over)."""
        reb = 0
        while True:
            inside = membership(b[:, :3], h, store, margins)
            if ratios is not None:
                ratios.append(ratios_of(b[:, :3], h, store))
            lst, cnt = rows_of(inside, cap)
            stats["builds"] += 1
            stats["entries"] += int(np.minimum(cnt, cap).sum())
            stats["max_count"] = int(cnt.max())
            stats["overflowed"] = int((cnt > cap).sum())
            if counts is not None:
                counts.append(int(cnt.max()))
            if not stats["overflowed"] or reb == maxreb:
                break
            h = shrink(h, cnt, cap, target, store)
            reb += 1
            stats["rows_shrunk"] += stats["overflowed"]
        stats["rebuilds"] += reb
        stats["last_rebuilds"] = reb
        over = None
        if stats["overflowed"]:
            over = Overflow("%d rows, largest count %d, cap %d" % (stats["overflowed"], stats["max_count"], cap))
        return [r(z) for z in split_sums(b, v, inside, G, eps2)], lst, cnt, h, over

    (ai, ji, ar, jr), lst, cnt, used, over = build(nxt)
    if over is not None:
        raise over
    built, nxt = used, rule(used, cnt, target, g, radius_min, radius_max, store)
    hs = dt / substeps
    for _ in range(steps):
        for s in range(substeps):
            tau = s * hs
            a, j = ai + (ar + tau * jr), ji + jr
            bp, vp = b.copy(), v.copy()
            bp[:, :3] = r(b[:, :3] + hs * (v[:, :3] + hs / 2 * (a + hs / 3 * j)))
            vp[:, :3] = r(v[:, :3] + hs * (a + hs / 2 * j))
            ai1, ji1 = [r(z) for z in list_sums(bp, vp, lst, cnt, G, eps2)]
            a1, j1 = ai1 + (ar + (tau + hs) * jr), ji1 + jr
            v1 = v[:, :3] + hs / 2 * (a + a1) + hs * hs / 12 * (j - j1)
            b[:, :3] = r(b[:, :3] + hs / 2 * (v[:, :3] + v1) + hs * hs / 12 * (a - a1))
            v[:, :3] = r(v1)
            ai, ji = ai1, ji1
        aio, jio = [r(z) for z in list_sums(b, v, lst, cnt, G, eps2)]
        (aip, jip, arp, jrp), lst, cnt, used, over = build(nxt)            # accepted in front of the correction, which moves x and v
        aro, jro = (arp + aip) - aio, (jrp + jip) - jio
        v[:, :3] = r(v[:, :3] + (dt / 2 * (aro - ar) - dt * dt / 12 * (5 * jr + jro)))
        b[:, :3] = r(b[:, :3] + (dt * dt / 6 * (aro - ar) - dt ** 3 / 24 * (3 * jr + jro)))
        ai, ji, ar, jr = aip, jip, arp, jrp
        built, nxt = used, rule(used, cnt, target, g, radius_min, radius_max, store)
        stats["regular_steps"] += 1
        stats["substeps"] += substeps
        if over is not None:
            raise over
    return b, v, ai, ji, ar, jr, lst, cnt, stats, built, nxt


def totals(out, store=np.float64):
    """(x, v, ai + ar, ji + jr) of a result: what nb_download and nb_download_jerk return."""
    r = _rnd(store)
    return out[0][:, :3], out[1][:, :3], r(out[2] + out[4]), r(out[3] + out[5])


def energy(b, v, G, eps2):
    """Kinetic + softened potential energy of a state (n, 4), fp64."""
    x, m = np.asarray(b, np.float64)[:, :3], np.asarray(b, np.float64)[:, 3]
    d = x[None, :, :] - x[:, None, :]
    rho = np.sqrt((d * d).sum(2) + eps2)
    w = m[:, None] * m[None, :] / rho
    np.fill_diagonal(w, 0.0)
    return 0.5 * float((m * (np.asarray(v, np.float64)[:, :3] ** 2).sum(1)).sum()) - 0.5 * G * float(w.sum())


def record():
    with open(JSON_PATH) as f:
        return json.load(f)


def state_path(case):
    return os.path.join(GOLDEN, "ac_adapt_%s.npy" % case)


def list_path(case):
    return os.path.join(GOLDEN, "ac_adapt_%s_list.npy" % case)


_cache = {}


def recorded_state(case):
    """The fp64 restatement's final (x, v, a, j, next, next of the binary32-storing run, list, count): computed once by
    measure_ac_adapt.py."""
    if case not in _cache:
        z, lst = np.load(state_path(case)), np.load(list_path(case))
        _cache[case] = tuple(z[:, 3 * q:3 * q + 3] for q in range(4)) + (z[:, 12], z[:, 13], lst, (lst != NONE).sum(1).astype(np.uint32))
    return _cache[case]
