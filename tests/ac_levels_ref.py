"""The fp64 numpy restatement of the neighbour scheme with block individual irregular steps (include/nbody3d_hip.h, "block
individual IRREGULAR steps per body"), built on ac_ref's membership, rows_of, list_sums, split_sums and block_ref's start_levels,
decide.  Imported by test_ac_levels_cpu.py, test_ac_levels_gpu.py and golden/measure_ac_levels.py; not a test module.

`ac_levels_ref` follows the header's numbered steps.  The regular time is ac_ref's, expression for expression, and so are the
predictor and the corrector: with every level frozen at L the result equals ac_ref(substeps = 2^L) bit for bit, frozen at 0
ac_ref(substeps = 1).  Every stored value is rounded once to `store`; everything else is fp64."""
import json
import os

import numpy as np

from ac_ref import GOLDEN, Overflow, _rnd, list_sums, membership, rows_of, split_sums
from block_ref import decide, start_levels

JSON_PATH = os.path.join(GOLDEN, "ac_levels.json")
L_REC, ETA_REC, STEPS_REC = 6, 0.02, 4          # what measure_ac_levels.py records: 2^6 ticks, eta, regular steps
MIN_LEVELS_REC = (0, 2)


def ac_levels_ref(b, v, G, eps2, dt, steps, L=3, cap=128, radius=None, radii=None, store=np.float64, min_level=0, eta=0.02,
                  frozen=False, levels=None, margins=None, dmargins=None, noise=None, per_step=None):
    """`steps` regular steps of dt with 2^L ticks each.  levels: uploaded levels (None: the start rule, or min_level everywhere
    when frozen).  margins: collects the membership margins of the builds (ac_ref's); dmargins: the relative distance of every
    finite tau from the nearest level boundary; noise: (relative size, generator) -- every list sum of a body-step is moved by
    uniform noise of that share of max |a| and max |j|; per_step: a list that gets the levels in front of every regular step.
    Returns (b, v, ai, ji, ar, jr, list, count, levels, stats, level_stats); the two stats as nb_neighbor_scheme_stats and
    nb_neighbor_level_stats."""
    r = _rnd(store)
    b, v = r(np.array(b, np.float64)), r(np.array(v, np.float64))
    n, nsub = len(b), 2 ** L
    h_rad = r(np.full(n, radius, np.float64) if radii is None else np.asarray(radii, np.float64).reshape(-1))
    stats = {"enabled": 1, "regular_steps": 0, "substeps": 0, "entries": 0, "builds": 0, "max_count": 0, "overflowed": 0}
    ls = {"enabled": 1, "regular_steps": 0, "ticks": 0, "block_steps": 0, "body_steps": 0, "entries": 0, "clamped": 0, "finest_level": 0}

    def build():
        inside = membership(b[:, :3], h_rad, store, margins)
        lst, cnt = rows_of(inside, cap)
        stats["builds"] += 1
        stats["entries"] += int(np.minimum(cnt, cap).sum())
        stats["max_count"] = int(cnt.max())
        stats["overflowed"] = int((cnt > cap).sum())
        if stats["overflowed"]:
            raise Overflow("%d rows, largest count %d, cap %d" % (stats["overflowed"], stats["max_count"], cap))
        return [r(z) for z in split_sums(b, v, inside, G, eps2)], lst, cnt

    (ai, ji, ar, jr), lst, cnt = build()
    if levels is not None:
        lev = np.array(levels, np.int64)
    elif frozen:
        lev = np.full(n, min_level, np.int64)
    else:
        lev = start_levels(ai + ar, ji + jr, dt, eta, min_level, L, ls, dmargins)
    ls["finest_level"] = int(lev.max())
    tick = dt / float(nsub)
    for _ in range(steps):
        if per_step is not None:
            per_step.append(lev.astype(np.uint8))
        t = np.zeros(n, np.int64)
        while True:
            s = 2 ** (L - lev)
            t_next = int((t + s).min())
            act = np.nonzero(t + s == t_next)[0]
            # 2. every body from its own stored state at t_i
            tau = (t * tick)[:, None]
            h = ((t_next - t).astype(np.float64) * tick)[:, None]
            a, j = ai + (ar + tau * jr), ji + jr
            bp, vp = b.copy(), v.copy()
            bp[:, :3] = r(b[:, :3] + h * (v[:, :3] + h / 2 * (a + h / 3 * j)))
            vp[:, :3] = r(v[:, :3] + h * (a + h / 2 * j))
            # 3. the list sums of the active rows at the predicted state
            ai1, ji1 = list_sums(bp, vp, lst, cnt, G, eps2)
            ai1, ji1 = ai1[act], ji1[act]
            if noise is not None:
                ai1 = ai1 + noise[0] * np.abs(a).max() * noise[1].uniform(-1, 1, ai1.shape)
                ji1 = ji1 + noise[0] * np.abs(j).max() * noise[1].uniform(-1, 1, ji1.shape)
            ai1, ji1 = r(ai1), r(ji1)
            # 4. the corrector over the body's own step
            hs = (s[act].astype(np.float64) * tick)[:, None]
            tau0 = tau[act]
            tau1 = tau0 + hs
            a0, j0 = a[act], j[act]
            a1, j1 = ai1 + (ar[act] + tau1 * jr[act]), ji1 + jr[act]
            v0 = v[act, :3]
            v1 = v0 + hs / 2 * (a0 + a1) + hs * hs / 12 * (j0 - j1)
            b[act, :3] = r(b[act, :3] + hs / 2 * (v0 + v1) + hs * hs / 12 * (a0 - a1))
            v[act, :3] = r(v1)
            ai[act], ji[act] = ai1, ji1
            # 5. the criterion on the totals; an empty row has tau = inf
            if not frozen:
                d = decide(a0, j0, a1, j1, hs, lev[act], t_next, dt, eta, min_level, L)
                empty = np.minimum(cnt[act], cap) == 0
                after = np.where(empty, np.where(d["aligned"] & (lev[act] > min_level), lev[act] - 1, lev[act]), d["after"])
                clamped = d["clamped"] & ~empty
                ls["clamped"] += int(clamped.sum())
                if dmargins is not None:
                    m = d["margin"][~empty]
                    dmargins.extend(m[np.isfinite(m)])
                lev[act] = after
            t[act] = t_next
            ls["block_steps"] += 1
            ls["body_steps"] += len(act)
            ls["entries"] += int(np.minimum(cnt[act], cap).sum())
            ls["finest_level"] = max(ls["finest_level"], int(lev.max()))
            if t_next == nsub:
                break
        # the regular time: ac_ref's
        aio, jio = [r(z) for z in list_sums(b, v, lst, cnt, G, eps2)]
        try:
            (aip, jip, arp, jrp), lst, cnt = build()
            over = None
        except Overflow as e:
            over = e
            inside = membership(b[:, :3], h_rad, store)
            aip, jip, arp, jrp = [r(z) for z in split_sums(b, v, inside, G, eps2)]
            lst, cnt = rows_of(inside, cap)
        aro, jro = (arp + aip) - aio, (jrp + jip) - jio
        v[:, :3] = r(v[:, :3] + (dt / 2 * (aro - ar) - dt * dt / 12 * (5 * jr + jro)))
        b[:, :3] = r(b[:, :3] + (dt * dt / 6 * (aro - ar) - dt ** 3 / 24 * (3 * jr + jro)))
        ai, ji, ar, jr = aip, jip, arp, jrp
        stats["regular_steps"] += 1
        stats["substeps"] += nsub
        ls["regular_steps"] += 1
        ls["ticks"] += nsub
        if over is not None:
            raise over
    return b, v, ai, ji, ar, jr, lst, cnt, lev.astype(np.uint8), stats, ls


def start_rule(ai, ji, ar, jr, dt, eta, min_level, L):
    """The host rule of the start of the levels on downloaded components ((n, 3) or (n, 4) arrays of any precision)."""
    z = [np.asarray(q, np.float64)[:, :3] for q in (ai, ji, ar, jr)]
    return start_levels(z[0] + z[2], z[1] + z[3], dt, eta, min_level, L, {"clamped": 0}).astype(np.uint8)


def body_steps_of(levels, L):
    """Body-steps of ONE regular step with frozen levels."""
    return int((2 ** np.asarray(levels, np.int64)).sum())


def record():
    with open(JSON_PATH) as f:
        return json.load(f)


def state_path(name, min_level):
    return os.path.join(GOLDEN, "ac_levels_%s_m%d.npy" % (name, min_level))


_cache = {}


def recorded_state(name, min_level):
    """The fp64 restatement's final (x, v, a, j), each (n, 3), of a recorded dynamic run: computed once by measure_ac_levels.py."""
    key = (name, min_level)
    if key not in _cache:
        z = np.load(state_path(name, min_level))
        _cache[key] = tuple(z[:, 3 * q:3 * q + 3] for q in range(4))
    return _cache[key]
