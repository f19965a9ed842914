"""The fp64 numpy restatement of the Ahmad-Cohen neighbour scheme with two shared step levels (include/nbody3d_hip.h, "Ahmad-Cohen
neighbour scheme"), and the fixtures the scheme's tests share.  Imported by test_ac_scheme_cpu.py, test_ac_scheme_gpu.py,
test_ac_scheme_node.py and golden/measure_ac_scheme.py; not a test module.

`ac_ref` follows the header's numbered steps.  Membership is decided in the handle's precision (`store`) with the header's
expression; the list sums are taken over the rows of the list, the split sums over all rows of the bodies by membership.  Every
stored value (x, v, the predicted pair, ai, ji, ar0, jr0) is rounded once to `store`; everything else is fp64.  At every build it
collects the smallest |d2 / h2 - 1| over all pairs (the margin: how far the nearest pair is from changing sides) and the counts."""
import json
import os

import numpy as np

from block_ref import EPS2, hermite_ref, norm_err  # noqa: F401

NONE = 0xFFFFFFFF
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
JSON_PATH = os.path.join(GOLDEN, "ac_scheme.json")
DT = 1.0 / 64
STEPS = 4
SUBSTEPS = (1, 2, 8)
QUANTITIES = ("x", "v", "a", "j")


def _rnd(store):
    return lambda z: np.asarray(z, store).astype(np.float64)


def membership(x, h, store, margins=None):
    """(n, n) bool: d2 = fma(dz, dz, fma(dy, dy, dx dx)) < h h, strictly, in `store` precision, the own row left out.  x (n, 3)
    holds stored values; h (n,) likewise.  margins collects min |d2 / h2 - 1| over the pairs with h > 0."""
    r = _rnd(store)
    d = r(x[None, :, :] - x[:, None, :])
    d2 = r(d[:, :, 0] * d[:, :, 0])                 # (a binary32 product is exact in fp64: these roundings are the fma's)
    d2 = r(d[:, :, 1] * d[:, :, 1] + d2)
    d2 = r(d[:, :, 2] * d[:, :, 2] + d2)
    h2 = r(h * h)[:, None]
    inside = d2 < h2
    np.fill_diagonal(inside, False)
    if margins is not None:
        off = ~np.eye(len(x), dtype=bool) & (h2 > 0)
        if off.any():
            with np.errstate(divide="ignore", invalid="ignore"):
                margins.append(float(np.abs(d2 / np.where(h2 > 0, h2, 1.0) - 1.0)[off].min()))
    return inside


def rows_of(inside, cap):
    """(list (n, cap) uint32 padded with 0xffffffff, count (n,) uint32): ascending j, the cap smallest when there are more."""
    n = len(inside)
    lst = np.full((n, cap), NONE, np.uint32)
    rank = np.cumsum(inside, axis=1) - 1
    k, j = np.nonzero(inside & (rank < cap))
    lst[k, rank[k, j]] = j
    return lst, inside.sum(1).astype(np.uint32)


def _terms(x, u, m, xi, ui, G, eps2, w):
    """Force and jerk at (xi, ui) (k, 3) from candidate rows x, u (k, c, 3) with masses m (k, c) and weights w (k, c)."""
    dr, dv = x - xi[:, None, :], u - ui[:, None, :]
    y2 = 1.0 / ((dr * dr).sum(2) + eps2)
    s3 = w * m * y2 * np.sqrt(y2)
    q = (dr * dv).sum(2) * y2
    return G * (s3[:, :, None] * dr).sum(1), G * (s3[:, :, None] * (dv - 3.0 * q[:, :, None] * dr)).sum(1)


def list_sums(b, v, lst, count, G, eps2):
    """nb_list_force at the bodies, accel and jerk, in fp64: the sums over the first min(count, cap) entries of every row."""
    n, cap = lst.shape
    ln = np.minimum(count, cap)
    width = int(ln.max()) if n else 0
    if width == 0:
        return np.zeros((n, 3)), np.zeros((n, 3))
    idx = lst[:, :width].astype(np.int64)
    ok = (np.arange(width)[None, :] < ln[:, None]) & (idx < n) & (idx != np.arange(n)[:, None])
    idx = np.where(ok, idx, 0)
    return _terms(b[idx, :3], v[idx, :3], b[idx, 3], b[:, :3], v[:, :3], G, eps2, ok.astype(np.float64))


def split_sums(b, v, inside, G, eps2):
    """nb_split_force at the bodies in fp64: (ai, ji, ar, jr), every pair's term in exactly one of the two sums."""
    n = len(b)
    out = [np.zeros((n, 3)) for _ in range(4)]
    for s in range(0, n, 256):
        e = min(n, s + 256)
        x, u, m = b[None, :, :3], v[None, :, :3], np.broadcast_to(b[None, :, 3], (e - s, n))
        w = inside[s:e].astype(np.float64)
        out[0][s:e], out[1][s:e] = _terms(x, u, m, b[s:e, :3], v[s:e, :3], G, eps2, w)
        w = 1.0 - w
        w[np.arange(e - s), np.arange(s, e)] = 0.0
        out[2][s:e], out[3][s:e] = _terms(x, u, m, b[s:e, :3], v[s:e, :3], G, eps2, w)
    return out


class Overflow(Exception):
    pass


def ac_ref(b, v, G, eps2, dt, steps, substeps=8, cap=128, radius=None, radii=None, store=np.float64, margins=None, counts=None):
    """`steps` regular steps of dt.  Returns (b, v, ai, ji, ar, jr, list, count, stats); stats as nb_neighbor_scheme_stats.  A build
    with a count > cap raises Overflow (the header's policy is an error return)."""
    r = _rnd(store)
    b, v = r(np.array(b, np.float64)), r(np.array(v, np.float64))
    n = len(b)
    h = r(np.full(n, radius, np.float64) if radii is None else np.asarray(radii, np.float64).reshape(-1))
    stats = {"enabled": 1, "regular_steps": 0, "substeps": 0, "entries": 0, "builds": 0, "max_count": 0, "overflowed": 0}

    def build():
        inside = membership(b[:, :3], h, store, margins)
        lst, cnt = rows_of(inside, cap)
        stats["builds"] += 1
        stats["entries"] += int(np.minimum(cnt, cap).sum())
        stats["max_count"] = int(cnt.max())
        stats["overflowed"] = int((cnt > cap).sum())
        if counts is not None:
            counts.append(int(cnt.max()))
        if stats["overflowed"]:
            raise Overflow("%d rows, largest count %d, cap %d" % (stats["overflowed"], stats["max_count"], cap))
        return [r(z) for z in split_sums(b, v, inside, G, eps2)], lst, cnt

    (ai, ji, ar, jr), lst, cnt = build()
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
        try:
            (aip, jip, arp, jrp), lst, cnt = build()
            over = None
        except Overflow as e:      # the state at this regular time is still completed below
            over = e
            inside = membership(b[:, :3], h, store)
            aip, jip, arp, jrp = [r(z) for z in split_sums(b, v, inside, G, eps2)]
            lst, cnt = rows_of(inside, cap)
        aro, jro = (arp + aip) - aio, (jrp + jip) - jio
        v[:, :3] = r(v[:, :3] + (dt / 2 * (aro - ar) - dt * dt / 12 * (5 * jr + jro)))
        b[:, :3] = r(b[:, :3] + (dt * dt / 6 * (aro - ar) - dt ** 3 / 24 * (3 * jr + jro)))
        ai, ji, ar, jr = aip, jip, arp, jrp
        stats["regular_steps"] += 1
        stats["substeps"] += substeps
        if over is not None:
            raise over
    return b, v, ai, ji, ar, jr, lst, cnt, stats


def totals(out, store=np.float64):
    """(x, v, ai + ar, ji + jr) of an ac_ref result: what nb_download and nb_download_jerk return."""
    r = _rnd(store)
    return out[0][:, :3], out[1][:, :3], r(out[2] + out[4]), r(out[3] + out[5])


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
def _load(name):
    b = np.fromfile(os.path.join(GOLDEN, name + "_bodies0.f32"), "<f4").reshape(-1, 4)
    v = np.fromfile(os.path.join(GOLDEN, name + "_vel0.f32"), "<f4").reshape(-1, 4)
    return b, v


def fixture(name):
    """(bodies0, vel0) float32 of a fixture of the record: plummer256 (the first 256 rows of plummer1024), plummer1024, disk771."""
    if name == "plummer256":
        b, v = _load("plummer1024")
        return b[:256].copy(), v[:256].copy()
    return _load(name)


FIXTURES = ("plummer256", "plummer1024", "disk771")
# what measure_ac_scheme.py runs per fixture: scan = the range of candidate radii (disk771: of the base of its per-body radii)
SETUP = {"plummer256": dict(G=1.0, dt=DT, cap=24, per_body=False, scan=(0.03, 0.2)),
         "plummer1024": dict(G=1.0, dt=DT, cap=24, per_body=False, scan=(0.02, 0.12)),
         "disk771": dict(G=1e-4, dt=1.0 / 256, cap=24, per_body=True, scan=(0.03, 0.2))}
ALL_MEMBERS = dict(n=77, G=1.0, dt=DT, substeps=4, cap=128, radius=100.0)


def radii_pattern(n):
    """The factors of a per-body radius: (1, 1.25, 0.75, 0) by index mod 4 -- a quarter of the rows has no neighbour sphere."""
    return np.array([1.0, 1.25, 0.75, 0.0])[np.arange(n) % 4]


def radius_args(n, per_body, h):
    """The radius / radii keywords of ac_ref and of Simulation.set_neighbor_scheme for a fixture of the record."""
    return {"radii": (radii_pattern(n) * h).astype(np.float32)} if per_body else {"radius": h}


def measure_order(ent, name="plummer256", substeps=8):
    """The restatement's error ratio per halving of dt, over the same time span, against the scheme at dt / 8."""
    b, v = fixture(name)
    kw = radius_args(len(b), ent["per_body"], ent["radius"])
    run = lambda k: ac_ref(b, v, ent["G"], EPS2, ent["dt"] / k, STEPS * k, substeps=substeps, cap=ent["cap"], **kw)[0][:, :3]
    fine = run(8)
    e1, e2 = norm_err(run(1), fine), norm_err(run(2), fine)
    return {"fixture": name, "substeps": substeps, "err_dt": e1, "err_half": e2, "ratio": e1 / e2}


def record():
    with open(JSON_PATH) as f:
        return json.load(f)


def state_path(name, substeps):
    return os.path.join(GOLDEN, "ac_scheme_%s_s%d.npy" % (name, substeps))


_cache = {}


def recorded_state(name, substeps):
    """The fp64 restatement's final (x, v, a, j), each (n, 3), after STEPS regular steps: computed once by measure_ac_scheme.py."""
    key = (name, substeps)
    if key not in _cache:
        z = np.load(state_path(name, substeps))
        _cache[key] = tuple(z[:, 3 * q:3 * q + 3] for q in range(4))
    return _cache[key]
