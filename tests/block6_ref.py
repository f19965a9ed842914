"""The numpy restatement of block individual time steps on 6th-order Hermite handles (include/nbody3d_hip.h, nb_set_block_steps6):
block_ref's schedule around hermite6_ref's sums, predictor, corrector and crackle, with the order-6 step criterion.  store =
np.float64: every array and operation binary64; store = np.float32: the binary32-storing mode of hermite6_ref (for frozen levels:
with binary32 storage the criterion is rounding noise).  Also the criterion alone (tau6, derivs45), a decision log with margins
(block_ref's format), the shared systems of the tests and the loader of tests/golden/block6.json.  Imported by
test_block6_cpu.py, test_block6_gpu.py, test_block6_node.py and tests/golden/measure_block6.py; not a test module."""
import json
import os

import numpy as np

import block_ref as B
import hermite6_ref as H6

EPS2 = B.EPS2
JSON_PATH = os.path.join(B.GOLDEN, "block6.json")
FACTOR = 8                        # every tolerance taken from a measured number is this many times the number
NOISE, NOISE_SEEDS = B.NOISE, B.NOISE_SEEDS
QUANTITIES = H6.QUANTITIES


def _norm(x):
    return np.sqrt((x * x).sum(-1))


def pqr(a0, j0, s0, a1, j1, s1, h):
    """The three differences every end-of-step derivative of the quintic is made of (rows of three components, h per row)."""
    P = a1 - a0 - h * j0 - h * h / 2 * s0
    Q = h * (j1 - j0 - h * s0)
    R = h * h * (s1 - s0)
    return P, Q, R


def derivs45(a0, j0, s0, a1, j1, s1, h):
    """(a4, a5): the fourth and fifth derivative of the acceleration's quintic at the END of the step."""
    P, Q, R = pqr(a0, j0, s0, a1, j1, s1, h)
    return (360.0 * P - 192.0 * Q + 36.0 * R) / h ** 4, (720.0 * P - 360.0 * Q + 60.0 * R) / h ** 5


def tau6(a0, j0, s0, a1, j1, s1, c1, h, eta):
    """tau = cbrt(sqrt(eta^3 (|a1| |s1| + |j1|^2) / (|c1| |a5| + |a4|^2))) per row, inf where the denominator is 0; fp64 on the
    values as stored."""
    a0, j0, s0, a1, j1, s1, c1 = [np.asarray(z, np.float64)[:, :3] for z in (a0, j0, s0, a1, j1, s1, c1)]
    h = np.asarray(h, np.float64).reshape(-1, 1)
    a4, a5 = derivs45(a0, j0, s0, a1, j1, s1, h)
    num = eta ** 3 * (_norm(a1) * _norm(s1) + _norm(j1) ** 2)
    den = _norm(c1) * _norm(a5) + _norm(a4) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den == 0, np.inf, np.cbrt(np.sqrt(num / den)))


def decide6(a0, j0, s0, a1, j1, s1, c1, h, level, t_next, dt, eta, lmin, L):
    """block_ref.decide with the order-6 criterion."""
    tau = tau6(a0, j0, s0, a1, j1, s1, c1, h, eta)
    level = np.broadcast_to(np.asarray(level, np.int64), tau.shape)
    want, clamped, margin = B.levels_for(tau, dt, lmin, L)
    aligned = t_next % (2 * 2 ** (L - level)) == 0
    after = np.where(want >= level, want, np.where(aligned, level - 1, level))
    return dict(tau=tau, want=want, after=after, aligned=aligned, clamped=clamped, margin=margin)


def block6_ref(b, v, G, eps2, dt, outer, eta=0.02, max_level=20, min_level=0, levels=None, frozen=False, state=None, margins=None,
               store=np.float64, log=None, noise=None):
    """`outer` outer steps of dt.  levels: initial levels (None: the start rule on (a, j), or min_level everywhere when frozen);
    state: a hermite6_ref state dict carried over (None: hermite6_ref.start, c = 0); store: np.float64, or np.float32 for the
    binary32-storing mode; noise: (relative size, generator) on every (a1, j1, s1) of a block step, as block_ref's.  Returns
    (state, levels, stats): the state a hermite6_ref dict of arrays of dtype `store`."""
    f = store
    d = lambda z: np.asarray(z, np.float64)
    st = H6.start(b, v, G, eps2, f) if state is None else {k: np.array(z, f) for k, z in state.items()}
    n, L = len(st["b"]), max_level
    stats = {"outer_steps": 0, "block_steps": 0, "body_steps": 0, "clamped": 0, "finest_level": 0}
    if levels is None:
        lev = np.full(n, min_level, np.int64) if frozen else B.start_levels(d(st["a"]), d(st["j"]), dt, eta, min_level, L, stats, margins, log)
    else:
        lev = np.array(levels, np.int64)
    stats["finest_level"] = int(lev.max())
    tick = dt / 2.0 ** L
    for _ in range(outer):
        t = np.zeros(n, np.int64)
        while True:
            s = 2 ** (L - lev)
            t_next = int((t + s).min())
            act = np.nonzero(t + s == t_next)[0]
            h = ((t_next - t) * tick)[:, None]
            x, u, a, j, sn, c = d(st["b"][:, :3]), d(st["v"][:, :3]), d(st["a"]), d(st["j"]), d(st["s"]), d(st["c"])
            bp, vp = st["b"].copy(), st["v"].copy()
            bp[:, :3] = (x + h * (u + h / 2 * (a + h / 3 * (j + h / 4 * (sn + h / 5 * c))))).astype(f)
            vp[:, :3] = (u + h * (a + h / 2 * (j + h / 3 * (sn + h / 4 * c)))).astype(f)
            ap = (a + h * (j + h / 2 * (sn + h / 3 * c))).astype(f)
            a1, j1, s1 = H6.fjs(bp, vp, ap, G, eps2, f, rows=act)              # as stored
            if noise is not None:
                a1 = (a1 + noise[0] * np.abs(a).max() * noise[1].uniform(-1, 1, a1.shape)).astype(f)
                j1 = (j1 + noise[0] * np.abs(j).max() * noise[1].uniform(-1, 1, j1.shape)).astype(f)
                s1 = (s1 + noise[0] * np.abs(sn).max() * noise[1].uniform(-1, 1, s1.shape)).astype(f)
            A1, J1, S1 = d(a1), d(j1), d(s1)
            h = (s[act] * tick)[:, None]
            x0, v0, a0, j0, s0 = x[act], u[act], a[act], j[act], sn[act]
            v1 = v0 + h / 2 * (a0 + A1) - h * h / 10 * (J1 - j0) + h ** 3 / 120 * (s0 + S1)
            x1 = x0 + h / 2 * (v0 + v1) - h * h / 10 * (A1 - a0) + h ** 3 / 120 * (j0 + J1)
            c1 = H6.crackle(a0, j0, s0, A1, J1, S1, h).astype(f)
            st["b"][act, :3], st["v"][act, :3] = x1.astype(f), v1.astype(f)
            st["a"][act], st["j"][act], st["s"][act], st["c"][act] = a1, j1, s1, c1
            entry = dict(kind="step", t_next=t_next, act=act, before=lev[act].copy())
            if not frozen:
                dec = decide6(a0, j0, s0, A1, J1, S1, d(c1), h, lev[act], t_next, dt, eta, min_level, L)
                lev[act] = dec["after"]
                stats["clamped"] += int(dec["clamped"].sum())
                if margins is not None:
                    margins.extend(dec["margin"][np.isfinite(dec["margin"])])
                entry.update(dec)
            if log is not None:
                entry.setdefault("after", entry["before"])
                log.append(entry)
            t[act] = t_next
            stats["block_steps"] += 1
            stats["body_steps"] += len(act)
            stats["finest_level"] = max(stats["finest_level"], int(lev.max()))
            if t_next == 2 ** L:
                break
        stats["outer_steps"] += 1
    return st, lev.astype(np.uint8), stats


def energy_of(st, G, eps2):
    return B.energy(st["b"], st["v"], G, eps2)


def decisions(log):
    """(decisions of the block steps, how many of them were clamped)."""
    steps = [e for e in log if e["kind"] == "step" and "clamped" in e]
    return sum(len(e["act"]) for e in steps), sum(int(e["clamped"].sum()) for e in steps)


# ---- the systems the tests share (each restatement computed once, never written) ---------------------------------------------
DT_FROZEN, L_FROZEN = 2.0 ** -4, 3
FROZEN_SIZES = (2, 77, 1025, 4099)
CENSUS = {"257in": (257, True), "257out": (257, False), "4099in": (4099, True), "4099out": (4099, False)}    # (n, heavy bodies inside the level-1 set)
CENSUS_ACTIVE = 64                # bodies 0 .. 63 at level 1, the rest at level 0
# the census's outer step: bodies of mass 1e3 make close orbits (|s| / |a| ~ 1e9 at the softening length), over which a step of
# DT_FROZEN amplifies rounding a thousandfold (binary32-storing distance of the crackle 3e3 at 2^-4, 1.7e-4 at 2^-10, on the
# restatements alone); at 2^-12 the restatement's own binary32 distance x 2^-29 (binary64 / binary32) stays below 1e-13
DT_CENSUS = 2.0 ** -12
_cache = {}


def frozen_levels(n):
    """test_block_gpu.frozen_levels: bodies 1 + 2k, k < 513, at level 2; 40 % of the rest at level 1; the others at level 0; body
    min(5, n - 1) at level 3."""
    lev = np.zeros(n, np.uint8)
    two = np.array([1 + 2 * k for k in range(513) if 1 + 2 * k < n], np.int64)
    lev[two] = 2
    rest = np.setdiff1d(np.arange(n), two)
    rng = np.random.default_rng(7)
    lev[rest[rng.random(len(rest)) < 0.4]] = 1
    lev[min(5, n - 1)] = 3
    return lev


def frozen_system(n):
    from nbody3d_amd import ic
    if n == 2:
        b, v = H6.kepler_pair()
        return b.astype(np.float32), v.astype(np.float32)
    return ic.plummer(n, seed=21)


def frozen_ref(n, store=np.float64):
    """(b0, v0, levels, (state, levels, stats)) of one outer step of DT_FROZEN at max_level L_FROZEN."""
    key = ("frozen", n, store)
    if key not in _cache:
        b0, v0 = frozen_system(n)
        lev = frozen_levels(n)
        _cache[key] = (b0, v0, lev, block6_ref(b0, v0, 1.0, EPS2, DT_FROZEN, 1, max_level=L_FROZEN, levels=lev, frozen=True, store=store))
    return _cache[key]


def census_heavy(n):
    return sorted({256, n - 1})   # the first row of the second tile, and the last row


def census_system(name):
    """A Plummer sphere with a body of mass 1e3 at row 256 and at row n - 1."""
    from nbody3d_amd import ic
    n = CENSUS[name][0]
    b, v = ic.plummer(n, seed=21)
    b = b.copy()
    b[census_heavy(n), 3] = 1e3
    return b, v


def census_levels(name):
    """Bodies 0 .. 63 at level 1, the rest at level 0; "in": the heavy bodies at level 1 as well (gathered i-rows themselves)."""
    n, inside = CENSUS[name]
    lev = np.zeros(n, np.uint8)
    lev[:CENSUS_ACTIVE] = 1
    if inside:
        lev[census_heavy(n)] = 1
    return lev


def census_ref(name, store=np.float64):
    key = ("census", name, store)
    if key not in _cache:
        b0, v0 = census_system(name)
        lev = census_levels(name)
        _cache[key] = (b0, v0, lev, block6_ref(b0, v0, 1.0, EPS2, DT_CENSUS, 1, max_level=1, levels=lev, frozen=True, store=store))
    return _cache[key]


def distances(got, ref, dt, L):
    """hermite6_ref.distances with the crackle's scale taken at the finest step."""
    return H6.distances(got, ref, dt / 2.0 ** L)


TINY = ((6, 9), (12, 15))         # (n, seed) of the exact dynamic cases
TINY_RUN = dict(dt=2.0 ** -3, outer=2, eta=0.02, max_level=12)
PAIR300 = dict(n=300, seed=21, dt=2.0 ** -4, outer=2, eta=0.02, max_level=12)


def tiny_ref(n, seed):
    key = ("tiny", n, seed)
    if key not in _cache:
        from nbody3d_amd import ic
        b0, v0 = B.tight_pair(*ic.plummer(n, seed=seed))
        margins = []
        p = TINY_RUN
        out = block6_ref(b0, v0, 1.0, EPS2, p["dt"], p["outer"], eta=p["eta"], max_level=p["max_level"], margins=margins)
        _cache[key] = (b0, v0, out, min(margins))
    return _cache[key]


def pair300_ref(noise_seed=None, margins=None):
    key = ("pair300", noise_seed)
    if key not in _cache or margins is not None:
        from nbody3d_amd import ic
        p = PAIR300
        b0, v0 = B.tight_pair(*ic.plummer(p["n"], seed=p["seed"]))
        noise = None if noise_seed is None else (NOISE, np.random.default_rng(noise_seed))
        out = block6_ref(b0, v0, 1.0, EPS2, p["dt"], p["outer"], eta=p["eta"], max_level=p["max_level"], noise=noise, margins=margins)
        e0, e1 = B.energy(b0, v0, 1.0, EPS2), energy_of(out[0], 1.0, EPS2)
        _cache[key] = (b0, v0, out, abs((e1 - e0) / e0))
    return _cache[key]


def kepler6_ref(eta=None):
    """(b0, v0, (state, levels, stats), |dE/E|) of block_ref.KEPLER at order 6 (eta: KEPLER's by default)."""
    k = B.KEPLER
    eta = k["eta"] if eta is None else eta
    key = ("kepler", eta)
    if key not in _cache:
        b0, v0 = B.kepler()
        out = block6_ref(b0, v0, k["G"], k["eps2"], k["dt"], k["outer"], eta=eta, max_level=k["max_level"])
        e0, e1 = B.energy(b0, v0, 1.0, k["eps2"]), energy_of(out[0], 1.0, k["eps2"])
        _cache[key] = (b0, v0, out, abs((e1 - e0) / e0))
    return _cache[key]


# ---- what binary32 costs the frozen cases, and what noise moves the 300-body run by (tests/golden/block6.json) ---------------
def measure_all(log=print):
    out = {"generator": "tests/golden/measure_block6.py (tests/block6_ref.py: the binary32-storing restatement against the fp64 one, and the "
                        "fp64 one under noise; numpy, no device)",
           "fixtures": {"eps2": EPS2, "dt_frozen": DT_FROZEN, "max_level_frozen": L_FROZEN, "frozen_sizes": list(FROZEN_SIZES),
                        "census": {k: {"n": c[0], "rows": census_heavy(c[0]), "inside": c[1], "mass": 1e3} for k, c in CENSUS.items()}, "census_active": CENSUS_ACTIVE, "dt_census": DT_CENSUS,
                        "pair300": PAIR300, "noise": NOISE, "noise_seeds": list(NOISE_SEEDS), "factor": FACTOR},
           "frozen": {}, "census": {}}
    for n in FROZEN_SIZES:
        r64, r32 = frozen_ref(n)[3], frozen_ref(n, np.float32)[3]
        assert r64[2] == r32[2]
        out["frozen"][str(n)] = distances(r32[0], r64[0], DT_FROZEN, L_FROZEN)
        log("frozen N=%-5d binary32-storing distance: %s; %s" % (n, "  ".join("%s %.3g" % kv for kv in out["frozen"][str(n)].items()), r64[2]))
    for name in CENSUS:
        r64, r32 = census_ref(name)[3], census_ref(name, np.float32)[3]
        out["census"][name] = distances(r32[0], r64[0], DT_CENSUS, 1)
        log("census %-8s binary32-storing distance: %s" % (name, "  ".join("%s %.3g" % kv for kv in out["census"][name].items())))
    margins = []
    b0, v0, (st, lev, stats), de = pair300_ref(margins=margins)
    dev, flipped = 0.0, 0
    for seed in NOISE_SEEDS:
        nst, nlev, _ = pair300_ref(seed)[2]
        dev = max(dev, B.norm_err(nst["b"][:, :3], st["b"][:, :3]))
        flipped += int((nlev != lev).sum())
    out["pair300"] = {"stats": stats, "dE": float(de), "min_margin": float(min(margins)), "noise_position_dev": dev, "noise_flipped": flipped,
                      "levels": np.bincount(lev, minlength=PAIR300["max_level"] + 1).tolist()}
    log("pair300: %s" % out["pair300"])
    return out


_record = {}


def record():
    if not _record:
        with open(JSON_PATH) as fh:
            _record.update(json.load(fh))
    return _record
