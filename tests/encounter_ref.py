"""The CPU restatement of the encounter watch (include/nbody3d_hip.h, nb_set_encounter_watch) on top of tests/block_ref.py's loop,
the integer lattice of the exact census with its O(n^2) int64 brute force, and the inputs the encounter tests share.  Imported by
test_encounter_cpu.py, test_encounter_gpu.py and test_encounter_node.py; not a test module."""
import numpy as np

import block_ref as R

NONE = 0xffffffff


def thresholds(radii, eps2, store):
    """w_i = h_i^2 + eps2 in fp64, rounded once to the handle's type; h_i = 0: 0 (below every rho^2: not watched)."""
    h = np.asarray(radii, np.float64)
    return np.where(h > 0, h * h + eps2, 0.0).astype(store)


def pass_answers(xp, act, w, eps2, store):
    """One gathered pass: for every active body the candidate (j != i by index, rho^2 < w_i, strict) of smallest rho^2, equal rho^2
    to the smallest index.  rho^2 = ((eps2 + dx^2) + dy^2) + dz^2 in the handle's type, the pass's order.  Returns (rho2, partner),
    partner NONE where there is no candidate."""
    x = np.asarray(xp)[:, :3].astype(store)
    e2 = store(eps2)
    rho2, partner = np.full(len(act), np.inf, store), np.full(len(act), NONE, np.uint32)
    cols = np.arange(len(x))
    for s in range(0, len(act), 512):
        r = act[s:s + 512]
        d = x[None, :, :] - x[r, None, :]
        r2 = ((e2 + d[:, :, 0] * d[:, :, 0]) + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        r2 = np.where((r2 < w[r, None]) & (cols[None, :] != r[:, None]), r2, store(np.inf))
        k = r2.argmin(1)                                   # the first of equal values: the smallest index
        best = r2[np.arange(len(r)), k]
        ok = np.isfinite(best)
        rho2[s:s + 512] = best
        partner[s:s + 512] = np.where(ok, k, NONE)
    return rho2, partner


def new_records(n, store):
    return dict(rho2=np.full(n, np.inf, store), partner=np.full(n, NONE, np.uint32), time=np.full(n, np.inf), count=np.zeros(n, np.uint32))


def watch_ref(b, v, G, eps2, dt, outer, radii, store=np.float64, first_outer=0, records=None, fj=None, **kw):
    """block_ref(b, v, G, eps2, dt, outer, store=store, **kw) with the watch on: every block step's pass is observed through the
    direct sum block_ref calls (its predicted rows and its active list), the block times come from its log.  radii: one radius or
    one per body.  first_outer: the outer steps the handle had run before.  records: carried over (None: the start values).
    Returns (block_ref's result, records, stats) -- stats: passes, hits, first_time and per outer step the hits so far."""
    n = len(b)
    w = thresholds(np.broadcast_to(np.asarray(radii, np.float64), (n,)), eps2, store)
    rec = new_records(n, store) if records is None else {k: np.array(a) for k, a in records.items()}
    base = R.fj_ref if fj is None else fj
    seen = []

    def observed(bp, vp, G_, e2, rows=None):
        if rows is not None:
            seen.append((np.array(bp[:, :3]), np.array(rows)))
        return base(bp, vp, G_, e2) if rows is None else base(bp, vp, G_, e2, rows)
    log = kw.pop("log", None)
    log = [] if log is None else log
    mark = len(log)
    out = R.block_ref(b, v, G, eps2, dt, outer, store=store, fj=observed, log=log, **kw)
    steps = [e for e in log[mark:] if e["kind"] == "step"]
    assert len(steps) == len(seen)
    L = kw.get("max_level", 20)
    stats = dict(passes=0, hits=0, first_time=np.inf, hits_after=[])
    k = first_outer
    for (xp, act), e in zip(seen, steps):
        assert np.array_equal(act, e["act"])
        t = k + e["t_next"] / 2.0 ** L
        r2, p = pass_answers(xp, act, w, eps2, store)
        ok = p != NONE
        i = act[ok]
        rec["count"][i] += 1
        better = r2[ok] < rec["rho2"][i]
        rec["rho2"][i[better]], rec["partner"][i[better]], rec["time"][i[better]] = r2[ok][better], p[ok][better], t
        stats["passes"] += 1
        stats["hits"] += int(ok.sum())
        if ok.any():
            stats["first_time"] = min(stats["first_time"], t)
        if e["t_next"] == 2 ** L:
            k += 1
            stats["hits_after"].append(stats["hits"])
    return out, rec, stats


# ---- the integer lattice of the exact census -----------------------------------------------------------------------------------
LATTICE_EPS2, LATTICE_L, LATTICE_DT = 0.25, 3, 2.0 ** -4
LATTICE_CASES = ("one", "per_body", "coincident")


def lattice(n, seed=5):
    """n bodies on distinct random integer sites of [0, 64)^3, then: body 0 at the origin (where the padding rows of the f32 kernels
    sit) with body 1 at (1, 0, 0); three coincident pairs of distinct indices; one coincident pair whose members lie in the first
    and the last 256-row tile (different j-chunks wherever there are two).  v = 0; with G = 0 nothing moves.  Returns (b, v,
    coincident pairs)."""
    rng = np.random.default_rng(seed)
    sites = rng.choice(64 ** 3 - 2, n, replace=False) + 2          # 0 = (0, 0, 0) and 1 = (1, 0, 0) are kept free
    x = np.stack([sites % 64, (sites // 64) % 64, sites // 4096], 1).astype(np.int64)
    x[0], x[1] = (0, 0, 0), (1, 0, 0)
    pairs = [(10, 700), (300, 301), (n - 2, 64), (5, n - 1)]
    for i, j in pairs:
        x[j] = x[i]
    b = np.zeros((n, 4))
    b[:, :3], b[:, 3] = x, 1.0 / n
    return b, np.zeros((n, 4)), pairs


def lattice_levels(n, second=False):
    """l_i = i mod 4; second: every body at level 3 except body 7 at level 0 (|A| = n - 1 seven times, then n)."""
    if not second:
        return (np.arange(n) % 4).astype(np.uint8)
    lev = np.full(n, 3, np.uint8)
    lev[7] = 0
    return lev


def lattice_radii(n, case):
    """one: h = 4 for every body (ties are frequent on the lattice); per_body: a mix with zeros; coincident: so small that only
    the coincident pairs answer.  Every h^2 + eps2 is exact in binary32."""
    if case == "one":
        return np.full(n, 4.0)
    if case == "coincident":
        return np.full(n, 0.5)
    return np.random.default_rng(11).choice([0.0, 1.5, 4.0, 6.0], n)


def lattice_brute(b, lev, radii, L=LATTICE_L, dtype=np.int64):
    """The records after ONE outer step from the start values, nothing moving: O(n^2) in exact integers.  Returns (records, hits,
    passes).  dtype: int64; the large census passes int16 (coordinates below 64: a squared distance is at most 11,907), which the
    same loop runs four times as fast.  An integer d2 is below h^2 exactly when it is below ceil(h^2)."""
    x = np.asarray(b)[:, :3].astype(dtype)
    n = len(x)
    lev = np.asarray(lev, np.int64)
    big = np.iinfo(dtype).max
    thr = np.minimum(np.ceil(np.asarray(radii, np.float64) ** 2), big - 1).astype(dtype)
    assert dtype == np.int64 or 3 * int(x.max() - x.min()) ** 2 < big - 1
    rec = new_records(n, np.float64)
    for s in range(0, n, 512):
        i = np.arange(s, min(s + 512, n))
        d2 = np.zeros((len(i), n), dtype)
        for c in range(3):                                            # (axis by axis: no (rows, n, 3) temporary at the large size)
            d = x[None, :, c] - x[i, None, c]
            d *= d
            d2 += d
        d2[np.arange(len(i)), i] = big                                # self, by index
        d2[d2 >= thr[i, None]] = big                                  # (radius 0: no candidate)
        k = d2.argmin(1)
        best = d2[np.arange(len(i)), k]
        ok = best != big
        rec["rho2"][i[ok]] = best[ok].astype(np.int64) + LATTICE_EPS2
        rec["partner"][i[ok]] = k[ok]
        rec["count"][i[ok]] = 2 ** lev[i[ok]]
        rec["time"][i[ok]] = 2.0 ** -lev[i[ok]]                       # the first own block time
    passes = 2 ** int(lev.max())
    return rec, int(rec["count"].sum()), passes


# The large census: big enough that the full-set pass of an f32 handle runs 1,024-row workgroups (NG = 2) and the fold one lane per
# row; with SMALL_SET bodies one level deeper, the first block step is a small set cut into more than 32 chunks (64 lanes per row).
LARGE_N, SMALL_SET = 32771, 100


def large_levels(n, mixed):
    """Every body at level 0; mixed: SMALL_SET bodies spread over the system at level 1 (|A| = SMALL_SET, then n)."""
    lev = np.zeros(n, np.uint8)
    if mixed:
        lev[np.linspace(3, n - 1, SMALL_SET).astype(np.int64)] = 1
    return lev


def ceil_div(a, b):
    return -(-a // b)


def pass_shape(n, na, f64, cus):
    """The engine's launch shape of a gathered pass of an order-4 handle and of the fold behind it, restated from
    nb_engine.hip (chunk_shape, gathered_shape, block_step): (rows per workgroup, j-chunks, lanes per row of the fold)."""
    want, rows, tiles = 8 * cus, 256 if f64 else 1024, ceil_div(n, 256)
    owned = max(max(min(ceil_div(want, ceil_div(n, rows)), n // 2048), 1), ceil_div(n, 1 << 20))
    owned = ceil_div(n, ceil_div(ceil_div(n, owned), 256) * 256)
    if not f64 and (na <= rows // 2 or ceil_div(na, rows) * tiles < want):
        rows //= 2
    c = min(ceil_div(want, ceil_div(na, rows)), min(owned * n // na, tiles))
    c = max(max(c, 1), ceil_div(n, 1 << 20))
    chunks = ceil_div(n, ceil_div(ceil_div(n, c), 256) * 256)
    lpr = 1
    while lpr < chunks and lpr < 64 and na * lpr * 2 <= 65536:
        lpr *= 2
    return rows, chunks, lpr


# ---- the dynamic runs ----------------------------------------------------------------------------------------------------------
KEPLER = dict(G=1.0, eps2=1e-10, dt=0.4, outer=16, eta=0.02, max_level=20, radius=0.2)      # the second pericentre (t = 2 pi) falls inside outer step 16
PAIR300 = dict(G=1.0, eps2=R.EPS2, dt=2.0 ** -4, outer=2, eta=0.02, max_level=12, radius=0.1)
_cache = {}


PERICENTRE2 = (1.0 - 0.9) ** 2                 # (a (1 - e))^2 of R.kepler()
KEPLER_DISTANCE = 2.3724891e-06               # |recorded rho2 - eps2 - PERICENTRE2| of the restatement below (measured; test_encounter_cpu holds it)


def kepler_watch_ref():
    """The orbit starts AT pericentre, so the watch's first sample sits right behind it: the records are reset after the first
    outer step, and what the remaining 15 record is the second passage, inside outer step 16.  (b0, v0, result, records, stats)."""
    if "kepler" not in _cache:
        b0, v0 = R.kepler()
        k = KEPLER
        run = dict(eta=k["eta"], max_level=k["max_level"])
        o1, _, _ = watch_ref(b0, v0, k["G"], k["eps2"], k["dt"], 1, k["radius"], **run)
        _cache["kepler"] = (b0, v0) + watch_ref(o1[0], o1[1], k["G"], k["eps2"], k["dt"], k["outer"] - 1, k["radius"], first_outer=1,
                                                levels=o1[4], aj=(o1[2], o1[3]), **run)
    return _cache["kepler"]


# NB_ENC_STOP on the N = 300 input: only bodies 96 and 283 are watched; they first come within 0.012 of each other in the third
# outer step of the restatement
STOP = dict(bodies=(96, 283), radius=0.012, outer=6)


def stop_ref():
    if "stop" not in _cache:
        b0, v0 = pair300()
        k = PAIR300
        rad = np.zeros(300)
        rad[list(STOP["bodies"])] = STOP["radius"]
        _cache["stop"] = (b0, v0, rad) + watch_ref(b0, v0, k["G"], k["eps2"], k["dt"], STOP["outer"], rad, eta=k["eta"], max_level=k["max_level"])
    return _cache["stop"]


def pair300():
    from nbody3d_amd import ic
    return R.tight_pair(*ic.plummer(300, seed=21))


def pair300_watch_ref():
    if "pair300" not in _cache:
        b0, v0 = pair300()
        k = PAIR300
        _cache["pair300"] = (b0, v0) + watch_ref(b0, v0, k["G"], k["eps2"], k["dt"], k["outer"], k["radius"], eta=k["eta"], max_level=k["max_level"])
    return _cache["pair300"]
