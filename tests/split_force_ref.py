"""Reference for nb_split_force (regular and irregular force+jerk in one pass).  Host only (numpy).

`split_ref`: the fp64 direct sums over ALL rows of the bodies, every pair's term added to one of two sums by membership (d2 < h^2,
strictly), membership decided in fp64 on the stored rows.  As list_force_ref.radius_rows it refuses an input with a pair within 1e-6
(relative) of its radius: binary32 then decides every membership as fp64 does.  `split_f32`: the binary32 restatement of the
kernel's pair arithmetic (plain d2, rho^2 = d2 + eps2, the pair of census_ref._f32_terms, an ordered ascending sum per side) from
which tests/golden/measure_split_force.py measures the tolerances.  `row_err`: the census row metric, separately for each of the
four outputs: err_k = |got_k - ref_k|_2 / sum |term|_2 over the terms of THAT sum; a sum without a term must be exactly 0."""
import json
import os

import numpy as np

from census_ref import EPS2, G, SPACING, TOL_FACTOR, TOL_F64, _ordered_sum, bodies, points, row_err, velocities  # noqa: F401
from list_force_ref import point_velocities

OUTPUTS = ("accel_irr", "accel_reg", "jerk_irr", "jerk_reg")
SIZES = (77, 1025, 4099)
SPACINGS = (1.6, 2.4)              # the radii, in lattice spacings
SEED = 5
POINTS = 300
NEAR = 8                           # boundary pairs per side and row
JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_force_census.json")


def _targets(b, vel, first, m, pts, pvel):
    """(positions (m, 3), velocities (m, 3) | None, own (m,) -- -1 at points) in fp64 of the stored rows."""
    if pts is None:
        own = np.arange(first, first + m)
        return np.asarray(b, np.float64)[own, :3], None if vel is None else np.asarray(vel, np.float64)[own, :3], own
    return np.asarray(pts, np.float64)[:, :3], None if pvel is None else np.asarray(pvel, np.float64)[:, :3], np.full(len(pts), -1)


def radii_of(radius, radii, m, dtype):
    """(m,) float64: the per-point radius as the handle stores it (rounded to its precision)."""
    h = np.full(m, radius, np.float64) if radii is None else np.asarray(radii, np.float64).reshape(-1)
    return h.astype(dtype).astype(np.float64)


def membership(b, xt, h, strict=True):
    """(m, n) bool: d2 < h^2 in fp64 on the stored rows.  strict: no pair within 1e-6 (relative) of its radius."""
    x = np.asarray(b, np.float64)[:, :3]
    d = x[None, :, :] - xt[:, None, :]
    d2 = (d * d).sum(2)
    h2 = (h * h)[:, None]
    if strict and d2.size:
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(h2 > 0, np.abs(d2 / np.where(h2 > 0, h2, 1.0) - 1.0), np.inf)
        assert rel.min() > 1e-6, "a pair too close to the radius for an exact comparison"
    return d2 < h2


def split_ref(b, vel=None, radius=None, radii=None, G=G, eps2=EPS2, first=0, m=None, pts=None, pvel=None, dtype=np.float32,
              member=None, strict=True, terms=True):
    """fp64 sums.  b (n, 4), vel (n, >= 3) | None (no jerk then); the points are the bodies first .. first + m (m defaults to n) or
    pts (m, >= 3) with velocities pvel.  `member` (m, n) bool overrides the membership (the exact-boundary test passes int64
    arithmetic's).  Returns a dict: per output name its (m, 3) float64 sum and name + "_scale" (m,) = sum |term|_2; "member"; "tn" /
    "tjn" (m, n): the norms of every pair's terms (the own pair: 0) -- terms=False leaves these three (m, n) arrays out."""
    bq = np.asarray(b, np.float64)
    n = len(bq)
    m = (n - first if m is None else m) if pts is None else len(pts)
    xt, ut, own = _targets(bq, vel, first, m, pts, pvel)
    h = radii_of(radius, radii, m, dtype) if member is None else None
    out = {}
    mem = np.zeros((m, n), bool) if terms else None
    tn_all = np.zeros((m, n)) if terms else None
    tjn_all = np.zeros((m, n)) if terms and ut is not None else None
    for name in OUTPUTS[:4 if ut is not None else 2]:
        out[name], out[name + "_scale"] = np.zeros((m, 3)), np.zeros(m)
    uq = None if ut is None else np.asarray(vel, np.float64)[:, :3]
    step = max(1, 1500000 // max(1, n))
    for k0 in range(0, m, step):
        sl = slice(k0, min(m, k0 + step))
        mk = membership(bq, xt[sl], h[sl], strict) if member is None else np.asarray(member, bool)[sl]
        if terms:
            mem[sl] = mk
        dr = bq[None, :, :3] - xt[sl, None, :]
        y2 = 1.0 / ((dr * dr).sum(2) + eps2)
        y = np.sqrt(y2)
        s3 = G * bq[None, :, 3] * y2 * y
        t = s3[:, :, None] * dr
        tn = np.sqrt((t * t).sum(2))
        if terms:
            tn_all[sl] = tn
        for name, w in (("accel_irr", mk), ("accel_reg", ~mk)):
            out[name][sl], out[name + "_scale"][sl] = (t * w[:, :, None]).sum(1), (tn * w).sum(1)
        if ut is not None:
            dv = uq[None, :, :] - ut[sl, None, :]
            rv = (dr * dv).sum(2) * y2
            tj = s3[:, :, None] * (dv - 3.0 * rv[:, :, None] * dr)
            tjn = np.sqrt((tj * tj).sum(2))
            if terms:
                tjn_all[sl] = tjn
            for name, w in (("jerk_irr", mk), ("jerk_reg", ~mk)):
                out[name][sl], out[name + "_scale"][sl] = (tj * w[:, :, None]).sum(1), (tjn * w).sum(1)
    out["member"], out["tn"], out["tjn"], out["own"] = mem, tn_all, tjn_all, own
    return out


def split_f32(b, vel=None, G=G, eps2=EPS2, first=0, m=None, pts=None, pvel=None, member=None, full=False):
    """The binary32 restatement of nb_split_pk's pair: dr, the plain d2 = dz dz + (dy dy + dx dx), rho^2 = d2 + eps2, rho^-1 = 1 /
    sqrt(rho^2) correctly rounded, G folded into the mass, the weight s3 or 0 per side, each side an ordered ascending binary32 sum
    over all rows.  `member` (m, n) bool: the membership (split_ref's).  Returns {output name: (m, 3) float32}; with full=True also
    "accel_full" / "jerk_full": the one ordered sum over every row (what a full pass holds before anything is subtracted)."""
    f = np.float32
    bq = np.asarray(b, f)
    n = len(bq)
    m = (n - first if m is None else m) if pts is None else len(pts)
    if pts is None:
        own = np.arange(first, first + m)
        xt, ut = bq[own, :3], None if vel is None else np.asarray(vel, f)[own, :3]
    else:
        xt, ut = np.asarray(pts, f)[:, :3], None if pvel is None else np.asarray(pvel, f)[:, :3]
    names = OUTPUTS[:4 if ut is not None else 2]
    out = {name: np.zeros((m, 3), f) for name in names}
    if full:
        out["accel_full"] = np.zeros((m, 3), f)
        if ut is not None:
            out["jerk_full"] = np.zeros((m, 3), f)
    uq = None if ut is None else np.asarray(vel, f)[:, :3]
    step = max(1, 1000000 // max(1, n))
    for k0 in range(0, m, step):
        sl = slice(k0, min(m, k0 + step))
        mk = np.asarray(member, bool)[sl]
        dr = bq[None, :, :3] - xt[sl, None, :]
        d2 = dr[:, :, 2] * dr[:, :, 2] + (dr[:, :, 1] * dr[:, :, 1] + dr[:, :, 0] * dr[:, :, 0])
        y = f(1) / np.sqrt(d2 + f(eps2))
        s3 = (f(G) * bq[None, :, 3]) * (y * y * y)
        si, sr = np.where(mk, s3, f(0)), np.where(mk, f(0), s3)
        out["accel_irr"][sl] = _ordered_sum(si[:, :, None] * dr)
        out["accel_reg"][sl] = _ordered_sum(sr[:, :, None] * dr)
        if full:
            out["accel_full"][sl] = _ordered_sum(s3[:, :, None] * dr)
        if ut is not None:
            dv = uq[None, :, :] - ut[sl, None, :]
            rv = (dr[:, :, 0] * dv[:, :, 0] + dr[:, :, 1] * dv[:, :, 1] + dr[:, :, 2] * dv[:, :, 2]) * (y * y)
            tt = dv - (f(3) * rv)[:, :, None] * dr
            out["jerk_irr"][sl] = _ordered_sum(si[:, :, None] * tt)
            out["jerk_reg"][sl] = _ordered_sum(sr[:, :, None] * tt)
            if full:
                out["jerk_full"][sl] = _ordered_sum(s3[:, :, None] * tt)
    return out


def errors(got, ref):
    """{output name: worst row error} of one result (a dict of (m, >= 3) arrays) on the census metric; a sum without a term must be
    exactly 0 (census_ref.row_err asserts it)."""
    return {name: row_err(np.asarray(got[name])[:, :3], ref[name], ref[name + "_scale"])[1] for name in OUTPUTS if name in got and name in ref}


def boundary_share(b, ref, xt, h, near=NEAR):
    """({output name: the smallest share of its row's scale held by any of the `near` pairs nearest the radius (in d2) on either
    side}, the (m, n) mask of those pairs).  A pair moved to the other sum changes BOTH sums by its term, so each pair is weighed
    against the scale of both sums of its kind; the own pair (term 0 by construction) is no boundary pair."""
    x = np.asarray(b, np.float64)[:, :3]
    m = len(xt)
    d = x[None, :, :] - xt[:, None, :]
    d2 = (d * d).sum(2)
    gap = np.abs(d2 - (h * h)[:, None])
    mem = ref["member"]
    own = ref["own"]
    self_pair = np.arange(len(x))[None, :] == own[:, None]
    pick = np.zeros_like(mem)
    for side in (mem, ~mem):
        g = np.where(side & ~self_pair, gap, np.inf)
        idx = np.argsort(g, axis=1)[:, :near]
        ok = np.take_along_axis(g, idx, 1) < np.inf
        rows = np.repeat(np.arange(m)[:, None], idx.shape[1], 1)
        pick[rows[ok], idx[ok]] = True
    out = {}
    for name in OUTPUTS:
        if name not in ref:
            continue
        t = ref["tn"] if name.startswith("accel") else ref["tjn"]
        scale = ref[name + "_scale"][:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(pick & (scale > 0), t / np.where(scale > 0, scale, 1.0), np.inf)
        out[name] = float(share.min())
    return out, pick


# ---- the census inputs and their measurement ----------------------------------------------------------------------------------------
_cache = {}


def census_input(n, spacings):
    """One input, computed once and shared (read-only): bodies, velocities, POINTS arbitrary points with random velocities and the
    fp64 references at the bodies ("ref") and at the points ("pref")."""
    key = (n, spacings)
    if key not in _cache:
        b, v = bodies(n, SEED), velocities(n, SEED)
        h = spacings * SPACING
        pts, pv = points(n, POINTS, SEED), point_velocities(POINTS, SEED)
        c = {"n": n, "spacings": spacings, "radius": h, "b": b, "v": v, "pts": pts, "pv": pv,
             "ref": split_ref(b, v, radius=h), "pref": split_ref(b, v, radius=h, pts=pts, pvel=pv)}
        for a in (b, v, pts, pv):
            a.setflags(write=False)
        _cache[key] = c
    return _cache[key]


def measure(n, spacings):
    c = census_input(n, spacings)
    e = {"n": n, "spacings": spacings, "radius": c["radius"], "points": POINTS, "factor": TOL_FACTOR,
         "mean_count": float(c["ref"]["member"].sum(1).mean()) - 1.0, "points_mean_count": float(c["pref"]["member"].sum(1).mean())}
    for pre, ref, kw in (("", c["ref"], {}), ("pt_", c["pref"], {"pts": c["pts"], "pvel": c["pv"]})):
        err = errors(split_f32(c["b"], c["v"], member=ref["member"], **kw), ref)
        xt = np.asarray(c["b"] if not pre else c["pts"], np.float64)[:, :3]
        share, _ = boundary_share(c["b"], ref, xt, radii_of(c["radius"], None, len(xt), np.float32))
        for name in OUTPUTS:
            e[pre + name + "_ref_f32_err"], e[pre + name + "_tol"], e[pre + name + "_boundary_share"] = err[name], TOL_FACTOR * err[name], share[name]
    return e


def plummer_radius(b, mean_count):
    """The radius at which the bodies of b have `mean_count` members on average (themselves left out), by bisection in fp64."""
    x = np.asarray(b, np.float64)[:, :3]
    d2 = ((x[None, :, :] - x[:, None, :]) ** 2).sum(2)
    lo, hi = 0.0, float(np.sqrt(d2.max())) + 1.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if (d2 < mid * mid).sum() / len(x) - 1.0 < mean_count:
            lo = mid
        else:
            hi = mid
    return float(np.float32(hi))


def measure_cancellation(n=4096, seed=7, mean_count=32, G=1.0, eps2=EPS2):
    """What the feature buys, on the CPU: the regular acceleration and jerk of ic.plummer(n, seed) at the radius of `mean_count`
    members taken two ways in binary32 -- (full sum) - (irregular sum), and the split restatement's regular sum -- both against fp64,
    on the row metric of the regular sum.  {"accel" | "jerk": {"subtract" | "split": {"worst", "median"}}}."""
    from nbody3d_amd import ic
    b, v = ic.plummer(n, seed=seed)
    b, v = np.asarray(b, np.float32), np.asarray(v, np.float32)
    h = plummer_radius(b, mean_count)
    ref = split_ref(b, v, radius=h, G=G, eps2=eps2, strict=False)
    r32 = split_f32(b, v, G=G, eps2=eps2, member=ref["member"], full=True)
    out = {"n": n, "seed": seed, "radius": h, "mean_count": float(ref["member"].sum(1).mean()) - 1.0, "G": G, "eps2": eps2}
    for kind in ("accel", "jerk"):
        sub = r32[kind + "_full"] - r32[kind + "_irr"]                   # binary32, as a caller of the two passes would take it
        out[kind] = {}
        for how, got in (("subtract", sub), ("split", r32[kind + "_reg"])):
            err = row_err(got, ref[kind + "_reg"], ref[kind + "_reg_scale"])[0]
            out[kind][how] = {"worst": float(err.max()), "median": float(np.median(err))}
    return out


def measure_all():
    return {"generator": "tests/golden/measure_split_force.py (tests/split_force_ref.py: a binary32 restatement, ordered ascending sums, against numpy fp64)",
            "metric": "err_k = |got_k - ref_k|_2 / sum |term|_2 over the terms of that sum, per row and output; tol = factor x ref_f32_err; "
                      "every input keeps boundary_share >= 8 tol",
            "G": G, "eps2": EPS2, "seed": SEED, "tol_f64": TOL_F64, "near": NEAR,
            "inputs": [measure(n, sp) for n in SIZES for sp in SPACINGS],
            "cancellation": measure_cancellation()}


def record():
    with open(JSON_PATH) as f:
        return json.load(f)


def entry(n, spacings):
    return [e for e in record()["inputs"] if e["n"] == n and e["spacings"] == spacings][0]
