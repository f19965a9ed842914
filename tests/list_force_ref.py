"""Reference for nb_list_force (acceleration, jerk and potential over neighbour rows).  Host only (numpy).

`list_ref`: the fp64 direct sum over the VALID entries of every row, on the rows as uploaded (binary32- or binary64-rounded), with the
census row metric of tests/census_ref.py: a row is judged on the scale of the terms that make it up,

    err_k = |got_k - ref_k|_2 / sum_e |term_ke|_2      (a and the jerk; phi: relative to |phi_k|, every term has one sign)

and a row without a term must be exactly 0 (census_ref.row_err).  `list_f32`: the binary32 restatement of the same sums (the pair of
census_ref._f32_terms, an ordered ascending sum over the row) from which tests/golden/measure_list_force.py measures the tolerances.
`radius_rows`: the rows nb_neighbor_lists gives for one radius, by numpy, refusing inputs whose membership binary32 could decide
differently."""
import json
import os

import numpy as np

from census_ref import EPS2, G, SPACING, TOL_FACTOR, TOL_F64, _ordered_sum, bodies, lattice, points, row_err, velocities  # noqa: F401

NONE = 0xffffffff
SIZES = (77, 1025, 4099)
SPACINGS = (1.6, 2.4)              # the radii, in lattice spacings
CAP = 128
SEED = 5
POINTS = 300
JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "list_force_census.json")


def point_velocities(m, seed):
    """(m, 4) float32 rows of order 1 for the arbitrary points of an input."""
    v = np.zeros((m, 4), np.float32)
    v[:, :3] = np.random.default_rng(seed + 4000).normal(0.0, 1.0, (m, 3))
    return v


def radius_rows(b, radius, cap, targets=None):
    """(lists (m, cap) uint32 padded with NONE, count (m,) uint32): per body of b (itself left out) -- or per target -- the bodies with
    |x_j - p|^2 < radius^2 in ascending order, computed in fp64 on the stored rows.  No pair may sit within 1e-6 (relative) of the
    radius (binary32 rounds d2 and the squared radius by less than 3e-7): binary32 then decides every membership as fp64 does, and
    the engine's rows must EQUAL these."""
    x = np.asarray(b, np.float64)[:, :3]
    p = x if targets is None else np.asarray(targets, np.float64)[:, :3]
    m = len(p)
    h2 = float(np.float32(radius)) ** 2
    lists = np.full((m, cap), NONE, np.uint32)
    count = np.zeros(m, np.uint32)
    step = max(1, 2000000 // max(1, len(x)))
    for k0 in range(0, m, step):
        d = x[None, :, :] - p[k0:k0 + step, None, :]
        d2 = (d * d).sum(2)
        assert np.abs(d2 / h2 - 1.0).min() > 1e-6, "a pair too close to the radius for an exact comparison"
        inside = d2 < h2
        if targets is None:
            kk = np.arange(k0, min(m, k0 + step))
            inside[kk - k0, kk] = False
        count[k0:k0 + step] = inside.sum(1)
        rank = np.cumsum(inside, axis=1) - 1
        k, j = np.nonzero(inside & (rank < cap))
        lists[k0 + k, rank[k, j]] = j
    return lists, count


def _valid(lists, n, own, count):
    """(index with every invalid entry replaced by 0, mask of the valid entries), cut to the columns anything reads."""
    lists = np.asarray(lists, np.uint32)
    m, cap = lists.shape
    length = np.full(m, cap, np.int64) if count is None else np.minimum(np.asarray(count, np.int64), cap)
    cols = int(length.max()) if m else 0
    lists = lists[:, :cols].astype(np.int64)
    ok = (lists < n) & (np.arange(cols)[None, :] < length[:, None])
    if own is not None:
        ok &= lists != np.asarray(own, np.int64)[:, None]
    return np.where(ok, lists, 0), ok


def _targets(b, vel, first, pts, pvel, m, dtype):
    """(positions (m, 3), velocities (m, 3) | None, own (m,) | None) of the rows' points."""
    if pts is None:
        own = np.arange(first, first + m)
        return np.asarray(b, dtype)[own, :3], None if vel is None else np.asarray(vel, dtype)[own, :3], own
    return np.asarray(pts, dtype)[:, :3], None if pvel is None else np.asarray(pvel, dtype)[:, :3], None


def list_ref(b, vel, lists, G=G, eps2=EPS2, first=0, pts=None, pvel=None, count=None):
    """fp64 sums over the valid entries of each row.  b (n, 4), vel (n, >=3) | None (no jerk then), lists (m, cap); the rows belong to
    the bodies first .. first + m (an entry equal to the own index is no entry) or, with pts (m, >=3), to those points (pvel: their
    velocities).  Returns a dict of float64 arrays a (m, 3), scale (m,), phi (m,), and with velocities j (m, 3), j_scale (m,);
    min_share / j_min_share / phi_min_share: the smallest share one entry has of its row's scale (inf without an entry); terms (m,): valid
    entries per row."""
    bq = np.asarray(b, np.float64)
    m = len(lists)
    xt, ut, own = _targets(bq, vel, first, pts, pvel, m, np.float64)
    idx, ok = _valid(lists, len(bq), own, count)
    out = {"a": np.zeros((m, 3)), "scale": np.zeros(m), "phi": np.zeros(m), "terms": ok.sum(1)}
    if ut is not None:
        uq = np.asarray(vel, np.float64)[:, :3]
        out["j"], out["j_scale"] = np.zeros((m, 3)), np.zeros(m)
    shares = {"min_share": np.inf, "j_min_share": np.inf, "phi_min_share": np.inf}
    step = max(1, 1500000 // max(1, idx.shape[1]))
    for k0 in range(0, m, step):
        sl = slice(k0, k0 + step)
        i, w = idx[sl], ok[sl]
        dr = bq[i, :3] - xt[sl, None, :]
        y2 = 1.0 / ((dr * dr).sum(2) + eps2)
        y = np.sqrt(y2)
        gm = G * bq[i, 3] * w
        t = (gm * y2 * y)[:, :, None] * dr
        tn = np.sqrt((t * t).sum(2))
        p = gm * y
        out["a"][sl], out["scale"][sl], out["phi"][sl] = t.sum(1), tn.sum(1), -p.sum(1)
        parts = [("min_share", tn), ("phi_min_share", p)]
        if ut is not None:
            dv = uq[i] - ut[sl, None, :]
            rv = (dr * dv).sum(2) * y2
            tj = (gm * y2 * y)[:, :, None] * (dv - 3.0 * rv[:, :, None] * dr)
            tjn = np.sqrt((tj * tj).sum(2))
            out["j"][sl], out["j_scale"][sl] = tj.sum(1), tjn.sum(1)
            parts.append(("j_min_share", tjn))
        for name, q in parts:
            with np.errstate(divide="ignore", invalid="ignore"):
                share = np.where(w, q / q.sum(1)[:, None], np.inf)
            if share.size:
                shares[name] = min(shares[name], float(share.min()))
    out.update(shares)
    return out


def naive_ref(b, vel, lists, G=G, eps2=EPS2, first=0, pts=None, pvel=None, count=None):
    """list_ref's a, j and phi by a plain Python loop per entry (for checking list_ref itself at small sizes)."""
    b = np.asarray(b, np.float64)
    n, m = len(b), len(lists)
    a, jk, phi = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros(m)
    for k in range(m):
        p = b[first + k, :3] if pts is None else np.asarray(pts, np.float64)[k, :3]
        u = None
        if vel is not None:
            u = np.asarray(vel, np.float64)[first + k, :3] if pts is None else np.asarray(pvel, np.float64)[k, :3]
        length = len(lists[k]) if count is None else min(int(count[k]), len(lists[k]))
        for e in range(length):
            j = int(lists[k][e])
            if j >= n or (pts is None and j == first + k):
                continue
            dr = b[j, :3] - p
            rho2 = float(dr @ dr) + eps2
            gm = G * b[j, 3]
            a[k] += gm * dr / rho2 ** 1.5
            phi[k] -= gm / rho2 ** 0.5
            if u is not None:
                dv = np.asarray(vel, np.float64)[j, :3] - u
                jk[k] += gm * (dv / rho2 ** 1.5 - 3.0 * float(dr @ dv) * dr / rho2 ** 2.5)
    return a, jk, phi


def list_f32(b, vel, lists, G=G, eps2=EPS2, first=0, pts=None, pvel=None, count=None):
    """The binary32 restatement: the pair of census_ref._f32_terms (rho^-1 = 1 / sqrt(r2) correctly rounded, G folded into the mass),
    each row an ordered ascending binary32 sum over its entries.  Returns (a (m, 3), j (m, 3) | None, phi (m,)) float32."""
    f = np.float32
    bq = np.asarray(b, f)
    m = len(lists)
    xt, ut, own = _targets(bq, vel, first, pts, pvel, m, f)
    idx, ok = _valid(lists, len(bq), own, count)
    a, phi = np.zeros((m, 3), f), np.zeros(m, f)
    jk = np.zeros((m, 3), f) if ut is not None else None
    step = max(1, 1500000 // max(1, idx.shape[1]))
    for k0 in range(0, m, step):
        sl = slice(k0, k0 + step)
        i = idx[sl]
        dr = bq[i, :3] - xt[sl, None, :]
        r2 = dr[:, :, 2] * dr[:, :, 2] + (dr[:, :, 1] * dr[:, :, 1] + (dr[:, :, 0] * dr[:, :, 0] + f(eps2)))
        y = f(1) / np.sqrt(r2)
        w = (f(G) * bq[i, 3]) * ok[sl]
        s3 = w * (y * y * y)
        a[sl] = _ordered_sum(s3[:, :, None] * dr)
        phi[sl] = -_ordered_sum(w * y)
        if ut is not None:
            dv = np.asarray(vel, f)[:, :3][i] - ut[sl, None, :]
            rv = (dr[:, :, 0] * dv[:, :, 0] + dr[:, :, 1] * dv[:, :, 1] + dr[:, :, 2] * dv[:, :, 2]) * (y * y)
            jk[sl] = _ordered_sum(s3[:, :, None] * (dv - (f(3) * rv)[:, :, None] * dr))
    return a, jk, phi


# ---- the census inputs and their measurement ----------------------------------------------------------------------------------------
_cache = {}


def census_input(n, spacings):
    """One input, computed once and shared (read-only): bodies, velocities, the numpy rows at the bodies and at POINTS arbitrary points
    with random velocities, and the fp64 references of both."""
    key = (n, spacings)
    if key not in _cache:
        b, v = bodies(n, SEED), velocities(n, SEED)
        h = spacings * SPACING
        pts, pv = points(n, POINTS, SEED), point_velocities(POINTS, SEED)
        lists, count = radius_rows(b, h, CAP)
        plists, pcount = radius_rows(b, h, CAP, targets=pts)
        assert int(count.max()) <= CAP and int(pcount.max()) <= CAP
        c = {"n": n, "spacings": spacings, "radius": h, "b": b, "v": v, "pts": pts, "pv": pv, "lists": lists, "count": count,
             "plists": plists, "pcount": pcount, "ref": list_ref(b, v, lists), "pref": list_ref(b, v, plists, pts=pts, pvel=pv)}
        for a in (b, v, pts, pv, lists, count, plists, pcount):
            a.setflags(write=False)
        _cache[key] = c
    return _cache[key]


def errors(got_a, got_j, got_phi, ref):
    """The worst row errors (a, jerk, phi) of one result on the census metric; None where nothing was given."""
    ea = None if got_a is None else row_err(np.asarray(got_a)[:, :3], ref["a"], ref["scale"])[1]
    ej = None if got_j is None else row_err(np.asarray(got_j)[:, :3], ref["j"], ref["j_scale"])[1]
    ep = None if got_phi is None else row_err(got_phi, ref["phi"], np.abs(ref["phi"]))[1]
    return ea, ej, ep


def measure(n, spacings):
    c = census_input(n, spacings)
    e = {"n": n, "spacings": spacings, "radius": c["radius"], "cap": CAP, "mean_count": float(c["count"].mean()), "max_count": int(c["count"].max()),
         "points": POINTS, "points_mean_count": float(c["pcount"].mean()), "factor": TOL_FACTOR}
    for pre, ref, kw in (("", c["ref"], {}), ("pt_", c["pref"], {"pts": c["pts"], "pvel": c["pv"]})):
        rows = c["plists"] if pre else c["lists"]
        ea, ej, ep = errors(*list_f32(c["b"], c["v"], rows, **kw), ref)
        for name, err, share in (("a", ea, "min_share"), ("jerk", ej, "j_min_share"), ("phi", ep, "phi_min_share")):
            e[pre + name + "_ref_f32_err"], e[pre + name + "_tol"], e[pre + name + "_min_share"] = err, TOL_FACTOR * err, ref[share]
    return e


def measure_all():
    return {"generator": "tests/golden/measure_list_force.py (tests/list_force_ref.py: a binary32 restatement, ordered ascending sums, against numpy fp64)",
            "metric": "err_k = |got_k - ref_k|_2 / sum_e |term_ke|_2 per row (phi: / |phi_k|); tol = factor x ref_f32_err; every input keeps min_share >= 8 tol",
            "G": G, "eps2": EPS2, "seed": SEED, "tol_f64": TOL_F64,
            "inputs": [measure(n, sp) for n in SIZES for sp in SPACINGS]}


def record():
    with open(JSON_PATH) as f:
        return json.load(f)


def entry(n, spacings):
    return [e for e in record()["inputs"] if e["n"] == n and e["spacings"] == spacings][0]
