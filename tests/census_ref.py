"""Pair census: inputs, fp64 references and the row metric that shows ONE missed, doubled or misattributed pair.  Host only (numpy).

The suite's force metric, max |a - ref| < 2e-5 max |ref|, bounds the rounding of a sum; at N >= 4,096 a sixth to two thirds of the
ordered pairs of a Plummer sphere are smaller than that bound and can vanish unseen.  Here a row is judged on the scale of the terms
that make it up,

    err_i = |a_i - ref_i|_2 / scale_i          scale_i = sum_{j hot} |t_ij|_2          t_ij = G m_j dr_ij / rho_ij^3

and the inputs keep every single share |t_ij| / scale_i large:

  - positions: a jittered lattice (bounded ratio of pair distances, so bounded ratio of terms), scaled by a non-power-of-two;
  - hot sets: run k of K gives mass to the rows i % K == k (random, [0.5, 1.5] / n) and zero to all others, so a row is a sum of n / K
    terms, and the K runs together visit every ordered pair (i <- j) exactly once.  The strided classes put hot bodies into every tile,
    block, chunk and lane class in every run; no kernel branches on a zero mass (padding rows rely on that) and the launch plan depends
    on n only;
  - reference: plain numpy fp64 on the stored (binary32-rounded) rows: every row up to FULL_ROWS_MAX bodies, above that a fixed
    sample of <= 512 rows (sample_rows), each still checked against every column.

The tolerance of an input is MEASURED from the fp32 reference arithmetic by tests/golden/measure_pair_census.py (measure_* below) and
recorded in tests/golden/pair_census.json; tests/test_pair_census_cpu.py holds the record to a fresh measurement and asserts
min_share >= 8 tol for every input, tests/test_pair_census_gpu.py holds the kernels to it.
"""
import json
import os

import numpy as np

EPS2 = 1e-4
G = 0.37
SPACING = 0.137               # lattice spacing: not a power of two, so no coordinate is exact in binary32
JITTER = 0.25                 # +- this share of the spacing, uniform
FULL_ROWS_MAX = 6200          # up to here the reference covers every row
SAMPLE_MAX = 512
TOL_FACTOR = 8.0              # tol = TOL_FACTOR x the fp32 reference's worst err_i; the inputs must keep min_share >= 8 tol
TOL_F64 = 1e-12               # the project's fp64 bound (tests/test_step_forms_gpu.py), on the row metric

JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_census.json")

# The accelerations' inputs: n -> (K, seeds).  One seed per size, except the two-body system: a row there is ONE term, and the rounding
# of one term is a lottery, so the input is 16 systems and the measured error the worst of them.  K is a power of two at which
# min_share >= 8 tol holds with room to spare: 17 x tol at the least (test_pair_census_cpu.py asserts the condition).
ACCEL_INPUTS = {1: (1, (5,)), 2: (2, tuple(range(40, 56))), 77: (4, (5,)), 129: (4, (5,)), 1000: (8, (5,)), 1001: (8, (5,)), 1025: (8, (5,)), 1500: (16, (5,)),
                2047: (16, (5,)), 2048: (16, (5,)), 2049: (16, (5,)), 5 * 512 + 1: (16, (5,)), 3 * 1024 + 64: (32, (5,)), 4099: (32, (5,)),
                5000: (32, (5,)), 6143: (32, (5,)), 8192: (64, (5,)), 12289: (64, (5,)), 16384: (128, (5,)), 20000: (128, (5,)), 20001: (128, (5,))}
FIELD_SIZES = (1025, 4099)    # nb_field_eval: the accelerations' input of that size, plus FIELD_POINTS arbitrary points and the potential
FIELD_POINTS = 300
HERMITE_SIZES = (77, 1025, 4099)
# nb_diagnostics: the potential energy is a scalar, so a hot set is the UNION of two residue classes (a <= b): pairs from different
# classes are hot together; the 136 unions of K = 16 cover every unordered pair, those within a class 16 times over.
DIAG_K = 16
DIAG_SIZES = (2, 257, 1023, 1025, 2049)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def lattice(n, seed, count=None, offset=0.0, jitter=JITTER):
    """`count` (default n) distinct sites of the ceil(n^(1/3))^3 integer lattice in random order, + offset, jittered, scaled; float64."""
    rng = np.random.default_rng(seed)
    count = n if count is None else count
    L = 1
    while L ** 3 < max(n, count):
        L += 1
    site = rng.permutation(L ** 3)[:count]
    p = np.stack([site // (L * L), site // L % L, site % L], axis=1).astype(np.float64)
    return (p + offset + rng.uniform(-jitter, jitter, (count, 3))) * SPACING


def bodies(n, seed):
    """(n, 4) float32 rows (x, y, z, m), every mass set: hot() keeps one residue class of them."""
    b = np.zeros((n, 4), np.float32)
    b[:, :3] = lattice(n, seed)
    b[:, 3] = np.random.default_rng(seed + 1000).uniform(0.5, 1.5, n) / n
    return b


def velocities(n, seed):
    """(n, 4) float32 rows (vx, vy, vz, 0) of order 1 (the Hermite census; the other passes do not read them)."""
    v = np.zeros((n, 4), np.float32)
    v[:, :3] = np.random.default_rng(seed + 2000).normal(0.0, 1.0, (n, 3))
    return v


def points(n, m, seed):
    """m arbitrary points between the bodies of bodies(n, seed): sites of the same lattice shifted by half a spacing, jittered by a
    tenth -- no closer than 0.15 spacings to a body on any axis, so the share of a single body stays bounded.  (m, 4) float32."""
    p = np.zeros((m, 4), np.float32)
    p[:, :3] = lattice(n, seed + 3000, count=m, offset=0.5, jitter=0.1)
    return p


def hot_ids(n, K, k):
    return np.arange(k, n, K)


def hot(b, K, k):
    """The rows of run k: masses of the class i % K == k kept, all others zero."""
    out = b.copy()
    keep = np.zeros(len(b), bool)
    keep[k::K] = True
    out[~keep, 3] = 0
    return out


def hot_union(b, K, a, c):
    out = b.copy()
    keep = np.zeros(len(b), bool)
    keep[a::K] = True
    keep[c::K] = True
    out[~keep, 3] = 0
    return out


def unions(K=DIAG_K):
    return [(a, c) for a in range(K) for c in range(a, K)]


def sample_rows(n):
    """The rows the reference covers: all of them up to FULL_ROWS_MAX bodies; above, a fixed sample of <= SAMPLE_MAX rows -- the first
    and last row of every 256-tile (the 512- and 1,024-row super-blocks begin and end on those), the first and last two rows of the
    system, the rows of the short block behind the last whole 1,024-row super-block (all of them up to 96, else the first and last
    row of each of its 64-row chunks) and random rows for the rest."""
    if n <= FULL_ROWS_MAX:
        return np.arange(n)
    rows = {0, 1, n - 2, n - 1}
    for t in range(0, n, 256):
        rows.update((t, min(t + 255, n - 1)))
    for S in (512, 1024):
        z0 = n // S * S
        if n - z0 <= 96:
            rows.update(range(z0, n))
        else:
            for c in range(z0, n, 64):
                rows.update((c, min(c + 63, n - 1)))
    rows = np.array(sorted(rows))
    assert len(rows) <= SAMPLE_MAX, (n, len(rows))
    rest = np.setdiff1d(np.arange(n), rows)
    extra = np.random.default_rng(n).choice(rest, SAMPLE_MAX - len(rows), replace=False)
    return np.sort(np.concatenate([rows, extra]))


# ---- fp64 references -------------------------------------------------------------------------------------------------------------
def _blocks(m, q):
    step = max(1, 1500000 // max(1, q))
    for k0 in range(0, m, step):
        yield k0, min(m, k0 + step)


def row_ref(b, rows, G=G, eps2=EPS2, targets=None, vel=None):
    """fp64 direct sums over the HOT rows of b (mass != 0) for the given rows of b -- or, with `targets` (m, >=3), for those points, none
    of them a body.  Returns a dict of float64 arrays: a (m, 3), scale (m,), min_share (float: the smallest |t_ij| / scale_i over the
    rows and the hot j != i, inf when there is no term; argmin = (its position in rows, its j)), phi (m,) = -sum G m_j / rho (its scale is |phi|: one sign), phi_min_share, and
    with vel (n, >=3) the jerk j (m, 3) = sum G m_j (dv / rho^3 - 3 (dr.dv) dr / rho^5) and its own scale j_scale = sum |term|_2."""
    bq = np.asarray(b, np.float64)
    q = np.nonzero(bq[:, 3])[0]
    xq, mq = bq[q, :3], bq[q, 3]
    if targets is None:
        rows = np.asarray(rows)
        xt = bq[rows, :3]
    else:
        xt = np.asarray(targets, np.float64)[:, :3]
        rows = np.full(len(xt), -1)
    m = len(xt)
    out = {"a": np.zeros((m, 3)), "scale": np.zeros(m), "phi": np.zeros(m)}
    if vel is not None:
        u = np.asarray(vel, np.float64)[:, :3]
        out["j"], out["j_scale"] = np.zeros((m, 3)), np.zeros(m)
    min_share, phi_min_share = np.inf, np.inf
    for k0, k1 in _blocks(m, len(q)):
        dr = xq[None, :, :] - xt[k0:k1, None, :]
        other = q[None, :] != rows[k0:k1, None]                      # the self pair: dr = 0, its term is exactly 0 and is no share
        y2 = 1.0 / ((dr * dr).sum(2) + eps2)
        y = np.sqrt(y2)
        w = G * mq[None, :] * other
        t = (w * y2 * y)[:, :, None] * dr
        tn = np.sqrt((t * t).sum(2))
        out["a"][k0:k1] = t.sum(1)
        out["scale"][k0:k1] = tn.sum(1)
        p = w * y
        out["phi"][k0:k1] = -p.sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(other, tn / tn.sum(1)[:, None], np.inf)
            pshare = np.where(other, p / p.sum(1)[:, None], np.inf)
        if share.size:
            if float(share.min()) < min_share:
                r, c = np.unravel_index(share.argmin(), share.shape)
                out["argmin"] = (k0 + int(r), int(q[c]))                  # (position in `rows`, j) of the smallest share
            min_share, phi_min_share = min(min_share, float(share.min())), min(phi_min_share, float(pshare.min()))
        if vel is not None:
            dv = u[q][None, :, :] - u[rows[k0:k1]][:, None, :]
            rv = (dr * dv).sum(2) * y2
            tj = (w * y2 * y)[:, :, None] * (dv - 3.0 * rv[:, :, None] * dr)
            out["j"][k0:k1] = tj.sum(1)
            out["j_scale"][k0:k1] = np.sqrt((tj * tj).sum(2)).sum(1)
    out["min_share"], out["phi_min_share"] = min_share, phi_min_share
    return out


def row_err(got, ref, scale):
    """err_i = |got_i - ref_i|_2 / scale_i, and the worst of them.  Rows without a term (scale 0) must be exactly zero."""
    got = np.asarray(got, np.float64)
    if got.ndim == 1:
        got, ref = got[:, None], np.asarray(ref)[:, None]
    d = np.sqrt(((got[:, :ref.shape[1]] - ref) ** 2).sum(1))
    empty = scale == 0
    assert not got[empty].any(), "a row without a single term is not exactly zero"
    err = np.where(empty, 0.0, d / np.where(empty, 1.0, scale))
    return err, float(err.max()) if len(err) else 0.0


def pe_ref(b, G=G, eps2=EPS2):
    """(PE, scale, min_share) of the hot rows in fp64: PE = -sum_{i<j hot} G m_i m_j / rho; every term has one sign, so scale = |PE|."""
    bq = np.asarray(b, np.float64)
    q = np.nonzero(bq[:, 3])[0]
    x, m = bq[q, :3], bq[q, 3]
    d = x[None, :, :] - x[:, None, :]
    t = G * m[None, :] * m[:, None] / np.sqrt((d * d).sum(2) + eps2)
    iu = np.triu_indices(len(q), 1)
    t = t[iu]
    s = float(t.sum())
    return -s, s, (float(t.min()) / s if len(t) else np.inf)


def ke_mom_ref(b, v):
    m = np.asarray(b, np.float64)[:, 3]
    u = np.asarray(v, np.float64)[:, :3]
    return float(0.5 * (m * (u * u).sum(1)).sum()), (m[:, None] * u).sum(0)


# ---- the fp32 reference arithmetic, for the tolerances ----------------------------------------------------------------------------
def oracle_rows_f32(b, rows=None, targets=None, G=G, eps2=EPS2):
    """oracle.accel_f32 (the reference's ordered binary32 loop) for rows of b or for arbitrary points.  The oracle is handed the hot
    rows followed by zero-mass copies of the targets: a zero-mass j adds an exact zero to the ordered sum and a target's own hot copy
    sits at distance 0 (an exact zero too), so the sums are bit for bit those of the whole system (test_pair_census_cpu.py checks it)."""
    from oracle import oracle
    b = np.asarray(b, np.float32)
    q = np.nonzero(b[:, 3])[0]
    t = np.zeros((len(rows) if targets is None else len(targets), 4), np.float32)
    t[:, :3] = b[rows, :3] if targets is None else np.asarray(targets, np.float32)[:, :3]
    packed = np.concatenate([b[q], t])
    return oracle.accel_f32(packed, G, eps2=eps2, i0=len(q), i1=len(packed))[:, :3]


def _f32_terms(b, rows, targets, vel, G, eps2):
    """The binary32 restatement of one pair, rho^-1 = 1 / sqrt(r2) correctly rounded: (w y^3, dr, w y, y2, dv | None), self pairs w = 0."""
    f = np.float32
    b = np.asarray(b, f)
    q = np.nonzero(b[:, 3])[0]
    if targets is None:
        xt, ids = b[rows, :3], np.asarray(rows)
    else:
        xt, ids = np.asarray(targets, f)[:, :3], np.full(len(targets), -1)
    dr = b[q, :3][None, :, :] - xt[:, None, :]
    r2 = dr[:, :, 2] * dr[:, :, 2] + (dr[:, :, 1] * dr[:, :, 1] + (dr[:, :, 0] * dr[:, :, 0] + f(eps2)))
    y = f(1) / np.sqrt(r2)
    w = (f(G) * b[q, 3])[None, :] * (q[None, :] != ids[:, None])
    dv = None
    if vel is not None:
        u = np.asarray(vel, f)[:, :3]
        dv = u[q][None, :, :] - u[ids][:, None, :]
    return w * (y * y * y), dr, w * y, y * y, dv


def _ordered_sum(t, axis=1):
    """A binary32 sum in ascending j, one addition after the other (np.sum would add pairwise)."""
    if t.shape[axis] == 0:
        return np.zeros(np.delete(t.shape, axis), np.float32)
    return np.take(np.cumsum(t, axis=axis, dtype=np.float32), -1, axis=axis)


def phi_f32(b, rows=None, targets=None, G=G, eps2=EPS2):
    out = []
    n_t = len(rows) if targets is None else len(targets)
    for k0 in range(0, n_t, 256):
        sl = slice(k0, k0 + 256)
        _, _, p, _, _ = _f32_terms(b, None if rows is None else np.asarray(rows)[sl], None if targets is None else targets[sl], None, G, eps2)
        out.append(-_ordered_sum(p))
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def jerk_f32(b, vel, rows, G=G, eps2=EPS2):
    """include/nbody3d_hip.h's jerk, j_i = sum_j G m_j [dv / rho^3 - 3 (dr.dv) dr / rho^5], restated in binary32 with an ordered sum."""
    out = []
    f = np.float32
    for k0 in range(0, len(rows), 256):
        s3, dr, _, y2, dv = _f32_terms(b, np.asarray(rows)[k0:k0 + 256], None, vel, G, eps2)
        rv = (dr[:, :, 0] * dv[:, :, 0] + dr[:, :, 1] * dv[:, :, 1] + dr[:, :, 2] * dv[:, :, 2]) * y2
        out.append(_ordered_sum(s3[:, :, None] * (dv - (f(3) * rv)[:, :, None] * dr)))
    return np.concatenate(out) if out else np.zeros((0, 3), f)


def pe_f32(b, G=G, eps2=EPS2):
    """nb_diag's arithmetic as its header states it: dr, r2 and 1 / sqrt(r2) in binary32 per pair, m_j / rho accumulated in fp64."""
    f = np.float32
    b = np.asarray(b, f)
    q = np.nonzero(b[:, 3])[0]
    x, m = b[q, :3], b[q, 3].astype(np.float64)
    total = 0.0
    for k0 in range(0, len(q), 512):
        dr = x[None, :, :] - x[k0:k0 + 512, None, :]
        r2 = dr[:, :, 2] * dr[:, :, 2] + (dr[:, :, 1] * dr[:, :, 1] + (dr[:, :, 0] * dr[:, :, 0] + f(eps2)))
        y = (f(1) / np.sqrt(r2)).astype(np.float64)
        upper = np.arange(len(q))[None, :] > np.arange(k0, min(k0 + 512, len(q)))[:, None]
        total += float((m[k0:k0 + 512] * (y * m[None, :] * upper).sum(1)).sum())
    return -G * total


# ---- measurements (tests/golden/measure_pair_census.py writes them; the CPU test repeats them) ---------------------------------------
_cache = {}


def cached_bodies(n, seed):
    if ("b", n, seed) not in _cache:
        b = bodies(n, seed)
        b.setflags(write=False)
        _cache[("b", n, seed)] = b
    return _cache[("b", n, seed)]


def accel_reference(n):
    """The fp64 reference of the accelerations' input of size n, computed once and shared: dict(K, seeds, rows, runs) with runs[(seed, k)]
    = row_ref(...) of hot(bodies(n, seed), K, k) on `rows`, jerk included for the Hermite sizes."""
    if ("a", n) not in _cache:
        K, seeds = ACCEL_INPUTS[n]
        rows = sample_rows(n)
        runs = {}
        for seed in seeds:
            b = bodies(n, seed)
            v = velocities(n, seed) if n in HERMITE_SIZES else None
            for k in range(K):
                runs[(seed, k)] = row_ref(hot(b, K, k), rows, vel=v)
        _cache[("a", n)] = {"K": K, "seeds": seeds, "rows": rows, "runs": runs}
    return _cache[("a", n)]


def field_reference(n):
    """The same at FIELD_POINTS arbitrary points (accelerations and potential)."""
    if ("f", n) not in _cache:
        K, seeds = ACCEL_INPUTS[n]
        b, pts = bodies(n, seeds[0]), points(n, FIELD_POINTS, seeds[0])
        _cache[("f", n)] = {"K": K, "seed": seeds[0], "points": pts, "runs": {k: row_ref(hot(b, K, k), None, targets=pts) for k in range(K)}}
    return _cache[("f", n)]


def diag_reference(n):
    if ("d", n) not in _cache:
        b = bodies(n, 7)
        v = velocities(n, 7)
        _cache[("d", n)] = {"b": b, "v": v, "runs": {u: pe_ref(hot_union(b, DIAG_K, *u)) for u in unions()}}
    return _cache[("d", n)]


def measure_accel(n):
    ref = accel_reference(n)
    K, rows = ref["K"], ref["rows"]
    worst = worst_j = worst_phi = 0.0
    min_share = phi_min_share = np.inf
    for (seed, k), r in ref["runs"].items():
        hb = hot(bodies(n, seed), K, k)
        worst = max(worst, row_err(oracle_rows_f32(hb, rows), r["a"], r["scale"])[1])
        min_share = min(min_share, r["min_share"])
        if n in HERMITE_SIZES:
            worst_j = max(worst_j, row_err(jerk_f32(hb, velocities(n, seed), rows), r["j"], r["j_scale"])[1])
        if n in FIELD_SIZES:
            worst_phi = max(worst_phi, row_err(phi_f32(hb, rows), r["phi"], np.abs(r["phi"]))[1])
            phi_min_share = min(phi_min_share, r["phi_min_share"])
    e = {"n": n, "K": K, "seeds": list(ref["seeds"]), "rows": int(len(rows)), "ref_f32_err": worst, "min_share": min_share,
         "factor": TOL_FACTOR, "tol": TOL_FACTOR * worst}
    if n in HERMITE_SIZES:
        e.update(jerk_ref_f32_err=worst_j, jerk_factor=TOL_FACTOR, jerk_tol=TOL_FACTOR * worst_j)
    if n in FIELD_SIZES:
        e.update(phi_ref_f32_err=worst_phi, phi_min_share=phi_min_share, phi_factor=TOL_FACTOR, phi_tol=TOL_FACTOR * worst_phi)
    return e


def measure_field(n):
    ref = field_reference(n)
    b = bodies(n, ref["seed"])
    worst = worst_phi = 0.0
    min_share = phi_min_share = np.inf
    for k, r in ref["runs"].items():
        hb = hot(b, ref["K"], k)
        worst = max(worst, row_err(oracle_rows_f32(hb, targets=ref["points"]), r["a"], r["scale"])[1])
        worst_phi = max(worst_phi, row_err(phi_f32(hb, targets=ref["points"]), r["phi"], np.abs(r["phi"]))[1])
        min_share, phi_min_share = min(min_share, r["min_share"]), min(phi_min_share, r["phi_min_share"])
    return {"n": n, "K": ref["K"], "seed": ref["seed"], "points": FIELD_POINTS, "ref_f32_err": worst, "min_share": min_share, "factor": TOL_FACTOR,
            "tol": TOL_FACTOR * worst, "phi_ref_f32_err": worst_phi, "phi_min_share": phi_min_share, "phi_factor": TOL_FACTOR, "phi_tol": TOL_FACTOR * worst_phi}


def measure_diag(n):
    ref = diag_reference(n)
    worst, min_share = 0.0, np.inf
    for u, (pe, scale, share) in ref["runs"].items():
        if scale:
            worst = max(worst, abs(pe_f32(hot_union(ref["b"], DIAG_K, *u)) - pe) / scale)
            min_share = min(min_share, share)
    return {"n": n, "K": DIAG_K, "seed": 7, "unions": len(ref["runs"]), "ref_f32_err": worst, "min_share": min_share, "factor": TOL_FACTOR,
            "tol": TOL_FACTOR * worst}


# A kernel that exceeds 8 x the reference's error with every pair present: (kind, n, "" | "jerk_" | "phi_") -> the raised factor, what the
# device gave and why.  Only while min_share >= 4 tol still holds (test_pair_census_cpu.py asserts it).
RAISED = {}


def _raise_factors(kind, e):
    for pre in ("", "jerk_", "phi_"):
        r = RAISED.get((kind, e["n"], pre))
        if r:
            e[pre + "factor"], e[pre + "tol"] = r["factor"], r["factor"] * e[pre + "ref_f32_err"]
            e[pre + "device_err"], e[pre + "why"] = r["device_err"], r["why"]
    return e


def _finite(e):
    """json has no infinity: an input without a single pair (n = 1) records min_share null."""
    return {k: (None if isinstance(v, float) and not np.isfinite(v) else v) for k, v in e.items()}


def measure_all():
    return {"generator": "tests/golden/measure_pair_census.py (tests/census_ref.py: oracle.accel_f32 and binary32 restatements against numpy fp64)",
            "metric": "err_i = |a_i - ref_i|_2 / sum_j |t_ij|_2 per row; tol = factor x ref_f32_err; every input keeps min_share >= 8 tol",
            "G": G, "eps2": EPS2, "tol_f64": TOL_F64,
            "accel": [_finite(_raise_factors("accel", measure_accel(n))) for n in sorted(ACCEL_INPUTS)],
            "field_points": [_raise_factors("field_points", measure_field(n)) for n in FIELD_SIZES],
            "diag": [_raise_factors("diag", measure_diag(n)) for n in DIAG_SIZES]}


def record():
    with open(JSON_PATH) as f:
        return json.load(f)


def entry(kind, n):
    return [e for e in record()[kind] if e["n"] == n][0]
