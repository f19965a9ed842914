"""The start of an order-6 handle at nb_set_start6(NB_START6_CRACKLE) (include/nbody3d_hip.h) restated in numpy: hermite6_ref.fjs
extended by the pair crackle, in hermite6_ref's two modes (fp64; binary32-storing: every difference and product in binary32, one
ordered ascending binary32 sum per row, G once in fp64), the start that stores it, the two-rule start levels on top of
block_ref.levels_for with margins, block6_ref's outer steps from such a start, the hard-pair fixture of tools/block_bench.py and
the loader of tests/golden/start6.json.  Imported by test_start6_cpu.py, test_start6_gpu.py, test_start6_node.py and
tests/golden/measure_start6.py; not a test module.  Nothing here knows of tiles, chunks or lanes."""
import json
import os

import numpy as np

import block6_ref as B6
import block_ref as B
import hermite6_ref as H6

EPS2, H, SIZES, STEPS, CENSUS, G_PASS = H6.EPS2, H6.H, H6.SIZES, H6.STEPS, H6.CENSUS, H6.G_PASS
QUANTITIES = H6.QUANTITIES
FACTOR = B6.FACTOR                # every tolerance taken from a measured number is this many times the number
JSON_PATH = os.path.join(B.GOLDEN, "start6.json")
ZERO, CRACKLE = 0, 1              # NB_START6_ZERO, NB_START6_CRACKLE


def crk(b, v, a, j, G, eps2=EPS2, f=np.float64, rows=None, scales=False):
    """C of the rows (all by default), (m, 3) in dtype f; with scales also sum_j |term|_2 in fp64.  hermite6_ref.fjs's loop with
      gamma = (3 dv.da + dr.dj) y^2 + alpha (3 beta - 4 alpha^2),   w = dj - 9 alpha q - 9 beta t - 3 gamma dr,   C = s3 w."""
    b = np.asarray(b, f)
    x, m = b[:, :3], b[:, 3]
    u, w_, k_ = np.asarray(v, f)[:, :3], np.asarray(a, f)[:, :3], np.asarray(j, f)[:, :3]
    n = len(x)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    out, sc = np.zeros((len(rows), 3), f), np.zeros(len(rows))
    step = max(1, 1000000 // n)
    three, four, six, nine, e2 = f(3), f(4), f(6), f(9), f(eps2)
    col = lambda z: [np.ascontiguousarray(z[:, k]) for k in range(3)]
    xs, us, ws, ks = col(x), col(u), col(w_), col(k_)
    dot = lambda p, q: p[0] * q[0] + p[1] * q[1] + p[2] * q[2]
    for k0 in range(0, len(rows), step):
        r = rows[k0:k0 + step]
        dr = [xs[k][None, :] - xs[k][r, None] for k in range(3)]
        dv = [us[k][None, :] - us[k][r, None] for k in range(3)]
        da = [ws[k][None, :] - ws[k][r, None] for k in range(3)]
        dj = [ks[k][None, :] - ks[k][r, None] for k in range(3)]
        r2 = dr[2] * dr[2] + (dr[1] * dr[1] + (dr[0] * dr[0] + e2))
        y = f(1) / np.sqrt(r2)
        y2 = y * y
        s3 = (m[None, :] * y) * y2
        alpha = dot(dr, dv) * y2
        beta = (dot(dv, dv) + dot(dr, da)) * y2 + alpha * alpha
        gamma = (three * dot(dv, da) + dot(dr, dj)) * y2 + alpha * (three * beta - four * (alpha * alpha))
        a3, a6, a9, b3, b9, g3 = three * alpha, six * alpha, nine * alpha, three * beta, nine * beta, three * gamma
        t = [dv[k] - a3 * dr[k] for k in range(3)]
        q = [da[k] - a6 * t[k] - b3 * dr[k] for k in range(3)]
        w = [dj[k] - a9 * q[k] - b9 * t[k] - g3 * dr[k] for k in range(3)]
        term = [s3 * w[c] for c in range(3)]
        for c in range(3):
            if f is np.float64:
                total = term[c].sum(1)
            else:      # one addition after the other, ascending j (np.sum would add pairwise)
                total = np.cumsum(term[c], axis=1, dtype=f)[:, -1]
            out[k0:k0 + step, c] = (G * total.astype(np.float64)).astype(f)
        if scales:
            t64 = [z.astype(np.float64) for z in term]
            sc[k0:k0 + step] = abs(G) * np.sqrt(t64[0] * t64[0] + t64[1] * t64[1] + t64[2] * t64[2]).sum(1)
    return (out, sc) if scales else out


def start(b, v, G, eps2=EPS2, f=np.float64, mode=CRACKLE):
    """hermite6_ref.start, and at CRACKLE c = the sum on (x, v, a, j) as stored; a, j and s are the same arrays in both modes."""
    st = H6.start(b, v, G, eps2, f)
    if mode == CRACKLE:
        st["c"] = crk(st["b"], st["v"], st["a"], st["j"], G, eps2, f)
    return st


def run(b, v, G, h, steps, eps2=EPS2, f=np.float64, keep=()):
    """hermite6_ref.run from the CRACKLE start."""
    st = start(b, v, G, eps2, f)
    kept = {}
    for k in range(steps):
        st = H6.step(st, h, G, eps2)
        if k + 1 in keep:
            kept[k + 1] = st
    return kept if keep else st


def _norm(x):
    return np.sqrt((x * x).sum(-1))


def start_levels2(a, j, s, c, dt, eta, lmin, L, stats=None, margins=None):
    """The two-rule start: l_i = max(level_for((eta / 2)|a|/|j|), level_for(sqrt(eta (|a||s| + |j|^2) / (|j||c| + |s|^2)))); a rule
    whose denominator is 0 votes lmin; a body counts once as clamped when either rule found no level.  margins collects the
    relative distance of every finite tau of either rule from its nearest level boundary."""
    na, nj, ns, nc = [_norm(np.asarray(z, np.float64)[:, :3]) for z in (a, j, s, c)]
    den = nj * nc + ns * ns
    with np.errstate(divide="ignore", invalid="ignore"):
        tau1 = np.where(nj == 0, np.inf, 0.5 * eta * na / nj)
        tau2 = np.where(den == 0, np.inf, np.sqrt(eta * (na * ns + nj * nj) / den))
    w1, c1, m1 = B.levels_for(tau1, dt, lmin, L)
    w2, c2, m2 = B.levels_for(tau2, dt, lmin, L)
    w1[nj == 0], c1[nj == 0] = lmin, False
    w2[den == 0], c2[den == 0] = lmin, False
    if stats is not None:
        stats["clamped"] += int((c1 | c2).sum())
    if margins is not None:
        margins.extend(m1[np.isfinite(m1)])
        margins.extend(m2[np.isfinite(m2)])
    return np.maximum(w1, w2), w1, w2


def block(b, v, G, eps2, dt, outer, eta, max_level, min_level=0, mode=CRACKLE, margins=None, start_margins=None):
    """block6_ref.block6_ref from the start of `mode`: (state, levels, stats, start levels).  At ZERO it is block6_ref as it stands."""
    if mode == ZERO:
        st0 = H6.start(b, v, G, eps2)
        stats0 = {"clamped": 0}
        lev0 = B.start_levels(st0["a"], st0["j"], dt, eta, min_level, max_level, stats0, start_margins)
    else:
        st0 = start(b, v, G, eps2)
        stats0 = {"clamped": 0}
        lev0 = start_levels2(st0["a"], st0["j"], st0["s"], st0["c"], dt, eta, min_level, max_level, stats0, start_margins)[0]
    st, lev, stats = B6.block6_ref(b, v, G, eps2, dt, outer, eta=eta, max_level=max_level, min_level=min_level, levels=lev0, state=st0,
                                   margins=margins)
    stats["clamped"] += stats0["clamped"]
    return st, lev, stats, lev0.astype(np.uint8)


def with_tight_pairs(n, seed=1, frac=0.01, half=0.02):
    """tools/block_bench.py's system: ic.plummer with frac * n bodies (consecutive pairs from body 0) re-placed +-half along x about
    the pair's centre of mass on the circular orbit of their masses (G = 1); the arrays rounded to float32."""
    from nbody3d_amd import ic
    b, v = ic.plummer(n, seed=seed)
    b, v = b.astype(np.float64), v.astype(np.float64)
    for p in range(int(frac * n) // 2):
        i, k = 2 * p, 2 * p + 1
        m0, m1 = b[i, 3], b[k, 3]
        c = (m0 * b[i, :3] + m1 * b[k, :3]) / (m0 + m1)
        u = (m0 * v[i, :3] + m1 * v[k, :3]) / (m0 + m1)
        w = np.sqrt((m0 + m1) / (2 * half))
        b[i, :3], b[k, :3] = c + (half, 0, 0), c - (half, 0, 0)
        v[i, :3], v[k, :3] = u + (0, w * m1 / (m0 + m1), 0), u - (0, w * m0 / (m0 + m1), 0)
    return b.astype(np.float32), v.astype(np.float32)


HARD = dict(n=1024, seed=21, frac=0.01, half=0.001, eps2=1e-8, dt=2.0 ** -4, max_level=16, eta=0.05, outer=1)
_cache = {}


def hard_system():
    if "hard" not in _cache:
        p = HARD
        _cache["hard"] = with_tight_pairs(p["n"], p["seed"], p["frac"], p["half"])
    return _cache["hard"]


def hard_ref(mode=CRACKLE):
    """(b0, v0, (state, levels, stats, start levels), first-step |dE/E0|, smallest start margin) of one outer step of HARD."""
    key = ("hardrun", mode)
    if key not in _cache:
        p = HARD
        b0, v0 = hard_system()
        sm = []
        out = block(b0, v0, 1.0, p["eps2"], p["dt"], p["outer"], p["eta"], p["max_level"], mode=mode, start_margins=sm)
        e0, e1 = B.energy(b0, v0, 1.0, p["eps2"]), B6.energy_of(out[0], 1.0, p["eps2"])
        _cache[key] = (b0, v0, out, abs((e1 - e0) / e0), float(min(sm)))
    return _cache[key]


def tiny_system(n, seed):
    return B6.tiny_ref(n, seed)[:2]


def tiny_start(n, seed):
    """(b0, v0, start levels, smallest start margin) of a block6_ref.TINY system under TINY_RUN."""
    key = ("tiny", n, seed)
    if key not in _cache:
        b0, v0 = tiny_system(n, seed)
        p = B6.TINY_RUN
        st = start(b0, v0, 1.0, EPS2)
        sm = []
        lev = start_levels2(st["a"], st["j"], st["s"], st["c"], p["dt"], p["eta"], 0, p["max_level"], None, sm)[0]
        _cache[key] = (b0, v0, lev.astype(np.uint8), float(min(sm)))
    return _cache[key]


def pair300_start():
    key = "pair300"
    if key not in _cache:
        from nbody3d_amd import ic
        p = B6.PAIR300
        b0, v0 = B.tight_pair(*ic.plummer(p["n"], seed=p["seed"]))
        st = start(b0, v0, 1.0, EPS2)
        sm = []
        lev = start_levels2(st["a"], st["j"], st["s"], st["c"], p["dt"], p["eta"], 0, p["max_level"], None, sm)[0]
        _cache[key] = (b0, v0, lev.astype(np.uint8), float(min(sm)))
    return _cache[key]


# ---- the pass cases and the stepping cases (hermite6_ref's systems) ---------------------------------------------------------------
_pass = {}


def pass_ref(key):
    """(b, v, a, j, c, scale) of a pass case: hermite6_ref.pass_ref's stored rows and fp64 (a, j), the fp64 crackle on them and its
    row scale.  Computed once, shared, never written."""
    if key not in _pass:
        b, v, a, j = H6.pass_ref(key)[:4]
        c, sc = crk(b, v, a, j, G_PASS, scales=True)
        c.setflags(write=False)
        _pass[key] = (b, v, a, j, c, sc)
    return _pass[key]


def pass_f32(key):
    b, v = pass_ref(key)[:2]
    return start(b, v, G_PASS, f=np.float32)["c"]


_steps = {}


def steps_ref(n, f=np.float64):
    """{k: state after k steps of H at G = 1 from the CRACKLE start} for k in STEPS."""
    if (n, f) not in _steps:
        b, v = H6.system(n)
        _steps[(n, f)] = run(b, v, 1.0, H, max(STEPS), f=f, keep=STEPS)
    return _steps[(n, f)]


def measure_all(log=print):
    out = {"generator": "tests/golden/measure_start6.py (tests/start6_ref.py: the binary32-storing restatement against the fp64 one, numpy, no device)",
           "fixtures": {"eps2": EPS2, "h": H, "G_pass": G_PASS, "sizes": list(SIZES), "steps": list(STEPS),
                        "census": {k: {"n": v[0], "row": v[1], "mass": 1e3} for k, v in CENSUS.items()}, "hard": HARD, "factor": FACTOR},
           "pass": {}, "steps": {}}
    for key in list(SIZES) + list(CENSUS):
        b, v, a, j, c, sc = pass_ref(key)
        out["pass"][str(key)] = {"c": H6.row_err(pass_f32(key), c, sc)}
        log("pass %-6s binary32 row error of the crackle: %.3g" % (key, out["pass"][str(key)]["c"]))
    for n in SIZES:
        r64, r32 = steps_ref(n), steps_ref(n, np.float32)
        out["steps"][str(n)] = {str(k): H6.distances(r32[k], r64[k], H) for k in STEPS}
        for k in STEPS:
            log("steps N=%-5d k=%d binary32-storing distance: %s" % (n, k, "  ".join("%s %.3g" % kv for kv in out["steps"][str(n)][str(k)].items())))
    hard = {}
    for name, mode in (("zero", ZERO), ("crackle", CRACKLE)):
        _, _, (st, lev, stats, lev0), de, margin = hard_ref(mode)
        hard[name] = {"dE": de, "stats": stats, "start_margin": margin, "start_levels": np.bincount(lev0, minlength=HARD["max_level"] + 1).tolist()}
        log("hard pairs, start %s: %s" % (name, hard[name]))
    out["hard"] = hard
    out["margins"] = {"tiny_%d_%d" % ns: tiny_start(*ns)[3] for ns in B6.TINY}
    out["margins"]["pair300"] = pair300_start()[3]
    log("start margins: %s" % out["margins"])
    return out


_record = {}


def record():
    if not _record:
        with open(JSON_PATH) as fh:
            _record.update(json.load(fh))
    return _record
