"""The 6th-order Hermite scheme of include/nbody3d_hip.h (nb_set_hermite_order(6)) restated in numpy: the force+jerk+snap sums and
one predictor-corrector step.  Two modes:
  - fp64 (f = np.float64): every array and every operation binary64; a row's sum is np.sum over j.
  - binary32-storing (f = np.float32): every stored array (x, v, a, j, s, c, the predicted state) is rounded to binary32, the
    polynomials of predictor and corrector run in fp64 on the stored values and are rounded once, and the pass that produces the
    stored (a, j, s) is the binary32 restatement of the pair sums: every difference, product and 1 / sqrt(r2) (correctly rounded)
    in binary32, each row ONE ordered ascending binary32 sum, G applied once in fp64.  What this mode differs by from the fp64
    one is what binary32 costs the scheme: the bounds of the f32 handles are 8 x that (tests/golden/hermite6.json).
Nothing here knows of tiles, chunks or lanes."""
import numpy as np

EPS2 = 1e-4          # the engine's default softening
H = 2.0 ** -6        # the step of the stepping cases
SIZES = (2, 3, 257, 1025, 4099)
STEPS = (1, 2, 5)
KEPLER_STEPS = (128, 256, 512)     # steps per period of the convergence cases; the solution they are held against takes 4 x the last
KEPLER_EPS2 = 1e-8


def fjs(b, v, a, G, eps2=EPS2, f=np.float64, rows=None, scales=False):
    """(A, J, S) of the rows (all by default), (m, 3) each in dtype f; with scales also sum_j |term|_2 of each in fp64.
    a may be None: zeros (A and J do not read it)."""
    b = np.asarray(b, f)
    x, m, u = b[:, :3], b[:, 3], np.asarray(v, f)[:, :3]
    w = np.zeros_like(x) if a is None else np.asarray(a, f)[:, :3]
    n = len(x)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    out = [np.zeros((len(rows), 3), f) for _ in range(3)]
    sc = [np.zeros(len(rows)) for _ in range(3)]
    step = max(1, 1000000 // n)
    three, six, e2 = f(3), f(6), f(eps2)
    xs, us, ws = [np.ascontiguousarray(x[:, k]) for k in range(3)], [np.ascontiguousarray(u[:, k]) for k in range(3)], [np.ascontiguousarray(w[:, k]) for k in range(3)]
    for k0 in range(0, len(rows), step):
        r = rows[k0:k0 + step]
        dr = [xs[k][None, :] - xs[k][r, None] for k in range(3)]         # one (rows, n) array per component
        dv = [us[k][None, :] - us[k][r, None] for k in range(3)]
        da = [ws[k][None, :] - ws[k][r, None] for k in range(3)]
        r2 = dr[2] * dr[2] + (dr[1] * dr[1] + (dr[0] * dr[0] + e2))
        y = f(1) / np.sqrt(r2)
        y2 = y * y
        s3 = (m[None, :] * y) * y2
        alpha = (dr[0] * dv[0] + dr[1] * dv[1] + dr[2] * dv[2]) * y2
        vr = (dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]) + (dr[0] * da[0] + dr[1] * da[1] + dr[2] * da[2])
        beta = vr * y2 + alpha * alpha
        a3, a6, b3 = three * alpha, six * alpha, three * beta
        t = [dv[k] - a3 * dr[k] for k in range(3)]
        q = [da[k] - a6 * t[k] - b3 * dr[k] for k in range(3)]
        for k, vec in enumerate((dr, t, q)):
            term = [s3 * vec[c] for c in range(3)]
            for c in range(3):
                if f is np.float64:
                    total = term[c].sum(1)
                else:      # one addition after the other, ascending j (np.sum would add pairwise)
                    total = np.cumsum(term[c], axis=1, dtype=f)[:, -1]
                out[k][k0:k0 + step, c] = (G * total.astype(np.float64)).astype(f)
            if scales:
                t64 = [z.astype(np.float64) for z in term]
                sc[k][k0:k0 + step] = abs(G) * np.sqrt(t64[0] * t64[0] + t64[1] * t64[1] + t64[2] * t64[2]).sum(1)
    return tuple(out) + (tuple(sc),) if scales else tuple(out)


def start(b, v, G, eps2=EPS2, f=np.float64):
    """The start: (a, j) from the sums on (x, v), s from the sums on (x, v, a), c = 0.  The state is a dict of (n, 4) / (n, 3) arrays
    of dtype f: b (x, y, z, m), v (n, 4), a, j, s, c (n, 3)."""
    b, v = np.array(b, f), np.array(v, f)
    a, j, _ = fjs(b, v, None, G, eps2, f)
    s = fjs(b, v, a, G, eps2, f)[2]
    return {"b": b, "v": v, "a": a, "j": j, "s": s, "c": np.zeros_like(a)}


def crackle(a0, j0, s0, a1, j1, s1, h):
    """c1 = p'''(t1) of the quintic through (a, j, s) at both ends of a step h, in fp64."""
    P = a1 - a0 - h * j0 - h * h / 2 * s0
    Q = h * (j1 - j0 - h * s0)
    R = h * h * (s1 - s0)
    return (60.0 * P - 36.0 * Q + 9.0 * R) / h ** 3


def step(st, h, G, eps2=EPS2):
    """One step of the scheme; returns the new state (the old one is not written)."""
    f = st["b"].dtype.type
    d = lambda z: np.asarray(z, np.float64)
    x, v, a, j, s, c = d(st["b"][:, :3]), d(st["v"][:, :3]), d(st["a"]), d(st["j"]), d(st["s"]), d(st["c"])
    bp, vp = st["b"].copy(), st["v"].copy()
    bp[:, :3] = (x + h * (v + h / 2 * (a + h / 3 * (j + h / 4 * (s + h / 5 * c))))).astype(f)
    vp[:, :3] = (v + h * (a + h / 2 * (j + h / 3 * (s + h / 4 * c)))).astype(f)
    ap = (a + h * (j + h / 2 * (s + h / 3 * c))).astype(f)
    a1, j1, s1 = fjs(bp, vp, ap, G, eps2, f)              # as stored
    A1, J1, S1 = d(a1), d(j1), d(s1)
    v1 = v + h / 2 * (a + A1) - h * h / 10 * (J1 - j) + h ** 3 / 120 * (s + S1)
    x1 = x + h / 2 * (v + v1) - h * h / 10 * (A1 - a) + h ** 3 / 120 * (j + J1)
    nb, nv = st["b"].copy(), st["v"].copy()
    nb[:, :3], nv[:, :3] = x1.astype(f), v1.astype(f)
    return {"b": nb, "v": nv, "a": a1, "j": j1, "s": s1, "c": crackle(a, j, s, A1, J1, S1, h).astype(f)}


def run(b, v, G, h, steps, eps2=EPS2, f=np.float64, keep=()):
    """`steps` steps from a start; h may be a sequence of steps sizes.  Returns the final state, or with keep = (k, ...) a dict
    {k: the state after k steps}."""
    st = start(b, v, G, eps2, f)
    hs = [h] * steps if np.isscalar(h) else list(h)
    kept = {}
    for k in range(len(hs)):
        st = step(st, hs[k], G, eps2)
        if k + 1 in keep:
            kept[k + 1] = st
    return kept if keep else st


QUANTITIES = ("x", "v", "a", "j", "s", "c")


def parts(st):
    return {"x": st["b"][:, :3], "v": st["v"][:, :3], "a": st["a"], "j": st["j"], "s": st["s"], "c": st["c"]}


def distances(got, ref, h):
    """max |got - ref| of each quantity over the largest |x|, |v|, |a|, |j|, |s| of the reference; the crackle over 60 max |a| / h^3
    (the differences that make c1 are divided by h^3)."""
    g, r = parts(got), parts(ref)
    out = {}
    for q in QUANTITIES:
        big = float(np.abs(np.asarray(r[q], np.float64)).max())
        if q == "c":
            big = 60.0 * float(np.abs(np.asarray(r["a"], np.float64)).max()) / h ** 3
        out[q] = float(np.abs(np.asarray(g[q], np.float64) - np.asarray(r[q], np.float64)).max()) / big
    return out


def kepler_pair():
    """Masses 0.6 / 0.4, relative orbit a = 1, e = 0.5, from pericentre: period 2 pi at G = 1."""
    m1, m2 = 0.6, 0.4
    r, w = 0.5, np.sqrt(3.0)
    b0 = np.array([[-m2 * r, 0, 0, m1], [m1 * r, 0, 0, m2]], np.float64)
    v0 = np.array([[0, -m2 * w, 0, 0], [0, m1 * w, 0, 0]], np.float64)
    return b0, v0


def system(n, seed=None):
    """The stepping and pass cases: the Kepler pair at N = 2, a Plummer sphere otherwise (with one heavier body)."""
    from nbody3d_amd import ic
    if n == 2:
        b, v = kepler_pair()
        return b.astype(np.float32), v.astype(np.float32)
    b, v = ic.plummer(n, seed=200 + n % 89 if seed is None else seed)
    if n > 7:
        b[7, 3] = 0.05
    return b, v


# ---- the cases and what binary32 costs them (tests/golden/hermite6.json) ------------------------------------------------------
import json      # noqa: E402
import os        # noqa: E402

JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hermite6.json")
G_PASS = 0.37                      # the pass cases (not a power of two)
CENSUS = {"tile": (257, 256), "chunk": (4099, 2304)}     # (n, row of the body of mass 1e3): the last row of the last tile; the first row of the second j-chunk
DT_SEQUENCE = (H, H / 2, H / 2, H)


def census_system(name):
    n, row = CENSUS[name]
    b, v = system(n)
    b = b.copy()
    b[row, 3] = 1e3
    return b, v


def row_err(got, ref, scale):
    """The project's row metric: the worst |got_i - ref_i|_2 / sum_j |term_ij|_2."""
    d = np.sqrt(((np.asarray(got, np.float64)[:, :3] - np.asarray(ref, np.float64)[:, :3]) ** 2).sum(1))
    assert (scale > 0).all()
    return float((d / scale).max())


_pass = {}


def pass_ref(key):
    """(b, v, a, j, s, scales) of a pass case in fp64 on the stored (binary32) rows at G_PASS: computed once, shared, never written.
    key: a size of SIZES or a name of CENSUS."""
    if key not in _pass:
        b, v = census_system(key) if key in CENSUS else system(key)
        a, j, _ = fjs(b, v, None, G_PASS)
        s, sc = fjs(b, v, a, G_PASS, scales=True)[2:]
        for z in (b, v, a, j, s):
            z.setflags(write=False)
        _pass[key] = (b, v, a, j, s, sc)
    return _pass[key]


def pass_f32(key):
    b, v = pass_ref(key)[:2]
    st = start(b, v, G_PASS, f=np.float32)
    return st["a"], st["j"], st["s"]


_steps = {}


def steps_ref(n, f=np.float64):
    """{k: state after k steps of H at G = 1} for k in STEPS: computed once per (n, mode), shared, never written."""
    if (n, f) not in _steps:
        b, v = system(n)
        _steps[(n, f)] = run(b, v, 1.0, H, max(STEPS), f=f, keep=STEPS)
    return _steps[(n, f)]


def kepler_ends(f=np.float64, steps=KEPLER_STEPS + (4 * KEPLER_STEPS[-1],)):
    b0, v0 = kepler_pair()
    return {k: run(b0, v0, 1.0, 2 * np.pi / k, k, eps2=KEPLER_EPS2, f=f) for k in steps}


def measure_all(log=print):
    out = {"generator": "tests/golden/measure_hermite6.py (tests/hermite6_ref.py: the binary32-storing restatement against the fp64 one, numpy, no device)",
           "fixtures": {"eps2": EPS2, "h": H, "G_pass": G_PASS, "sizes": list(SIZES), "steps": list(STEPS),
                        "census": {k: {"n": v[0], "row": v[1], "mass": 1e3} for k, v in CENSUS.items()},
                        "dt_sequence": list(DT_SEQUENCE), "kepler_steps": list(KEPLER_STEPS), "kepler_eps2": KEPLER_EPS2,
                        "kepler_bodies": kepler_pair()[0].tolist(), "kepler_vel": kepler_pair()[1].tolist()},
           "pass": {}, "steps": {}}
    for key in list(SIZES) + list(CENSUS):
        b, v, a, j, s, sc = pass_ref(key)
        ga, gj, gs = pass_f32(key)
        e = {"a": row_err(ga, a, sc[0]), "j": row_err(gj, j, sc[1]), "s": row_err(gs, s, sc[2])}
        out["pass"][str(key)] = e
        log("pass %-6s binary32 row error: a %.3g  j %.3g  s %.3g" % (key, e["a"], e["j"], e["s"]))
    for n in SIZES:
        r64, r32 = steps_ref(n), steps_ref(n, np.float32)
        out["steps"][str(n)] = {str(k): distances(r32[k], r64[k], H) for k in STEPS}
        for k in STEPS:
            log("steps N=%-5d k=%d binary32-storing distance: %s" % (n, k, "  ".join("%s %.3g" % kv for kv in out["steps"][str(n)][str(k)].items())))
    b, v = system(257)
    d = distances(run(b, v, 1.0, DT_SEQUENCE, len(DT_SEQUENCE), f=np.float32), run(b, v, 1.0, DT_SEQUENCE, len(DT_SEQUENCE)), min(DT_SEQUENCE))
    out["dt_sequence"] = d
    log("dt sequence N=257 binary32-storing distance: %s" % "  ".join("%s %.3g" % kv for kv in d.items()))
    ends = kepler_ends()
    fine = ends[4 * KEPLER_STEPS[-1]]["b"][:, :3]
    err = {k: float(np.abs(ends[k]["b"][:, :3] - fine).max()) for k in KEPLER_STEPS}
    out["kepler"] = {"errors": {str(k): err[k] for k in KEPLER_STEPS},
                     "ratios": [err[KEPLER_STEPS[i]] / err[KEPLER_STEPS[i + 1]] for i in range(len(KEPLER_STEPS) - 1)]}
    log("Kepler e = 0.5, one period, steps %s: errors %s, ratios %s" % (KEPLER_STEPS, ["%.3g" % err[k] for k in KEPLER_STEPS], ["%.1f" % r for r in out["kepler"]["ratios"]]))
    return out


_record = {}


def record():
    if not _record:
        with open(JSON_PATH) as fh:
            _record.update(json.load(fh))
    return _record
