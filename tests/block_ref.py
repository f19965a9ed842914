"""The fp64 numpy restatement of the block-time-step Hermite scheme (include/nbody3d_hip.h, "block individual time steps"), next
to a copy of the force+jerk direct sum, and the systems the block-step tests share.  Imported by test_block_cpu.py,
test_block_gpu.py and test_block_node.py; not a test module."""
import numpy as np

EPS2 = 1e-4                       # the engine's default softening


def fj_ref(b, v, G, eps2, rows=None):
    """Force and jerk by direct summation in fp64 (a copy of test_hermite_gpu.fj_ref)."""
    x, m, u = np.asarray(b, np.float64)[:, :3], np.asarray(b, np.float64)[:, 3], np.asarray(v, np.float64)[:, :3]
    rows = np.arange(len(x)) if rows is None else np.asarray(rows)
    a, j = np.zeros((len(rows), 3)), np.zeros((len(rows), 3))
    for s in range(0, len(rows), 256):
        r = rows[s:s + 256]
        dr, dv = x[None, :, :] - x[r, None, :], u[None, :, :] - u[r, None, :]
        y2 = 1.0 / ((dr * dr).sum(2) + eps2)
        s3 = m[None, :] * y2 * np.sqrt(y2)
        q = (dr * dv).sum(2) * y2
        a[s:s + 256] = G * (s3[:, :, None] * dr).sum(1)
        j[s:s + 256] = G * (s3[:, :, None] * (dv - 3.0 * q[:, :, None] * dr)).sum(1)
    return a, j


def hermite_ref(b, v, G, eps2, h, steps, aj=None):
    """One shared step h (a copy of test_hermite_gpu.hermite_ref)."""
    b, v = np.array(b, np.float64), np.array(v, np.float64)
    a, j = fj_ref(b, v, G, eps2) if aj is None else aj
    for _ in range(steps):
        bp, vp = b.copy(), v.copy()
        bp[:, :3] = b[:, :3] + h * v[:, :3] + h * h / 2 * a + h ** 3 / 6 * j
        vp[:, :3] = v[:, :3] + h * a + h * h / 2 * j
        a1, j1 = fj_ref(bp, vp, G, eps2)
        v1 = v[:, :3] + h / 2 * (a + a1) + h * h / 12 * (j - j1)
        b[:, :3] = b[:, :3] + h / 2 * (v[:, :3] + v1) + h * h / 12 * (a - a1)
        v[:, :3], a, j = v1, a1, j1
    return b, v, a, j


def norm_err(got, ref):
    """The project's metric: max |delta|_inf / max |ref|_inf."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def energy(b, v, G, eps2):
    b, v = np.asarray(b, np.float64), np.asarray(v, np.float64)
    m = b[:, 3]
    d = b[None, :, :3] - b[:, None, :3]
    inv = 1.0 / np.sqrt((d * d).sum(2) + eps2)
    np.fill_diagonal(inv, 0.0)
    return 0.5 * (m * (v[:, :3] ** 2).sum(1)).sum() - 0.5 * G * (m[:, None] * m[None, :] * inv).sum()


def _norm(x):
    return np.sqrt((x * x).sum(-1))


def level_for(tau, dt, lmin, L, stats, margins=None):
    """The smallest l in [lmin, L] with dt / 2^l <= tau; none: L, counted as clamped.  margins collects the relative distance of
    tau from the nearest level boundary."""
    if margins is not None and np.isfinite(tau):
        margins.append(min(abs(tau / (dt / 2.0 ** l) - 1.0) for l in range(lmin, L + 1)))
    for l in range(lmin, L + 1):
        if dt / 2.0 ** l <= tau:
            return l
    stats["clamped"] += 1
    return L


def start_levels(a, j, dt, eta, lmin, L, stats, margins=None):
    na, nj = _norm(np.asarray(a, np.float64)), _norm(np.asarray(j, np.float64))
    return np.array([lmin if nj[i] == 0 else level_for(0.5 * eta * na[i] / nj[i], dt, lmin, L, stats, margins)
                     for i in range(len(na))], np.int64)


def block_ref(b, v, G, eps2, dt, outer, eta=0.02, max_level=20, min_level=0, levels=None, frozen=False, aj=None, margins=None,
              store=np.float64):
    """`outer` outer steps of dt with block individual time steps.  levels: initial levels (None: the start rule, or min_level
    everywhere when frozen); aj: derivatives carried over (None: evaluated); store: the precision (a1, j1) and the state are
    rounded to when stored.  Returns (b, v, a, j, levels, stats)."""
    rnd = lambda z: np.asarray(z, store).astype(np.float64)
    b, v = np.array(b, np.float64), np.array(v, np.float64)
    n, L = len(b), max_level
    a, j = [rnd(z) for z in (fj_ref(b, v, G, eps2) if aj is None else aj)]
    a, j = np.array(a[:, :3]), np.array(j[:, :3])
    stats = {"outer_steps": 0, "block_steps": 0, "body_steps": 0, "clamped": 0, "finest_level": 0}
    if levels is None:
        lev = np.full(n, min_level, np.int64) if frozen else start_levels(a, j, dt, eta, min_level, L, stats, margins)
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
            bp, vp = b.copy(), v.copy()
            bp[:, :3] = rnd(b[:, :3] + h * (v[:, :3] + h / 2 * (a + h / 3 * j)))
            vp[:, :3] = rnd(v[:, :3] + h * (a + h / 2 * j))
            a1, j1 = [rnd(z) for z in fj_ref(bp, vp, G, eps2, act)]
            h = (s[act] * tick)[:, None]
            a0, j0 = a[act], j[act]
            v1 = v[act, :3] + h / 2 * (a0 + a1) + h * h / 12 * (j0 - j1)
            b[act, :3] = rnd(b[act, :3] + h / 2 * (v[act, :3] + v1) + h * h / 12 * (a0 - a1))
            v[act, :3], a[act], j[act] = rnd(v1), a1, j1
            if not frozen:
                a2 = (-6 * (a0 - a1) - h * (4 * j0 + 2 * j1)) / h ** 2
                a3 = (12 * (a0 - a1) + 6 * h * (j0 + j1)) / h ** 3
                a2e = a2 + h * a3
                num = eta * (_norm(a1) * _norm(a2e) + _norm(j1) ** 2)
                den = _norm(j1) * _norm(a3) + _norm(a2e) ** 2
                for k, i in enumerate(act):
                    tau = np.inf if den[k] == 0 else np.sqrt(num[k] / den[k])
                    want = level_for(tau, dt, min_level, L, stats, margins)
                    if want >= lev[i]:
                        lev[i] = want
                    elif t_next % (2 * s[i]) == 0:
                        lev[i] -= 1
            t[act] = t_next
            stats["block_steps"] += 1
            stats["body_steps"] += len(act)
            stats["finest_level"] = max(stats["finest_level"], int(lev.max()))
            if t_next == 2 ** L:
                break
        stats["outer_steps"] += 1
    return b, v, a, j, lev.astype(np.uint8), stats


def tight_pair(b, v):
    """Bodies 0 and 1 at their common centre +- (0.02, 0, 0) with velocities +- (0, w, 0) about their mean velocity,
    w = sqrt((m0 + m1) / 0.04) / 2; the arrays rounded to float32."""
    b, v = np.array(b, np.float64), np.array(v, np.float64)
    c, u = 0.5 * (b[0, :3] + b[1, :3]), 0.5 * (v[0, :3] + v[1, :3])
    w = np.sqrt((b[0, 3] + b[1, 3]) / 0.04) / 2
    b[0, :3], b[1, :3] = c + (0.02, 0, 0), c - (0.02, 0, 0)
    v[0, :3], v[1, :3] = u + (0, w, 0), u - (0, w, 0)
    return b.astype(np.float32), v.astype(np.float32)


def kepler(e=0.9):
    """Masses 0.6 / 0.4, relative orbit a = 1, eccentricity e, from pericentre, G = 1: period 2 pi."""
    m1, m2 = 0.6, 0.4
    r, w = 1.0 - e, np.sqrt((1.0 + e) / (1.0 - e))
    b = np.array([[-m2 * r, 0, 0, m1], [m1 * r, 0, 0, m2]], np.float64)
    v = np.array([[0, -m2 * w, 0, 0], [0, m1 * w, 0, 0]], np.float64)
    return b, v


KEPLER = dict(G=1.0, eps2=1e-10, dt=2 * np.pi / 16, outer=16, eta=0.02, max_level=20)

_cache = {}


def kepler_ref():
    """(b0, v0, restatement result, |dE/E|): computed once, shared."""
    if "kepler" not in _cache:
        b0, v0 = kepler()
        k = KEPLER
        out = block_ref(b0, v0, k["G"], k["eps2"], k["dt"], k["outer"], eta=k["eta"], max_level=k["max_level"])
        e0, e1 = energy(b0, v0, 1.0, k["eps2"]), energy(out[0], out[1], 1.0, k["eps2"])
        _cache["kepler"] = (b0, v0, out, abs((e1 - e0) / e0))
    return _cache["kepler"]
