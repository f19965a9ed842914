"""The fp64 numpy restatement of the block-time-step Hermite scheme (include/nbody3d_hip.h, "block individual time steps"), next
to a copy of the force+jerk direct sum, the systems the block-step tests share, the decision log of the restatement, and the
inputs and measurements of the decision audit (tests/golden/block_decisions.json).  Imported by test_block_cpu.py,
test_block_gpu.py, test_block_decisions_gpu.py, test_block_node.py and tests/golden/measure_block_decisions.py; not a test
module."""
import json
import os

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


def levels_for(tau, dt, lmin, L):
    """level_for over an array: (want, clamped, margin); margin is inf where tau is not finite."""
    tau = np.asarray(tau, np.float64)
    want, hit, margin = np.full(tau.shape, L, np.int64), np.zeros(tau.shape, bool), np.full(tau.shape, np.inf)
    with np.errstate(invalid="ignore"):
        for l in range(L, lmin - 1, -1):
            ok = dt / 2.0 ** l <= tau
            want[ok] = l
            hit |= ok
            margin = np.fmin(margin, np.abs(tau / (dt / 2.0 ** l) - 1.0))
    margin[~np.isfinite(tau)] = np.inf
    return want, ~hit, margin


def start_levels(a, j, dt, eta, lmin, L, stats, margins=None, log=None):
    """The start rule: level_for((eta / 2) |a| / |j|), |j| = 0: lmin.  log: a list that gets one {"kind": "start", ...} entry."""
    na, nj = _norm(np.asarray(a, np.float64)), _norm(np.asarray(j, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = np.where(nj == 0, np.inf, 0.5 * eta * na / nj)
    want, clamped, margin = levels_for(tau, dt, lmin, L)
    want[nj == 0], clamped[nj == 0], margin[nj == 0] = lmin, False, np.inf
    stats["clamped"] += int(clamped.sum())
    if margins is not None:
        margins.extend(margin[np.isfinite(margin)])
    if log is not None:
        log.append(dict(kind="start", act=np.arange(len(na)), tau=tau, want=want.copy(), after=want.copy(), clamped=clamped, margin=margin))
    return want


def correct(x0, v0, a0, j0, a1, j1, h):
    """The Hermite corrector over h (a scalar or one value per row), rows of three components, fp64, nothing rounded: (x1, v1)."""
    x0, v0, a0, j0, a1, j1 = [np.asarray(z, np.float64)[:, :3] for z in (x0, v0, a0, j0, a1, j1)]
    h = np.asarray(h, np.float64).reshape(-1, 1)
    v1 = v0 + h / 2 * (a0 + a1) + h * h / 12 * (j0 - j1)
    return x0 + h / 2 * (v0 + v1) + h * h / 12 * (a0 - a1), v1


def tau_of(a0, j0, a1, j1, h, eta, dtype=np.float64, regroup=False):
    """The step criterion's tau per row, evaluated in `dtype`; regroup: the same quantity with a2e taken as one expression,
    a2e = (6 (a0 - a1) + h (2 j0 + 4 j1)) / h^2 (for the evaluation spread of the decision audit)."""
    a0, j0, a1, j1 = [np.asarray(z, np.float64)[:, :3].astype(dtype) for z in (a0, j0, a1, j1)]
    h, eta = np.asarray(h, np.float64).reshape(-1, 1).astype(dtype), dtype(eta)
    a3 = (12 * (a0 - a1) + 6 * h * (j0 + j1)) / h ** 3
    if regroup:
        a2e = (6 * (a0 - a1) + h * (2 * j0 + 4 * j1)) / h ** 2
    else:
        a2 = (-6 * (a0 - a1) - h * (4 * j0 + 2 * j1)) / h ** 2
        a2e = a2 + h * a3
    num = eta * (_norm(a1) * _norm(a2e) + _norm(j1) ** 2)
    den = _norm(j1) * _norm(a3) + _norm(a2e) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den == 0, np.inf, np.sqrt(num / den))


def decide(a0, j0, a1, j1, h, level, t_next, dt, eta, lmin, L):
    """The step criterion and the level rule for rows stepped over h from `level` (a scalar or one per row) to the tick t_next:
    a dict of tau, want, after, aligned (t_next is a multiple of the doubled step), clamped and margin, one value per row."""
    tau = tau_of(a0, j0, a1, j1, h, eta)
    level = np.broadcast_to(np.asarray(level, np.int64), tau.shape)
    want, clamped, margin = levels_for(tau, dt, lmin, L)
    aligned = t_next % (2 * 2 ** (L - level)) == 0
    after = np.where(want >= level, want, np.where(aligned, level - 1, level))
    return dict(tau=tau, want=want, after=after, aligned=aligned, clamped=clamped, margin=margin)


def block_ref(b, v, G, eps2, dt, outer, eta=0.02, max_level=20, min_level=0, levels=None, frozen=False, aj=None, margins=None,
              store=np.float64, log=None, fj=None, noise=None):
    """`outer` outer steps of dt with block individual time steps.  levels: initial levels (None: the start rule, or min_level
    everywhere when frozen); aj: derivatives carried over (None: evaluated); store: the precision (a1, j1) and the state are
    rounded to when stored.  log: a list that gets the decision log (see replay_log): an entry for the start rule where it ran,
    then one per block step.  fj: the direct sum to use in place of fj_ref (fj_torch).  noise: (relative size, generator) --
    every (a1, j1) of a block step is moved by uniform noise of that share of the system's max |a| and max |j| (the flip-safe margin of the
    decision audit).  Returns (b, v, a, j, levels, stats)."""
    rnd = lambda z: np.asarray(z, store).astype(np.float64)
    fj = fj_ref if fj is None else fj
    b, v = np.array(b, np.float64), np.array(v, np.float64)
    n, L = len(b), max_level
    a, j = [rnd(z) for z in (fj(b, v, G, eps2) if aj is None else aj)]
    a, j = np.array(a[:, :3]), np.array(j[:, :3])
    stats = {"outer_steps": 0, "block_steps": 0, "body_steps": 0, "clamped": 0, "finest_level": 0}
    if levels is None:
        lev = np.full(n, min_level, np.int64) if frozen else start_levels(a, j, dt, eta, min_level, L, stats, margins, log)
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
            a1, j1 = fj(bp, vp, G, eps2, act)
            if noise is not None:
                a1 = a1 + noise[0] * np.abs(a).max() * noise[1].uniform(-1, 1, a1.shape)
                j1 = j1 + noise[0] * np.abs(j).max() * noise[1].uniform(-1, 1, j1.shape)
            a1, j1 = rnd(a1), rnd(j1)
            h = (s[act] * tick)[:, None]
            a0, j0 = a[act], j[act]
            x1, v1 = correct(b[act], v[act], a0, j0, a1, j1, h)
            b[act, :3] = rnd(x1)
            v[act, :3], a[act], j[act] = rnd(v1), a1, j1
            entry = dict(kind="step", t_next=t_next, act=act, before=lev[act].copy())
            if not frozen:
                d = decide(a0, j0, a1, j1, h, lev[act], t_next, dt, eta, min_level, L)
                lev[act] = d["after"]
                stats["clamped"] += int(d["clamped"].sum())
                if margins is not None:
                    margins.extend(d["margin"][np.isfinite(d["margin"])])
                entry.update(d)
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
    return b, v, a, j, lev.astype(np.uint8), stats


def fj_torch(b, v, G, eps2, rows=None):
    """fj_ref's direct sum with torch on the CPU in fp64 (several threads); for the 4k systems of the decision audit."""
    import torch
    t = lambda z: torch.from_numpy(np.ascontiguousarray(np.asarray(z, np.float64)))
    x, m, u = t(b)[:, :3], t(b)[:, 3], t(v)[:, :3]
    rows = np.arange(len(x)) if rows is None else np.asarray(rows)
    a, j = torch.zeros((len(rows), 3), dtype=torch.float64), torch.zeros((len(rows), 3), dtype=torch.float64)
    for s in range(0, len(rows), 256):
        r = torch.from_numpy(rows[s:s + 256].astype(np.int64))
        dr, dv = x[None, :, :] - x[r][:, None, :], u[None, :, :] - u[r][:, None, :]
        y2 = 1.0 / ((dr * dr).sum(2) + eps2)
        s3 = m[None, :] * y2 * torch.sqrt(y2)
        q = (dr * dv).sum(2) * y2
        a[s:s + 256] = G * (s3[:, :, None] * dr).sum(1)
        j[s:s + 256] = G * (s3[:, :, None] * (dv - 3.0 * q[:, :, None] * dr)).sum(1)
    return a.numpy(), j.numpy()


# ---- the decision log ------------------------------------------------------------------------------------------------------
def replay_log(log, n, L, levels=None, check=False):
    """Levels and stats from the log alone: every entry sets the levels of its bodies to `after` and, a block step, their time to
    t_next.  levels: the initial levels where the log has no start entry.  check: also assert that every block step is the one
    the levels and times before it ask for (t_next = min t_i + s_i, the active set exactly the bodies due then, in ascending
    order)."""
    lev = np.zeros(n, np.int64) if levels is None else np.array(levels, np.int64)
    t = np.zeros(n, np.int64)
    stats = {"outer_steps": 0, "block_steps": 0, "body_steps": 0, "clamped": 0, "finest_level": 0}
    for k, e in enumerate(log):
        if e["kind"] == "step":
            if check:
                due = t + 2 ** (L - lev)
                assert e["t_next"] == due.min() and np.array_equal(e["act"], np.nonzero(due == e["t_next"])[0]), k
                assert np.array_equal(e["before"], lev[e["act"]]), k
            t[e["act"]] = e["t_next"]
            stats["block_steps"] += 1
            stats["body_steps"] += len(e["act"])
            if e["t_next"] == 2 ** L:
                t[:] = 0
                stats["outer_steps"] += 1
        lev[e["act"]] = e["after"]
        stats["clamped"] += int(np.sum(e.get("clamped", 0)))
        stats["finest_level"] = max(stats["finest_level"], int(lev.max()))
    if levels is not None:
        stats["finest_level"] = max(stats["finest_level"], int(np.max(levels)))
    return lev.astype(np.uint8), stats


def log_min_margins(log, n):
    """Each body's smallest margin over all its decisions (inf: none with a finite tau)."""
    m = np.full(n, np.inf)
    for e in log:
        if "margin" in e:
            np.minimum.at(m, e["act"], e["margin"])
    return m


def log_active_sizes(log):
    return np.array([len(e["act"]) for e in log if e["kind"] == "step"], np.int64)


def log_kinds(log):
    """Counts of the block steps' decisions by kind: deepened by one level, by more than one, coarsened, wanted to coarsen at a time
    that is no multiple of the doubled step."""
    k = {"deepened_one": 0, "deepened_more": 0, "coarsened": 0, "coarsen_unaligned": 0, "kept": 0}
    for e in log:
        if e["kind"] == "step" and "want" in e:
            d = e["after"] - e["before"]
            k["deepened_one"] += int((d == 1).sum())
            k["deepened_more"] += int((d > 1).sum())
            k["coarsened"] += int((d < 0).sum())
            k["coarsen_unaligned"] += int(((e["want"] < e["before"]) & ~e["aligned"]).sum())
            k["kept"] += int((e["want"] == e["before"]).sum())
    return k


def first_divergence(log, levels):
    """For final levels that differ from the log's: the earliest block step that holds the LAST logged decision of such a body
    -- the levels cannot have followed the log beyond it -- as text; None where the levels agree."""
    n = len(levels)
    want, _ = replay_log(log, n, 0)
    bad = np.nonzero(want != np.asarray(levels))[0]
    if not len(bad):
        return None
    last, step = {}, -1
    for e in log:
        step += e["kind"] == "step"
        for i in e["act"][np.isin(e["act"], bad)]:
            last[int(i)] = (step, e)
    first = min(s for s, _ in last.values())
    e = next(e for s, e in last.values() if s == first)
    lines = ["%d bodies differ; the log cannot be followed past block step %d (t_next %s, |A| %d)"
             % (len(bad), first, e.get("t_next", "start"), len(e["act"]))]
    for i in bad[:16]:
        s, e = last[int(i)]
        q = int(np.nonzero(e["act"] == i)[0][0])
        lines.append("  body %d: engine level %d, log %d; last decision in block step %d: before %s want %d aligned %s margin %.3g"
                     % (i, levels[i], want[i], s, e["before"][q] if "before" in e else "-", e["want"][q],
                        e["aligned"][q] if "aligned" in e else "-", e["margin"][q]))
    return "\n".join(lines)


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


# ---- the decision audit (test_block_decisions_gpu.py; measured by tests/golden/measure_block_decisions.py) -------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DECISIONS_JSON = os.path.join(GOLDEN, "block_decisions.json")
ETA = 0.02
NOISE = 1e-12                     # the project's fp64 bound on a and j (norm_err), as noise on every (a1, j1)
NOISE_SEEDS = (1, 2, 3)
FACTOR = 8                        # every tolerance taken from a measured number is this many times the number
EXCLUDED_CAP = 0.005              # the largest share of one run's decisions that may sit inside the exclusion margin
BUCKETS = ((1, 63), (64, 512), (513, 1024), (1025, 2048), (2049, None))      # |A|; None: n - 1 (|A| = n is counted as "all")
# part A: n -> the schedule's parameters (chosen on the restatement alone, see schedule_conditions); the scheduler's segments are
# 256 bodies per wave up to 4,096 and 512 above: 1025 and 1026 end in a wave of one and two bodies, 3841 fills all 16 waves and ends
# in one body, 4099 has nine waves of 512, the last of three bodies
SCHEDULES = {1025: dict(seed=21, dt_log2=-5, max_level=10, outer=3), 1026: dict(seed=22, dt_log2=-5, max_level=12, outer=1),
             3841: dict(seed=21, dt_log2=-5, max_level=12, outer=1), 4099: dict(seed=22, dt_log2=-5, max_level=12, outer=1)}
STORED = (3841, 4099)             # expected levels and a sample of the expected state are fixtures; the others are computed live
SAMPLE = 256
# part B: one block step of every body from level 0, and the start rule (dt_log2, max_level, min_level)
STEP_SIZES, STEP_SEED = (1025, 4099), 21
STEP_RUNS = ((-3, 12), (-5, 12), (-7, 12), (-3, 4))                                # (dt_log2, max_level); the last one: clamped decisions
START_RUNS = ((-3, 12, 0), (-5, 12, 0), (-7, 12, 0), (-3, 12, 2), (-3, 3, 0))      # the last one: clamped decisions
ZERO_JERK = (3, 100, -1)          # bodies whose uploaded jerk is zeroed: the |j| = 0 -> min_level branch


def direct_sum(n):
    return fj_torch if n > 2048 else fj_ref


def audit_system(n, seed):
    from nbody3d_amd import ic
    return tight_pair(*ic.plummer(n, seed=seed))


def run_schedule(n, noise_seed=None):
    """The restatement of part A's input n, outer step by outer step (each continues from everything the one before left): the list
    of (b, v, a, j, levels, cumulative stats) after every outer step, and the log of all of them."""
    p = SCHEDULES[n]
    b, v = audit_system(n, p["seed"])
    noise = None if noise_seed is None else (NOISE, np.random.default_rng(noise_seed))
    outs, log, lev, aj, total = [], [], None, None, None
    for _ in range(p["outer"]):
        b, v, a, j, lev, st = block_ref(b, v, 1.0, EPS2, 2.0 ** p["dt_log2"], 1, eta=ETA, max_level=p["max_level"], levels=lev, aj=aj,
                                       log=log, fj=direct_sum(n), noise=noise)
        aj = (a, j)
        total = st if total is None else {k: max(total[k], st[k]) if k == "finest_level" else total[k] + st[k] for k in st}
        outs.append((b, v, a, j, lev, dict(total)))
    return outs, log


def sample_rows(n):
    """The rows whose expected state is stored: the pair, the last wave's bodies, and an even stride over the rest."""
    return np.unique(np.concatenate([np.arange(4), np.arange(n - 4, n), np.linspace(0, n - 1, SAMPLE - 8).astype(np.int64)]))


def bucket_counts(sizes, n):
    out = {"%d-%s" % (lo, hi if hi else "n-1"): int(((sizes >= lo) & (sizes <= (hi if hi else n - 1)) & (sizes < n)).sum()) for lo, hi in BUCKETS}
    out["all"] = int((sizes == n).sum())
    return out


def measure_schedule(n, noise_seeds=NOISE_SEEDS):
    """The record of part A's input n, the final levels and the state of the sampled rows (the stored sizes' fixtures)."""
    p = SCHEDULES[n]
    outs, log = run_schedule(n)
    rb, lev, stats = outs[-1][0], outs[-1][4], outs[-1][5]
    mm = log_min_margins(log, n)
    flip, dev, flipped = 0.0, 0.0, 0
    for seed in noise_seeds:
        nb, _, _, _, nlev, _ = run_schedule(n, seed)[0][-1]
        changed = nlev != lev
        flipped += int(changed.sum())
        flip = max(flip, float(mm[changed].max()) if changed.any() else 0.0)
        dev = max(dev, norm_err(nb[:, :3], rb[:, :3]))
    rec = dict(n=n, eta=ETA, **p, stats=[o[5] for o in outs], levels=np.bincount(lev, minlength=p["max_level"] + 1).tolist(),
               active_sizes=bucket_counts(log_active_sizes(log), n), kinds=log_kinds(log), min_margin=float(mm.min()),
               noise=NOISE, noise_seeds=list(noise_seeds), noise_flipped=flipped, flip_safe_margin=flip, noise_position_dev=dev)
    rows = sample_rows(n)
    state = np.concatenate([rows[:, None].astype(np.float64)] + [outs[-1][k][rows, :3] for k in range(4)], axis=1)
    return rec, lev, state


def schedule_conditions(rec):
    """What part A asks of an input, on its record (the restatement alone)."""
    n, act, kinds = rec["n"], rec["active_sizes"], rec["kinds"]
    assert sum(c >= 16 for c in rec["levels"]) >= 5, rec["levels"]
    assert act["1-63"] and act["64-512"] and act["513-1024"] and act["all"] + act["1025-2048"] + act["2049-n-1"], act
    assert n < 2048 or act["2049-n-1"], act
    assert all(kinds[k] >= 1 for k in ("deepened_one", "deepened_more", "coarsened", "coarsen_unaligned")), kinds
    assert rec["stats"][-1]["clamped"] == 0, rec["stats"]
    assert rec["min_margin"] >= FACTOR * rec["flip_safe_margin"], (rec["min_margin"], rec["flip_safe_margin"])


def step_inputs(n, prec):
    """Part B's system in the handle's precision: (b0, v0, a0, j0), a0 and j0 the fp64 direct sum rounded to it (w = 0), the jerk
    rows of ZERO_JERK zeroed."""
    dtype = np.float32 if prec == "f32" else np.float64
    b0, v0 = audit_system(n, STEP_SEED)
    a, j = direct_sum(n)(b0, v0, 1.0, EPS2)
    a0, j0 = np.zeros((n, 4), dtype), np.zeros((n, 4), dtype)
    a0[:, :3], j0[:, :3] = a, j
    j0[list(ZERO_JERK)] = 0
    return b0.astype(dtype), v0.astype(dtype), a0, j0


def emulate_step(n, prec, dt):
    """One block step of h = dt of every body, by the restatement's arithmetic with a direct sum in fp64: (a1, j1) as the handle
    would store them (its own differ by its force error; the audit takes the handle's)."""
    dtype = np.float32 if prec == "f32" else np.float64
    rnd = lambda z: np.asarray(z, dtype).astype(np.float64)
    b0, v0, a0, j0 = [z.astype(np.float64) for z in step_inputs(n, prec)]
    bp, vp = b0.copy(), v0.copy()
    bp[:, :3] = rnd(b0[:, :3] + dt * (v0[:, :3] + dt / 2 * (a0[:, :3] + dt / 3 * j0[:, :3])))
    vp[:, :3] = rnd(v0[:, :3] + dt * (a0[:, :3] + dt / 2 * j0[:, :3]))
    a1, j1 = [rnd(z) for z in direct_sum(n)(bp, vp, 1.0, EPS2)]
    return a0, j0, a1, j1


def tau_spread(a0, j0, a1, j1, h, eta):
    """The largest relative difference, over the rows, between tau as decide() evaluates it and two other host evaluations of
    the same inputs: in np.longdouble, and in fp64 with a2e as one expression."""
    ref = tau_of(a0, j0, a1, j1, h, eta, np.longdouble)
    ok = np.isfinite(ref) & (ref > 0)
    return max(float(np.max(np.abs(tau_of(a0, j0, a1, j1, h, eta, regroup=g)[ok] / ref[ok] - 1))) for g in (False, True))


def start_tau_spread(a, j, eta):
    """tau_spread for the start rule's tau = (eta / 2) |a| / |j|."""
    t = lambda d: 0.5 * d(eta) * _norm(a[:, :3].astype(d)) / _norm(j[:, :3].astype(d))
    with np.errstate(divide="ignore", invalid="ignore"):
        t64, tl = t(np.float64), t(np.longdouble)
    ok = np.isfinite(tl) & (tl > 0)
    return float(np.max(np.abs(t64[ok] / tl[ok] - 1)))


def measure_step(n, prec):
    """The record of part B's input (n, prec): per dt the evaluation spread of tau on the emulated step and the smallest margins."""
    a0, j0 = step_inputs(n, prec)[2:]
    rec = dict(n=n, precision=prec, seed=STEP_SEED, eta=ETA, start_tau_spread=start_tau_spread(a0, j0, ETA), steps=[])
    for l2, L in STEP_RUNS:
        dt = 2.0 ** l2
        e = emulate_step(n, prec, dt)
        d = decide(*e, dt, 0, 2 ** L, dt, ETA, 0, L)
        rec["steps"].append(dict(dt_log2=l2, max_level=L, tau_spread=tau_spread(*e, dt, ETA), min_margin=float(d["margin"].min()),
                                 levels=np.bincount(d["after"], minlength=L + 1).tolist(), clamped=int(d["clamped"].sum())))
    return rec


def exclusion_margin(steps):
    """FACTOR x the largest evaluation spread of tau over part B's inputs: decisions closer to a level boundary are left out."""
    return FACTOR * max(max([s["start_tau_spread"]] + [x["tau_spread"] for x in s["steps"]]) for s in steps)


def decisions_record():
    if "decisions" not in _cache:
        with open(DECISIONS_JSON) as f:
            _cache["decisions"] = json.load(f)
    return _cache["decisions"]


def fixture_paths(n):
    return [os.path.join(GOLDEN, "block_decisions_n%d_%s.npy" % (n, k)) for k in ("levels", "state")]


# part B, the level rule alone: G = 0 and (a0, j0) = 0 make every (a1, j1) exactly zero in either precision, so tau is inf and want is
# min_level at every decision, whatever the force kernel does -- the schedule from mixed uploaded levels is then integer logic: a
# body at level l steps once unaligned (kept), then coarsens by ONE level at every further step down to min_level
FREE_RUNS = ((6, 0), (5, 1))      # (max_level, min_level)
FREE_DT_LOG2, FREE_SEED = -5, 5


def free_levels(n, L, lmin):
    return np.random.default_rng(FREE_SEED).integers(lmin, L + 1, n).astype(np.uint8)


def free_schedule(n, prec, L, lmin, log=None):
    """The restatement of one outer step of free motion from free_levels: (b, v, a, j, levels, stats)."""
    dtype = np.float32 if prec == "f32" else np.float64
    b0, v0 = audit_system(n, STEP_SEED)
    zero = np.zeros((n, 3))
    return block_ref(b0, v0, 0.0, EPS2, 2.0 ** FREE_DT_LOG2, 1, eta=ETA, max_level=L, min_level=lmin, levels=free_levels(n, L, lmin),
                     aj=(zero, zero), store=dtype, log=log, fj=direct_sum(n))
