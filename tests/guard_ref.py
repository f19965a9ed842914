"""The numpy restatement of the guarded sums of the mixed-precision force+jerk pass (include/nbody3d_hip.h, "guarded sums";
kernels/guard.hip.h), the barycentre rows of the fixtures' hard pairs, and the record tests/golden/guard.json.  The fixtures, the
per-pair arithmetic and the block-step run are mixed_ref's.  Imported by test_guard_cpu.py, test_guard_gpu.py and
tests/golden/measure_guard.py; not a test module."""
import json
import os

import numpy as np

import block_ref as R
import mixed_ref as M
from block_ref import norm_err
from mixed_ref import F, _fma

GUARD_JSON = os.path.join(M.GOLDEN, "guard.json")
R_NEARS = (0.01, 0.03, 1e3)       # a body has O(1) others inside; a third body enters a near set at 4,099; every term is compensated
STEPS_SIZES = (300, 1025)         # the shared-step record
H = 2.0 ** -7
QUANTITIES = ("pair_a", "pair_j", "bary_a", "bary_j")
_cache = {}


def key(r_near):
    return "guard_%g" % r_near


def fj_guarded(b, v, G, eps2, r_near, rows=None, flush=1024):
    """The guarded mixed pass with block_ref's fj signature.  Per pair mixed_ref.fj_mixed's arithmetic up to s3, dr and t.  A pair
    is near iff binary32 d2 < (float)(r_near * r_near), d2 with eps2 in it.  Far terms: fma into a binary32 register in ascending
    j, flushed into a second one every `flush` pairs (near or far).  Near terms: the rounded products p = s3 dr, p = s3 t into an
    unevaluated binary32 pair (hi, lo) by branch-free TwoSum, never flushed.  The row: (double)far + (double)hi + (double)lo, times
    G.  (One j-chunk, as fj_mixed.)"""
    xh, xl, vf, mf = M.split(b, v)
    n = len(xh)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    e2, m3, r2 = F(eps2), F(-3.0), F(float(r_near) * float(r_near))
    a, j = np.zeros((len(rows), 3)), np.zeros((len(rows), 3))
    for s in range(0, len(rows), 256):
        r = rows[s:s + 256]
        dr = (xh[None, :, :] - xh[r, None, :]) + (xl[None, :, :] - xl[r, None, :])
        dv = vf[None, :, :] - vf[r, None, :]
        d2 = _fma(dr[..., 2], dr[..., 2], _fma(dr[..., 1], dr[..., 1], _fma(dr[..., 0], dr[..., 0], np.broadcast_to(e2, dr.shape[:2]))))
        y = (1.0 / np.sqrt(d2.astype(np.float64))).astype(F)
        sm = mf[None, :] * y
        y2 = y * y
        s3 = sm * y2
        rv = _fma(dr[..., 2], dv[..., 2], _fma(dr[..., 1], dv[..., 1], dr[..., 0] * dv[..., 0]))
        q3 = (rv * y2) * m3
        t = _fma(q3[..., None], dr, dv)
        near = d2 < r2
        some = near.any(0)
        zero = F(0)
        reg, REG = np.zeros((len(r), 6), F), np.zeros((len(r), 6), F)      # (a, j) far sums: the register and the chunk's
        hi, lo = np.zeros((len(r), 6), F), np.zeros((len(r), 6), F)
        for jj in range(n):
            term = np.concatenate([dr[:, jj, :], t[:, jj, :]], axis=1)
            w = s3[:, jj, None]
            if some[jj]:
                nr = near[:, jj, None]
                reg = _fma(np.where(nr, zero, w), term, reg)
                p = np.where(nr, w, zero) * term
                sm_ = hi + p
                bb = sm_ - hi
                e = (hi - (sm_ - bb)) + (p - bb)
                hi, lo = sm_, lo + e
            else:
                reg = _fma(w, term, reg)
            if jj % flush == flush - 1:
                REG, reg = REG + reg, np.zeros_like(reg)
        tot = ((REG + reg).astype(np.float64) + hi.astype(np.float64)) + lo.astype(np.float64)
        a[s:s + 256], j[s:s + 256] = G * tot[:, :3], G * tot[:, 3:]
    return a, j


def with_guard(r_near):
    return lambda b, v, G, eps2, rows=None: fj_guarded(b, v, G, eps2, r_near, rows)


def bary(a, b):
    """The mass-weighted barycentre row of each pair (2k, 2k + 1), k < PAIRS, of the per-body rows a: what acts on the pair as a
    whole (the partner's terms cancel)."""
    a, m = np.asarray(a, np.float64)[:2 * M.PAIRS, :3], np.asarray(b, np.float64)[:2 * M.PAIRS, 3]
    return (m[0::2, None] * a[0::2] + m[1::2, None] * a[1::2]) / (m[0::2] + m[1::2])[:, None]


def bary_err(got, ref, b):
    """The worst error of the pairs' barycentre rows, relative to the row's own |ref|."""
    g, r = bary(got, b), bary(ref, b)
    return float((np.sqrt(((g - r) ** 2).sum(1)) / np.sqrt((r * r).sum(1))).max())


def four(a, j, ra, rj, b):
    """pair_a, pair_j, bary_a, bary_j of (a, j) against (ra, rj); (a, j) may hold the pair members' rows only."""
    rows = np.arange(2 * M.PAIRS)
    return dict(pair_a=M.row_err(a, ra, rows), pair_j=M.row_err(j, rj, rows), bary_a=bary_err(a, ra, b), bary_j=bary_err(j, rj, b))


def measure_pass(kind, n):
    """The record of one hard pass case: the four figures for the guarded restatement at every R_NEARS and for fj_mixed's binary32
    and fp64 sums, all against fj_ref, on the pair members' rows."""
    b, v, ra, rj = M.pass_ref(kind, n)
    rows = M.pair_rows(kind)
    rec = dict(kind=kind, n=n, eps2=M.KINDS[kind])
    for r_near in R_NEARS:
        rec[key(r_near)] = four(*fj_guarded(b, v, 1.0, M.KINDS[kind], r_near, rows), ra, rj, b)
    for acc in ("f32", "fp64"):
        rec[acc] = four(*M.fj_mixed(b, v, 1.0, M.KINDS[kind], rows, acc=acc), ra, rj, b)
    return rec


def measure_plummer(n):
    b, v, ra, rj = M.pass_ref("plummer", n)
    a, j = fj_guarded(b, v, 1.0, M.KINDS["plummer"], R_NEARS[0])
    return dict(n=n, r_near=R_NEARS[0], a=norm_err(a, ra), j=norm_err(j, rj))


def hermite_guarded(b, v, G, eps2, h, steps, fj):
    """mixed_ref.hermite_mixed with the direct sum as an argument."""
    b, v = np.array(b, np.float64), np.array(v, np.float64)
    a, j = fj(b, v, G, eps2)
    for _ in range(steps):
        bp, vp = b.copy(), v.copy()
        bp[:, :3] = b[:, :3] + h * v[:, :3] + h * h / 2 * a + h ** 3 / 6 * j
        vp[:, :3] = v[:, :3] + h * a + h * h / 2 * j
        a1, j1 = fj(bp, vp, G, eps2)
        v1 = v[:, :3] + h / 2 * (a + a1) + h * h / 12 * (j - j1)
        b[:, :3] = b[:, :3] + h / 2 * (v[:, :3] + v1) + h * h / 12 * (a - a1)
        v[:, :3], a, j = v1, a1, j1
    return b, v, a, j


def steps_ref(n):
    """(b0, v0, five shared steps of the fp64 scheme, block_ref.hermite_ref): once per size, shared, never written."""
    if ("steps", n) not in _cache:
        b0, v0 = M.pass_system("hard", n)
        _cache["steps", n] = (b0, v0, R.hermite_ref(b0, v0, 1.0, 1e-8, H, 5))
    return _cache["steps", n]


def measure_steps(n):
    """The distance of five shared steps of the restatement with the guarded sum at R_NEARS[0] from the fp64 scheme's: what the
    binary32 pair arithmetic and the guarded sums leave on the state."""
    b0, v0, d = steps_ref(n)
    g = hermite_guarded(b0, v0, 1.0, 1e-8, H, 5, with_guard(R_NEARS[0]))
    return dict(n=n, r_near=R_NEARS[0], x=norm_err(g[0][:, :3], d[0][:, :3]), v=norm_err(g[1][:, :3], d[1][:, :3]))


def record():
    if "record" not in _cache:
        with open(GUARD_JSON) as f:
            _cache["record"] = json.load(f)
    return _cache["record"]


def pass_record(kind, n):
    return next(r for r in record()["pass"] if r["kind"] == kind and r["n"] == n)
