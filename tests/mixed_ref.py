"""The numpy restatement of the mixed-precision force+jerk pass (include/nbody3d_hip.h, "the force+jerk pass of an NB_F64 Hermite
handle in mixed precision"; kernels/mixed.hip.h), the fixtures with hard pairs that are NOT rounded to float32, the shared-step loop
on it, and the record tests/golden/mixed.json.  Imported by test_mixed_cpu.py, test_mixed_gpu.py and tests/golden/measure_mixed.py;
not a test module."""
import json
import os

import numpy as np

import block_ref as R
from block_ref import fj_ref, norm_err

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MIXED_JSON = os.path.join(GOLDEN, "mixed.json")
F = np.float32
FACTOR = 8                        # a GPU bound taken from a recorded figure is this many times the figure
ACCS = ("fp64", "f32", "f32rev", "f32pair")


def _fma(a, b, c):
    """binary32 fused multiply-add: the product of two binary32 numbers is exact in binary64; one rounding to binary64 in between
    is the only difference from the hardware's single rounding (rare, half an ulp of binary64)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def split(b, v, lo=True):
    """The four binary32 streams of the pass, from fp64 rows: xh, xl (zeros with lo=False), vf, mf."""
    x, m, u = np.asarray(b, np.float64)[:, :3], np.asarray(b, np.float64)[:, 3], np.asarray(v, np.float64)[:, :3]
    xh = x.astype(F)
    xl = (x - xh.astype(np.float64)).astype(F) if lo else np.zeros_like(xh)
    return xh, xl, u.astype(F), m.astype(F)


def fj_mixed(b, v, G, eps2, rows=None, lo=True, acc="f32", flush=1024):
    """The mixed pass with block_ref's fj signature: (a, j) of `rows` as float64.  Per pair, all binary32:
    dr = (xh_j - xh_i) + (xl_j - xl_i), dv = vf_j - vf_i, rho^2 by three fma from eps2, y = rsq, s3 = (m y) y^2, q = (dr.dv) y^2,
    t = dv - 3 q dr, a += s3 dr, j += s3 t.  lo=False drops the lo word.  acc: "fp64" -- the pair terms s3 dr, s3 t summed in
    binary64; "f32" -- the kernel's sums: fma into a binary32 register in ascending j, flushed into a second binary32 register
    every `flush` terms; "f32rev" -- the same in descending j; "f32pair" -- numpy's pairwise binary32 sum of the rounded terms.  (The
    engine adds its j-chunks in fp64: the restatement is one chunk.)"""
    assert acc in ACCS, acc
    xh, xl, vf, mf = split(b, v, lo)
    n = len(xh)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    e2, m3 = F(eps2), F(-3.0)
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
        if acc == "fp64":
            sa = (s3.astype(np.float64)[..., None] * dr.astype(np.float64)).sum(1)
            sj = (s3.astype(np.float64)[..., None] * t.astype(np.float64)).sum(1)
        elif acc == "f32pair":
            sa = (s3[..., None] * dr).sum(1, dtype=F).astype(np.float64)
            sj = (s3[..., None] * t).sum(1, dtype=F).astype(np.float64)
        else:
            order = range(n) if acc == "f32" else range(n - 1, -1, -1)
            ra, rj, RA, RJ = [np.zeros((len(r), 3), F) for _ in range(4)]
            for k, jj in enumerate(order):
                w = s3[:, jj, None]
                ra, rj = _fma(w, dr[:, jj, :], ra), _fma(w, t[:, jj, :], rj)
                if k % flush == flush - 1:
                    RA, RJ, ra, rj = RA + ra, RJ + rj, np.zeros_like(ra), np.zeros_like(rj)
            sa, sj = (RA + ra).astype(np.float64), (RJ + rj).astype(np.float64)
        a[s:s + 256], j[s:s + 256] = G * sa, G * sj
    return a, j


def hard(n, seed, pairs, half, shift=None):
    """A Plummer sphere whose bodies (2k, 2k + 1), k < pairs, are re-placed at a separation of 2 half about their centre of mass
    (+- half for equal masses) on the circular orbit about it, in float64 and NOT rounded to float32 (their lo words are not zero);
    shift: a constant vector added to every position (every lo word is then non-zero and |x| >> the separation)."""
    from nbody3d_amd import ic
    b, v = [np.array(z, np.float64) for z in ic.plummer(n, seed=seed)]
    for k in range(pairs):
        p, q = 2 * k, 2 * k + 1
        M = b[p, 3] + b[q, 3]
        c = (b[p, 3] * b[p, :3] + b[q, 3] * b[q, :3]) / M
        u = (b[p, 3] * v[p, :3] + b[q, 3] * v[q, :3]) / M
        d, w = 2.0 * half, np.sqrt(M / (2.0 * half))
        b[p, :3], b[q, :3] = c + (d * b[q, 3] / M, 0, 0), c - (d * b[p, 3] / M, 0, 0)
        v[p, :3], v[q, :3] = u + (0, w * b[q, 3] / M, 0), u - (0, w * b[p, 3] / M, 0)
    if shift is not None:
        b[:, :3] += np.asarray(shift, np.float64)
    return b, v


BLOCK = dict(n=512, seed=21, pairs=4, half=1e-3, eps2=1e-8, dt=2 ** -4, max_level=16, eta=0.02, outer=4)

# the pass cases: name -> (fixture, eps2); every one at every size of SIZES
SIZES = (300, 1025, 4099)         # less than one tile; a second workgroup of one row; two j-chunks with ragged last tile and workgroup
PAIRS, HALF, SHIFT, SEED = 16, 1e-3, (3.0, -2.0, 1.0), 21
KINDS = {"plummer": 1e-4, "hard": 1e-8, "hard_shifted": 1e-8, "tight": 1e-8, "tight_shifted": 1e-8}
HALVES = {"hard": HALF, "hard_shifted": HALF, "tight": 1e-4, "tight_shifted": 1e-4}      # half the separation of a kind's pairs
HARD_KINDS = tuple(HALVES)        # the GPU test holds the pair members' rows of every one to FACTOR x the recorded figure
# The inputs on which a lost lo word must miss that bound by a factor of four, on accelerations AND jerks (test_mixed_cpu.py): the
# shifted ones (recorded ratios 98 to 17,660 where 32 is asked).  The unshifted inputs are accuracy cases only: at |x| ~ 0.5 the
# rounded positions are wrong by 3e-5 of a 2e-3 separation, and the binary32 SUMS of the pass itself already leave 1e-6 to 2.6e-6 on
# those pair rows (ratios 21 to 85); on the pairs at +-1e-4 the partner's term is 1.7e7 / n, its register's ulp exceeds most other
# bodies' terms and the field of the rest of the system is largely lost from the sum: 1e-5 of the row (ratios 19 to 177 on a).
DISCRIMINATING = ("hard_shifted", "tight_shifted")
_cache = {}


def pass_system(kind, n):
    if kind == "plummer":
        from nbody3d_amd import ic
        return [np.array(z, np.float64) for z in ic.plummer(n, seed=SEED)]
    return hard(n, SEED, PAIRS, HALVES[kind], SHIFT if kind.endswith("_shifted") else None)


def pair_rows(kind):
    return np.arange(2 * PAIRS) if kind in HARD_KINDS else np.arange(0)


def row_err(got, ref, rows):
    """The worst error over `rows`, relative to the row's own |ref|."""
    d = np.asarray(got, np.float64)[rows, :3] - np.asarray(ref, np.float64)[rows, :3]
    return float((np.sqrt((d * d).sum(1)) / np.sqrt((np.asarray(ref, np.float64)[rows, :3] ** 2).sum(1))).max())


def pass_ref(kind, n):
    """(b, v, fj_ref's (a, j)): computed once per case, shared, never written."""
    key = ("pass", kind, n)
    if key not in _cache:
        b, v = pass_system(kind, n)
        _cache[key] = (b, v) + tuple(R.direct_sum(n)(b, v, 1.0, KINDS[kind]))
    return _cache[key]


def measure_pass(kind, n):
    """The record of one pass case: for lo in (True, False) the restatement's errors against fj_ref -- norm_err of a and j and, on
    the hard inputs, the worst relative error over the pair members' rows."""
    b, v, ra, rj = pass_ref(kind, n)
    rec = dict(kind=kind, n=n, eps2=KINDS[kind])
    for lo in (True, False):
        a, j = fj_mixed(b, v, 1.0, KINDS[kind], lo=lo)
        e = dict(a=norm_err(a, ra), j=norm_err(j, rj))
        if kind in HARD_KINDS:
            e.update(pair_a=row_err(a, ra, pair_rows(kind)), pair_j=row_err(j, rj, pair_rows(kind)))
        rec["lo" if lo else "hi_only"] = e
    return rec


def block_system():
    k = BLOCK
    return hard(k["n"], k["seed"], k["pairs"], k["half"])


def measure_block(fj=None, store=np.float64):
    """One row of BLOCK's table: the restatement's counts and |dE/E0| with `fj` as its direct sum."""
    k = BLOCK
    b0, v0 = [z.astype(store).astype(np.float64) for z in block_system()]      # (a binary32-storing handle rounds what is uploaded)
    b, v, _, _, _, st = R.block_ref(b0, v0, 1.0, k["eps2"], k["dt"], k["outer"], eta=k["eta"], max_level=k["max_level"], fj=fj, store=store)
    e0, e1 = R.energy(b0, v0, 1.0, k["eps2"]), R.energy(b, v, 1.0, k["eps2"])
    return dict(block_steps=st["block_steps"], body_steps=st["body_steps"], clamped=st["clamped"], finest_level=st["finest_level"],
                dE=float(abs((e1 - e0) / e0)))


def with_acc(acc, lo=True):
    return lambda b, v, G, eps2, rows=None: fj_mixed(b, v, G, eps2, rows, lo=lo, acc=acc)


def hermite_mixed(b, v, G, eps2, h, steps, acc="f32"):
    """block_ref.hermite_ref with fj_mixed swapped in: the fp64 state, the predictor rounded to double, the mixed pass on it."""
    fj = with_acc(acc)
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


def record():
    if "record" not in _cache:
        with open(MIXED_JSON) as f:
            _cache["record"] = json.load(f)
    return _cache["record"]


def pass_record(kind, n):
    return next(r for r in record()["pass"] if r["kind"] == kind and r["n"] == n)
