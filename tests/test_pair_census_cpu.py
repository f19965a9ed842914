"""The pair census on the CPU (tests/census_ref.py): its record is what a fresh measurement gives, every input keeps a single pair
visible (min_share >= 8 tol), the hot sets visit every ordered pair once, the reference's own binary32 arithmetic passes -- and a
binary32 direct sum with ONE pair dropped, doubled or taken from the wrong row fails, while the same three mutations pass the suite's
older metric, max |a - ref| < 2e-5 max |ref|, on the Plummer sphere of 20,001 bodies.  No GPU."""
import numpy as np
import pytest

import census_ref as cr
from oracle import oracle
from nbody3d_amd import ic

INPUTS = [("accel", n) for n in sorted(cr.ACCEL_INPUTS)] + [("field_points", n) for n in cr.FIELD_SIZES] + [("diag", n) for n in cr.DIAG_SIZES]
MEASURE = {"accel": cr.measure_accel, "field_points": cr.measure_field, "diag": cr.measure_diag}


@pytest.mark.parametrize("kind,n", INPUTS)
def test_record_is_a_fresh_measurement_and_keeps_every_pair_visible(kind, n):
    """measure_*: the reference's binary32 arithmetic against numpy fp64 on this input.  It passes at the recorded tolerance (the
    tolerance is TOL_FACTOR x its error), the record is what it measures now, and the smallest single share is 8 tolerances or more."""
    fresh, rec = cr._finite(MEASURE[kind](n)), cr.entry(kind, n)
    assert set(fresh) <= set(rec)
    for key, val in fresh.items():
        if key in ("factor", "jerk_factor", "phi_factor", "tol", "jerk_tol", "phi_tol"):
            continue                                             # a raised factor is checked below; tol follows from it
        if isinstance(val, float):
            assert rec[key] == pytest.approx(val, rel=1e-6), key
        else:
            assert rec[key] == val, key
    for pre in ("", "jerk_", "phi_"):
        if pre + "tol" not in rec:
            continue
        ref, factor, tol = rec[pre + "ref_f32_err"], rec[pre + "factor"], rec[pre + "tol"]
        assert tol == pytest.approx(factor * ref, rel=1e-12) and fresh[pre + "ref_f32_err"] <= tol
        share = rec.get(pre + "min_share")                       # (the jerk has none: a jerk term can cancel internally)
        if factor != cr.TOL_FACTOR:
            assert factor > cr.TOL_FACTOR and pre + "device_err" in rec and pre + "why" in rec, "a raised factor records what the device gave and why"
            assert share is None or share >= 4 * tol
        elif pre != "jerk_" and share is not None:
            assert share >= 8 * tol, (kind, n, share, tol)


@pytest.mark.parametrize("n", sorted(cr.ACCEL_INPUTS))
def test_hot_sets_visit_every_ordered_pair_exactly_once(n):
    """Over the K runs every column j is hot exactly once, for every checked row (all rows, or every row of the sample)."""
    K, seeds = cr.ACCEL_INPUTS[n]
    rows = cr.sample_rows(n)
    assert len(rows) == n if n <= cr.FULL_ROWS_MAX else len(rows) == cr.SAMPLE_MAX
    assert len(np.unique(rows)) == len(rows) and rows.min() >= 0 and rows.max() < n and {0, n - 1} <= set(rows.tolist())
    b = cr.bodies(n, seeds[0])
    assert np.all(b[:, 3] > 0) and len(np.unique(b[:, :3], axis=0)) == n
    visits = np.zeros(n, np.int64)
    for k in range(K):
        h = cr.hot(b, K, k)
        ids = np.nonzero(h[:, 3])[0]
        assert np.array_equal(ids, cr.hot_ids(n, K, k)) and np.array_equal(h[:, :3], b[:, :3]) and np.array_equal(h[ids], b[ids])
        visits[ids] += 1
    assert np.all(visits == 1)                 # the same columns for every row: (i <- j) once for every checked i
    if n > cr.FULL_ROWS_MAX:
        for t in range(0, n, 256):
            assert t in rows and min(t + 255, n - 1) in rows


def test_unions_of_two_classes_make_every_unordered_pair_hot_together():
    n = 257
    seen = np.zeros((n, n), np.int64)
    b = cr.bodies(n, 7)
    for a, c in cr.unions():
        ids = np.nonzero(cr.hot_union(b, cr.DIAG_K, a, c)[:, 3])[0]
        seen[np.ix_(ids, ids)] += 1
    i, j = np.triu_indices(n, 1)
    same = i % cr.DIAG_K == j % cr.DIAG_K
    assert np.all(seen[i, j][~same] == 1) and np.all(seen[i, j][same] == cr.DIAG_K) and len(cr.unions()) == 136


def test_packed_oracle_call_is_the_whole_system_sum_bit_for_bit():
    """oracle_rows_f32 hands the oracle the hot rows + zero-mass copies of the targets: the same bits as the whole system."""
    n, K = 1001, 8
    b = cr.bodies(n, 5)
    for k in (0, 5):
        h = cr.hot(b, K, k)
        whole = oracle.accel_f32(h, cr.G, eps2=cr.EPS2)[:, :3]
        assert cr.oracle_rows_f32(h, np.arange(n)).tobytes() == whole.tobytes()
        rows = np.array([0, 5, 13, 1000])
        assert cr.oracle_rows_f32(h, rows).tobytes() == whole[rows].tobytes()


def f32_row(h, i, mutate=None, full=None):
    """Row i of a binary32 direct sum over the hot rows of h, ascending j, with one pair (i <- j) mutated: ("drop", j), ("double", j) or
    ("shift", j): the term computed from row j + 1 of the system `full` (every mass set) instead of row j -- the wrong partner."""
    f = np.float32
    h = np.asarray(h, f)
    q = np.nonzero(h[:, 3])[0]
    q = q[q != i]
    src = h[q].copy()
    weight = np.ones(len(q), f)
    if mutate is not None:
        kind, j = mutate
        at = int(np.nonzero(q == j)[0][0])
        if kind == "drop":
            weight[at] = 0
        elif kind == "double":
            weight[at] = 2
        else:
            j1 = j + 1 if j + 1 < len(h) and j + 1 != i else j - 1
            src[at] = np.asarray(full, f)[j1]
    dr = src[:, :3] - h[i, :3]
    r2 = dr[:, 2] * dr[:, 2] + (dr[:, 1] * dr[:, 1] + (dr[:, 0] * dr[:, 0] + f(cr.EPS2)))
    y = f(1) / np.sqrt(r2)
    t = ((f(cr.G) * src[:, 3]) * (y * y * y) * weight)[:, None] * dr
    return np.cumsum(t, axis=0, dtype=f)[-1]


@pytest.mark.parametrize("n", [1025, 4099, 6143, 12289, 20001])
def test_one_dropped_doubled_or_misattributed_pair_fails_the_census(n):
    """The pair with the SMALLEST share of the whole input: the clean binary32 sum of its row passes, each mutation fails."""
    ref, tol = cr.accel_reference(n), cr.entry("accel", n)["tol"]
    (seed, k), r = min(ref["runs"].items(), key=lambda kv: kv[1]["min_share"])
    at, j = r["argmin"]
    i = int(ref["rows"][at])
    full = cr.bodies(n, seed)
    h = cr.hot(full, ref["K"], k)
    assert j % ref["K"] == k and j != i

    def err(a):
        return float(np.sqrt(((a.astype(np.float64) - r["a"][at]) ** 2).sum()) / r["scale"][at])
    clean = err(f32_row(h, i))
    got = {m: err(f32_row(h, i, (m, j), full)) for m in ("drop", "double", "shift")}
    print("N=%d K=%d: row %d <- %d has share %.3g; clean %.3g, tol %.3g, mutated %s" % (n, ref["K"], i, j, r["min_share"], clean, tol, got))
    assert clean <= tol
    assert all(e > tol for e in got.values()), got
    assert got["drop"] == pytest.approx(r["min_share"], rel=0.05) and got["double"] == pytest.approx(r["min_share"], rel=0.05)


def test_the_same_mutations_pass_the_older_metric_on_the_plummer_sphere():
    """The gap the census closes: on ic.plummer(20001) a pair as large as 5e-6 of the largest acceleration -- the rounding of
    the whole row is smaller -- can be dropped, doubled or taken from the next row, and max |a - ref| < 2e-5 max |ref| still holds."""
    n, TOL_ACC = 20001, 2e-5
    b, _ = ic.plummer(n, seed=3)
    ref = oracle.accel_f64(b, 1.0, eps2=cr.EPS2)[:, :3]
    a32 = oracle.accel_f32(b, 1.0, eps2=cr.EPS2)[:, :3].astype(np.float64)
    amax = np.abs(ref).max()
    assert np.abs(a32 - ref).max() < TOL_ACC * amax
    x, m = b[:, :3].astype(np.float64), b[:, 3].astype(np.float64)
    rows = np.random.default_rng(0).choice(n, 64, replace=False)
    hidden = total = 0
    best = None
    for i in rows:
        dr = x - x[i]
        r2 = (dr * dr).sum(1) + cr.EPS2
        t = (m / (r2 * np.sqrt(r2)))[:, None] * dr
        size = np.sqrt((t * t).sum(1))
        size[i] = np.inf
        quiet = (size < 0.25 * TOL_ACC * amax) & (np.roll(size, -1) < 0.25 * TOL_ACC * amax)      # the pair and the one behind it
        quiet[-1] = False
        hidden, total = hidden + int((size < TOL_ACC * amax).sum()), total + n - 1
        j = int(np.argmax(np.where(quiet, size, -1.0)))
        if best is None or size[j] > best[2]:
            best = (int(i), j, float(size[j]), t)
    i, j, size, t = best
    assert hidden > 0.4 * total                       # 46 % of all ordered pairs are smaller than the whole bound
    j1 = j + 1
    for name, delta in (("drop", -t[j]), ("double", t[j]), ("shift", t[j1] - t[j])):
        mutated = a32.copy()
        mutated[i] += delta
        old = np.abs(mutated - ref).max() / amax
        scale = np.sqrt((t * t).sum(1)).sum()
        census = np.sqrt(((mutated[i] - ref[i]) ** 2).sum()) / scale
        print("plummer %d, row %d <- %d (%.3g of max|a|) %s: older metric %.3g (bound 2e-5), on the row's own scale %.3g" % (n, i, j, size / amax, name, old, census))
        assert old < TOL_ACC, name
