"""tests/query_state.py proven without a GPU: a numpy handle with the wrapper's method names answers every query from the brute-force
references (neighbors_ref.float_ref's fp64 distances for nb_neighbors / nb_neighbor_lists / nb_knn -- the lattice references of
neighbor_lists_ref.py and knn_ref.py take integer coordinates only, so their row rules are restated here on those distances --,
list_force_ref.list_ref, test_field_gpu.ref_field and query_state.ref_energy) over a state it is handed.

compare() passes on two such handles over one state and fails, in every category, against the state one oracle.run_f32 step
(dt = 1e-2, G = 1, ic.plummer(n, seed=21)) earlier -- which is what tests/test_query_state_gpu.py relies on for its control.

Rows that one step changes, of 256 points / 300 bodies (cap 16, k 7, h 0.3, radii in [0.15, 0.45]), as this test derived them
(n = 777 / 1024 / 2002):

    nearest index, points + bodies rows (16 + 3, 24 + 5, 23 + 6)      19 /  29 /  29
    count, at the points                                               46 /  56 /  61
    count, at the bodies                                              112 / 125 / 141
    list rows, at the points                                           34 /  37 /  37
    list rows, at the bodies                                           99 /  98 / 116
    k = 7 rows, at the points                                          78 /  82 /  94
    k = 7 rows, at the bodies                                         190 / 183 / 202

(neighbors() and neighbor_lists() give the same counts.)  The points stand still, half of them in the thin outskirts of the bounding
box: the nearest body of only 3 to 6 of the 256 changes in one step, so the control takes a query's nearest index over its point
and body rows together (query_state.INT_GROUPS); every other output clears the 10 rows on its own.  A step also moves the field by
1e-2 to 4 (relative, bound 2e-5) and the energies by 1e-4.
"""
import numpy as np
import pytest

from knn_ref import NONE
from list_force_ref import list_ref
from neighbors_ref import float_ref
from oracle import oracle
from query_state import MIN_ROWS, answers, compare, ref_energy, requests, stale_must_fail
from test_field_gpu import EPS2, ref_field

DT, G, SEED = 1e-2, 1.0, 21


class FakeHandle:
    """The answers the header promises, by numpy in fp64 on the rows of `state`, rounded to the handle's precision."""

    def __init__(self, state, dtype=np.float32, G=G, eps2=EPS2, steps=0):
        self.b, self.v = np.asarray(state[0]), np.asarray(state[1])
        self.n = self.shard_count = len(self.b)
        self.dtype, self.G, self.eps2, self.steps = dtype, G, eps2, steps

    def _d2(self, points, bodies):
        """(m, n) fp64 squared distances, a body's own column at +inf; the radii's squares come in the handle's precision."""
        p, skip0 = (self.b[bodies[0]:bodies[0] + bodies[1]], bodies[0]) if bodies is not None else (np.asarray(points), None)
        block, _ = float_ref(self.b, p, skip0)
        return block(0, len(p))

    def _h2(self, m, radius, radii):
        h = np.full(m, radius, self.dtype) if radii is None else np.asarray(radii, self.dtype)
        return (h * h).astype(np.float64)

    def _nearest(self, q):
        j = q.argmin(1)                                    # the first of equal minima: the smallest index
        best = q[np.arange(len(q)), j]
        return np.where(np.isfinite(best), j, NONE).astype(np.uint32), best.astype(self.dtype)

    def neighbors(self, points=None, *, bodies=None, radius=None, radii=None):
        q = self._d2(points, bodies)
        index, dist2 = self._nearest(q)
        count = None if radius is None and radii is None else (q < self._h2(len(q), radius, radii)[:, None]).sum(1).astype(np.uint32)
        return index, dist2, count

    def neighbor_lists(self, points=None, *, bodies=None, radius=None, radii=None, cap=64, nearest=False):
        q = self._d2(points, bodies)
        inside = q < self._h2(len(q), radius, radii)[:, None]
        lists = np.full((len(q), cap), NONE, np.uint32)
        rank = np.cumsum(inside, axis=1) - 1               # ascending index; the cap smallest where there are more
        k, j = np.nonzero(inside & (rank < cap))
        lists[k, rank[k, j]] = j
        count = inside.sum(1).astype(np.uint32)
        return (lists, count) + self._nearest(q) if nearest else (lists, count)

    def knn(self, points=None, *, bodies=None, k=6, dist2=True):
        q = self._d2(points, bodies)
        order = np.argsort(q, axis=1, kind="stable")[:, :k]      # d2 ascending, then index ascending
        best = np.take_along_axis(q, order, axis=1)
        return np.where(np.isfinite(best), order, NONE).astype(np.uint32), best.astype(self.dtype) if dist2 else None

    def list_force(self, lists, *, bodies=None, points=None, point_vel=None, count=None, accel=True, jerk=False, phi=False):
        r = list_ref(self.b, self.v if jerk else None, lists, G=self.G, eps2=self.eps2, first=0 if bodies is None else bodies[0],
                     pts=points, pvel=point_vel, count=count)
        four = lambda x: np.concatenate([x, np.zeros((len(x), 1))], axis=1).astype(self.dtype)
        return four(r["a"]) if accel else None, four(r["j"]) if jerk else None, r["phi"].astype(self.dtype) if phi else None

    def field(self, points=None, *, bodies=None, accel=True, phi=True, f64=False):
        rows = None if bodies is None else np.arange(bodies[0], bodies[0] + bodies[1])
        a, f = ref_field(self.b, self.b[rows] if bodies is not None else points, G=self.G, eps2=self.eps2, skip=rows)
        t = np.float64 if f64 else self.dtype
        return np.concatenate([a, np.zeros((len(a), 1))], axis=1).astype(t), f.astype(t)

    def diagnostics(self):
        e, _ = ref_energy((self.b, self.v), self.G, self.eps2)
        return e[0], e[1], e[2:]

    def request_frame(self):
        pass

    def frame(self):
        return self.b.astype(np.float32), np.sqrt((self.v[:, :3].astype(np.float64) ** 2).sum(1)).astype(np.float32), self.steps


@pytest.fixture(scope="module", params=[777, 1024, 2002])
def case(request):
    """(n, request set, the states after one and after two steps, the answers on both) -- computed once per n."""
    n = request.param
    req = requests(n, np.float32, SEED, hermite=(n == 777))        # one size also with the jerk outputs
    s1 = oracle.run_f32(req["bodies"], req["vel"], None, DT, G, 1)
    s2 = oracle.run_f32(*s1, DT, G, 1)
    return n, req, s1, s2, answers(FakeHandle(s1, steps=1), req), answers(FakeHandle(s2, steps=2), req)


def test_request_set_is_what_the_gpu_tests_expect(case):
    n, req, *_ = case
    first, count = req["range"]
    assert req["points"].shape == (256, 4) and first == n // 3 and count == min(300, n - first)
    assert first // 256 != (first + count - 1) // 256, "the AT_BODIES range does not straddle a 256-row tile boundary"
    on = (req["points"][::10, None, :3] == req["bodies"][None, :, :3]).all(2).any(1)
    assert on.all(), "every 10th point sits exactly on a body"
    lists = req["lists"]
    assert lists.shape == (300, 24) and 0.05 < (lists == NONE).mean() < 0.15 and ((lists >= n) & (lists != NONE)).sum() >= 3
    assert (req["count"] > 24).any() and (req["count"] < 24).any()
    again = requests(n, np.float32, SEED, hermite=False)
    assert all(np.array_equal(req[k], again[k]) for k in req if isinstance(req[k], np.ndarray))


def test_same_state_passes(case):
    n, req, s1, s2, a1, a2 = case
    assert ("lf_pts.jerk" in a2) == req["hermite"] and "field64_pts.accel" in a2 and "frame.bodies" in a2
    assert int((a2["nbl_bod.count"] > req["cap"]).sum()) >= MIN_ROWS, "no row overflows: the truncation path is not exercised"
    again = answers(FakeHandle(s2, steps=2), req)
    compare(a2, again, s2, req, "f32", True, G=G, steps=2, where="numpy handle, n=%d" % n)
    compare(a2, again, s2, req, "f32", False, G=G, where="numpy handle, n=%d, tolerance only" % n)


def test_one_step_old_state_fails_every_category(case):
    n, req, s1, s2, a1, a2 = case
    where = "numpy handle, n=%d" % n
    rows = stale_must_fail(a2, a1, s1, req, "f32", G=G, where=where)
    assert min(rows.values()) >= MIN_ROWS
    for same_shape in (True, False):
        with pytest.raises(AssertionError):
            compare(a2, a1, s1, req, "f32", same_shape, G=G, where=where)
    with pytest.raises(AssertionError) as e:                       # the step index alone
        compare(a2, answers(FakeHandle(s2, steps=2), req), s2, req, "f32", True, G=G, steps=3, where=where)
    assert "frame.step" in str(e.value) and "nbr_pts" not in str(e.value)


def test_a_single_wrong_row_is_named(case):
    n, req, s1, s2, a1, a2 = case
    for name in ("nbl_bod.list", "knn_pts.dist2", "lf_bod.phi", "field_bod.accel", "diag", "frame.bodies"):
        other = {k: x.copy() for k, x in a2.items()}
        flat = other[name].reshape(len(other[name]), -1)
        flat[len(flat) // 2, 0] = np.nextafter(flat[len(flat) // 2, 0], np.inf) if flat.dtype.kind == "f" else flat[len(flat) // 2, 0] ^ 1
        with pytest.raises(AssertionError) as e:
            compare(other, a2, s2, req, "f32", True, G=G, where="numpy handle, n=%d" % n)
        assert name in str(e.value) and ("[%d]" % (len(flat) // 2) in str(e.value) or name == "frame.bodies" or len(flat) == 5), str(e.value)


def test_a_handle_without_a_frame_feed_compares_with_a_twin_that_has_one(case):
    """Multi and shard handles answer no frame; their twin, a whole-system handle, does.  The reverse is a missing output."""
    n, req, s1, s2, a1, a2 = case
    shard = FakeHandle(s2)
    shard.shard_count = n // 2
    got = answers(shard, req)
    assert "frame.bodies" not in got and "diag" in got
    compare(got, a2, s2, req, "f32", False, G=G, where="numpy handle, n=%d, no frame" % n)
    with pytest.raises(AssertionError) as e:
        compare(a2, got, s2, req, "f32", False, G=G, where="numpy handle, n=%d" % n)
    assert "different sets of outputs" in str(e.value)
