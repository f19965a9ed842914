"""GPU tests of nb_list_force: acceleration, jerk and potential summed over neighbour rows.

The census inputs of tests/list_force_ref.py (jittered lattice, the bodies inside 1.6 / 2.4 spacings) are held to the tolerances
recorded in tests/golden/list_force_census.json -- 8 x the worst row error of a binary32 restatement, on the metric |got - ref|_2 /
sum |term|_2 where ONE missed, doubled or misattributed entry shows --, f64 handles to 1e-12 on the same metric.  The structure cases
(caps and row counts around every boundary of the launch shape, padding, entries that are no body, own indices, duplicates) run on
sub-rows and re-packings of the input (1025, 2.4 spacings) -- the same pairs, rows no longer than its rows -- and are held to that
input's tolerances, with exact zeros where a row has no valid entry.  Why that input's tolerance covers shorter rows: on this metric a
row's error is at most (the rounding of one term, ~10 x 2^-24 for a, more for the jerk) + (terms in one chain) x 2^-24, both relative
to sum |term|, so the restatement's worst row error grows with the row's length and a row of fewer terms from the same pairs stays
inside the bound measured for the longer rows (the knn and batch cases say which input they borrow from, for the same reason).  The
promises about bits are checked as bits."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden32, torch
import list_force_ref as R
from list_force_ref import NONE
from nbody3d_amd import MultiSimulation, Simulation, capi, ic
from nbody3d_amd.capi import NBodyError

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f64": np.float64}
FLAT = {"f32": 2e-5, "f64": 1e-12}          # the project's flat bound (tests/test_field_gpu.py)
INPUTS = [(n, sp) for n in R.SIZES for sp in R.SPACINGS]


def flat_errors(a, f, ra, rf):
    """tests/test_field_gpu.py's norm: per row max |a - ref| / max |ref| over the components, the worst row; phi relative."""
    ea = (np.abs(a[:, :3].astype(np.float64) - ra).max(1) / np.abs(ra).max(1)).max() if a is not None else 0.0
    ef = (np.abs(f.astype(np.float64) - rf) / np.abs(rf)).max() if f is not None else 0.0
    return float(ea), float(ef)


def handle(b, v=None, precision="f32", G=R.G, dt=1e-3, eps2=R.EPS2, **kw):
    s = Simulation(len(b), precision=precision, eps2=eps2, **kw)
    s.init(b, np.zeros_like(b) if v is None else v)
    s.set_params(dt, G)
    return s


def hermite(b, v, precision="f32", **kw):
    return handle(b.astype(DT[precision]), v.astype(DT[precision]), precision, integrator="hermite4", **kw)


def tols(precision, n=1025, spacings=2.4, pre=""):
    if precision == "f64":
        return (R.TOL_F64,) * 3
    e = R.entry(n, spacings)
    return e[pre + "a_tol"], e[pre + "jerk_tol"], e[pre + "phi_tol"]


def hold(got, ref, tol, what):
    """Every output that was asked for within its tolerance on the row metric; rows without a term exactly zero (row_err asserts it)."""
    err = R.errors(got[0], got[1], got[2], ref)
    print(what, "errors (a, jerk, phi):", err, "tolerances:", tol)
    for e, t, name in zip(err, tol, ("a", "jerk", "phi")):
        assert e is None or e <= t, (what, name, e, t)
    for x in got[:2]:
        assert x is None or not x[:, 3].any(), what
    empty = ref["terms"] == 0
    for x in got:
        if x is not None and empty.any():
            assert not np.signbit(x[empty]).any(), (what, "an empty row must give +0")


def bits(x, y, what):
    for p, q in zip(x, y):
        assert (p is None) == (q is None), what
        if p is not None:
            assert p.dtype == q.dtype and p.tobytes() == q.tobytes(), what


_fix = {}


def fixture(precision):
    """The input (1025, 2.4 spacings) in the handle's precision with its fp64 reference, and one full result, computed once."""
    if precision not in _fix:
        c = R.census_input(1025, 2.4)
        dt = DT[precision]
        b, v = c["b"].astype(dt), c["v"].astype(dt)
        with hermite(b, v, precision) as s:
            full = s.list_force(c["lists"], bodies=(0, 1025), jerk=True, phi=True)
            shape = s.list_force_shape(1025, 128)
        _fix[precision] = dict(c=c, b=b, v=v, full=full, LS=shape["lanes_per_row"], shape=shape)
    return _fix[precision]


# ---- 1. census ---------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n,spacings", INPUTS)
def test_census_four_ways(n, spacings, precision):
    c = R.census_input(n, spacings)
    dt = DT[precision]
    b, v, pts, pv = (c[k].astype(dt) for k in ("b", "v", "pts", "pv"))
    ref, pref = c["ref"], c["pref"]            # (the stored rows are binary32 in both precisions: one reference serves both)
    tol, ptol = tols(precision, n, spacings), tols(precision, n, spacings, "pt_")
    with hermite(b, v, precision) as s:
        hold(s.list_force(c["lists"], bodies=(0, n), jerk=True, phi=True), ref, tol, "at the bodies, Hermite")
        hold(s.list_force(c["plists"], points=pts, point_vel=pv, jerk=True, phi=True), pref, ptol, "at the points")
        own, cnt = s.neighbor_lists(bodies=(0, n), radius=c["radius"], cap=R.CAP)
        assert np.array_equal(own, c["lists"]) and np.array_equal(cnt, c["count"])
        hold(s.list_force(own, bodies=(0, n), count=cnt, jerk=True, phi=True), ref, tol, "nb_neighbor_lists' own rows")
        pown, pcnt = s.neighbor_lists(pts, radius=c["radius"], cap=R.CAP)
        assert np.array_equal(pown, c["plists"]) and np.array_equal(pcnt, c["pcount"])
    with handle(b, v, precision) as s:
        hold(s.list_force(c["lists"], bodies=(0, n), phi=True), ref, tol, "a + phi, leapfrog handle")


# ---- 2. structure ------------------------------------------------------------------------------

def caps(LS):
    return sorted({1, LS - 1, LS, LS + 1, 64, 65, 128})


def row_counts(LS):
    return sorted({1, 64 // LS - 1, 64 // LS + 1, 256 // LS - 1, 256 // LS + 1, 1025} - {0})


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_caps_and_row_counts_around_every_boundary(precision):
    f = fixture(precision)
    c, LS = f["c"], f["LS"]
    assert LS in (8, 16, 32) and f["shape"]["batch"] == 1025
    tol = tols(precision)
    with hermite(f["b"], f["v"], precision) as s:
        for cap in caps(LS):
            rows = np.ascontiguousarray(c["lists"][:, :cap])
            ref = R.list_ref(f["b"], f["v"], rows)
            hold(s.list_force(rows, bodies=(0, 1025), jerk=True, phi=True), ref, tol, "cap %d" % cap)
        for m in row_counts(LS):
            for first in (0, 1025 - m):
                rows = c["lists"][first:first + m]
                got = s.list_force(rows, bodies=(first, m), jerk=True, phi=True)
                hold(got, R.list_ref(f["b"], f["v"], rows, first=first), tol, "m %d first_body %d" % (m, first))
                bits(got, [x[first:first + m] for x in f["full"]], "a sub-range has the bits of the full request")


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_entries_that_are_no_entries(precision):
    f = fixture(precision)
    c, n = f["c"], 1025
    b, v = f["b"], f["v"]
    tol = tols(precision)
    rng = np.random.default_rng(3)
    rows = c["lists"].copy()
    rows[5] = NONE                                          # empty rows
    rows[1024] = NONE
    mid = rng.random(rows.shape) < 0.25                     # padding in the middle of the rows
    mid[:, 0] = False
    holes = np.where(mid, NONE, rows)
    junk = rows.copy()                                      # an entry = n and an entry = 0xfffffffe in front of every row
    junk[:, 40:] = NONE
    junk = np.concatenate([np.full((n, 1), n, np.uint32), np.full((n, 1), 0xfffffffe, np.uint32), junk], axis=1)[:, :128]
    own = rows.copy()                                       # the own index, first and in the middle of an AT_BODIES row
    own[:, 40:] = NONE
    own = np.concatenate([np.arange(n, dtype=np.uint32)[:, None], own[:, :20], np.arange(n, dtype=np.uint32)[:, None], own[:, 20:]], axis=1)[:, :128]
    dup = rows.copy()                                       # the first entry once more at the end of the row's 60 columns: it counts twice
    dup[:, 60:] = NONE
    dup[:, 60] = dup[:, 0]
    with hermite(b, v, precision) as s:
        for name, r in (("empty rows", rows), ("padding in the middle", holes), ("entries >= n", junk), ("own index", own), ("duplicate", dup)):
            hold(s.list_force(r, bodies=(0, n), jerk=True, phi=True), R.list_ref(b, v, r), tol, name)
        # (the reference leaves the own index out and counts a duplicate twice: the own term, m / sqrt(eps2), and the doubled term are
        # each a share of phi far above the tolerance)
        # count > cap reads cap entries; a count of 0 empties the row
        cnt = np.full(n, 4096 + 7, np.uint32)
        cnt[::3] = 0
        got = s.list_force(rows, bodies=(0, n), count=cnt, jerk=True, phi=True)
        hold(got, R.list_ref(b, v, rows, count=cnt), tol, "count > cap, count = 0")
        assert not got[0][::3].any() and not got[1][::3].any() and not got[2][::3].any()
    for nn in (1, 2):                                       # n = 1 and n = 2
        bb, vv = b[:nn].copy(), v[:nn].copy()
        r = np.array([[0, 1, NONE, 1, 0, 7]], np.uint32).repeat(nn, 0)
        with hermite(bb, vv, precision) as s:
            hold(s.list_force(r, bodies=(0, nn), jerk=True, phi=True), R.list_ref(bb, vv, r), tol, "n = %d" % nn)
            p, pv = f["c"]["pts"][:3].astype(DT[precision]), f["c"]["pv"][:3].astype(DT[precision])
            r3 = np.array([[0, 1, NONE]], np.uint32).repeat(3, 0)
            hold(s.list_force(r3, points=p, point_vel=pv, jerk=True, phi=True), R.list_ref(bb, vv, r3, pts=p, pvel=pv), tol, "n = %d, points" % nn)


# ---- 3. bits -----------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_a_rows_bits_depend_on_its_entries_alone(precision):
    assert torch is not None
    f = fixture(precision)
    c, n, b, v = f["c"], 1025, f["b"], f["v"]
    assert int(c["count"].max()) <= 64                      # no row longer than 64: cap 128 re-packs to cap 64
    tt = torch.float64 if precision == "f64" else torch.float32
    stream = torch.cuda.Stream()
    with hermite(b, v, precision, stream=stream.cuda_stream) as s:
        bits(s.list_force(c["lists"], bodies=(0, n), jerk=True, phi=True), f["full"], "the same request twice")
        bits(s.list_force(np.ascontiguousarray(c["lists"][:, :64]), bodies=(0, n), jerk=True, phi=True), f["full"], "cap 128 re-packed to cap 64")
        bits(s.list_force(c["lists"], bodies=(0, n), count=c["count"], jerk=True, phi=True), f["full"], "count given")
        a_only = s.list_force(c["lists"], bodies=(0, n))
        bits(a_only[:1], f["full"][:1], "accel alone")
        with torch.cuda.stream(stream):
            lst = torch.from_numpy(c["lists"].view(np.int32).copy()).to("cuda")
            cnt = torch.from_numpy(c["count"].view(np.int32).copy()).to("cuda")
            a, j = (torch.full((n, 4), 7.0, device="cuda", dtype=tt) for _ in range(2))
            p = torch.full((n,), 7.0, device="cuda", dtype=tt)
            s.list_force_device(lst.data_ptr(), 0, 128, bodies=(0, n), count_ptr=cnt.data_ptr(), accel_ptr=a.data_ptr(), jerk_ptr=j.data_ptr(),
                                phi_ptr=p.data_ptr())
        stream.synchronize()
        bits([x.cpu().numpy() for x in (a, j, p)], f["full"], "device pointers")
        with torch.cuda.stream(stream):
            a.fill_(7.0)
            j.fill_(7.0)
            s.list_force_device(lst.data_ptr(), 0, 128, bodies=(0, n), phi_ptr=p.data_ptr())       # phi only: nothing else is written
        stream.synchronize()
        assert bool((a == 7).all()) and bool((j == 7).all()) and p.cpu().numpy().tobytes() == f["full"][2].tobytes()
    with hermite(b, v, precision) as s:
        ia, ij, ip, icnt = s.irregular_force(c["radius"], 128, phi=True)
        assert np.array_equal(icnt, c["count"])
        bits((ia, ij, ip), f["full"], "irregular_force against lists, then list_force through the host")


# ---- 4. against the passes over all pairs ------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n", [1025, 4097])
def test_full_rows_against_the_all_pairs_passes(n, precision):
    """cap = n - 1, every other body in every row: a and phi against nb_field_eval AT_BODIES, the jerk against read_jerk() of a fresh
    Hermite handle, each within 2 x the flat bound (both sides are within the bound of the fp64 sum), and each within the flat bound of
    the fp64 reference.  A lane's chain has at most 4096 / 8 = 512 terms: worst case 512 x 2^-24 = 3e-5.
    Measured worst rows (f32, MI355X): see profiles/r14/list_force.md."""
    dt = DT[precision]
    b, v = (x.astype(dt) for x in ic.plummer(n, seed=14))
    rows = np.arange(n, dtype=np.uint32)[None, :].repeat(n, 0)
    rows = np.ascontiguousarray(rows[~np.eye(n, dtype=bool)].reshape(n, n - 1))
    ref = R.list_ref(b, v, rows, G=1.0, eps2=1e-4)
    bound = FLAT[precision]
    with hermite(b, v, precision, G=1.0, eps2=1e-4) as s:
        a, j, phi = s.list_force(rows, bodies=(0, n), jerk=True, phi=True)
        fa, fphi = s.field(bodies=(0, n))
        fj = s.read_jerk()
    ea, ep = flat_errors(a, phi, ref["a"], ref["phi"])
    ej = flat_errors(j, None, ref["j"], None)[0]
    ca, cp = flat_errors(a, phi, fa[:, :3].astype(np.float64), fphi.astype(np.float64))
    cj = flat_errors(j, None, fj[:, :3].astype(np.float64), None)[0]
    print("n %d %s: against fp64 a %.3g jerk %.3g phi %.3g; against the all-pairs passes a %.3g jerk %.3g phi %.3g" % (n, precision, ea, ej, ep, ca, cj, cp))
    assert max(ea, ej, ep) <= bound, (ea, ej, ep)
    assert max(ca, cj, cp) <= 2 * bound, (ca, cj, cp)


# ---- 5. nb_knn rows ----------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("k", [6, 64])
def test_knn_rows_are_valid_input(k, precision):
    f = fixture(precision)
    b, v, n = f["b"], f["v"], 1025
    with hermite(b, v, precision) as s:
        index, _ = s.knn(bodies=(0, n), k=k)
        assert (np.diff(index.astype(np.int64), axis=1) < 0).any()          # nearest first: the rows do not ascend
        ref = R.list_ref(b, v, index)
        # (the k nearest bodies: every share is larger than in the radius rows, which hold up to 64 members)
        hold(s.list_force(index, bodies=(0, n), jerk=True, phi=True), ref, tols(precision), "knn rows, k = %d" % k)


# ---- 6. batches --------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_wide_rows_go_through_in_two_batches(precision):
    f = fixture(precision)
    b, v, n, m, cap = f["b"], f["v"], 1025, 16400, 4096
    rng = np.random.default_rng(8)
    pts = np.zeros((m, 4), DT[precision])
    pts[:, :3] = b[rng.integers(0, n, m), :3] + rng.uniform(0.2, 0.4, (m, 3)) * R.SPACING * rng.choice([-1, 1], (m, 3))
    rows = np.full((m, cap), 0, np.uint32)                               # what lies behind count is never read: body 0, not padding
    cnt = rng.integers(0, 4, m).astype(np.uint32)
    near = R.radius_rows(b, 1.2 * R.SPACING, 3, targets=pts)[0]
    rows[:, :3] = np.where(near == NONE, rng.integers(0, n, (m, 3)), near)
    with hermite(b, v, precision) as s:
        shape = s.list_force_shape(m, cap)
        assert shape["batch"] < m <= 2 * shape["batch"] and shape["batch"] * cap * 4 <= 256 << 20 and shape["batch"] % (256 // f["LS"]) == 0
        got = s.list_force(rows, points=pts, count=cnt, phi=True)
        ref = R.list_ref(b, v, rows, pts=pts, count=cnt)
        # rows of at most three terms between the bodies: the tolerances of the input's point rows
        hold(got, ref, tols(precision, pre="pt_"), "16,400 rows at cap 4096")
        assert (ref["terms"] == cnt).all() and not got[0][cnt == 0].any() and not got[2][cnt == 0].any()
        k = shape["batch"]                                               # the rows around the seam, alone: the same bits
        bits(s.list_force(rows[k - 2:k + 2], points=pts[k - 2:k + 2], count=cnt[k - 2:k + 2], phi=True), [x if x is None else x[k - 2:k + 2] for x in got],
             "the rows around the seam of the batches")


# ---- 7. the state is untouched -----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["symmetric", "hermite", "block"])
def test_stepping_is_bit_identical_with_a_call_in_between(kind):
    n = 4096 if kind == "symmetric" else 1024
    b, v = ic.plummer(n, seed=21)
    kw = {"force_variant": 708013} if kind == "symmetric" else {"integrator": "hermite4"}
    rows = np.random.default_rng(2).integers(0, n, (n, 24)).astype(np.uint32)

    def run(query):
        with handle(b, v, **kw) as s:
            if kind == "block":
                s.set_block_steps()
            s.simulate(3)
            if query:
                a, j, phi = s.list_force(rows, bodies=(0, n), jerk=kind != "symmetric", phi=True)
                assert np.isfinite(a).all() and np.isfinite(phi).all() and (phi < 0).all()
                s.list_force(rows[:100], points=b[:100], accel=False, phi=True)
            s.simulate(3)
            return s.read() + (s.variant,)

    plain, mixed = run(False), run(True)
    print(kind, plain[3])
    if kind == "symmetric":
        assert "sym" in plain[3], plain[3]
    for x, y in zip(plain[:3], mixed[:3]):
        assert x.tobytes() == y.tobytes()


# ---- 8. shards ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shards", [2, 3])
def test_multi_handles_have_the_single_handles_bits(shards):
    f = fixture("f32")
    c, b, v, n = f["c"], f["b"], f["v"], 1025
    rows = c["lists"].copy()
    rows[:, 100] = n                                                     # a padding row of the padded system: never a body
    rows[:, 101] = n + 1
    with handle(b, v) as s:
        single = s.list_force(rows, bodies=(0, n), phi=True) + s.list_force(c["plists"], points=c["pts"], phi=True)
    bits(single[:3], (f["full"][0], None, f["full"][2]), "a leapfrog handle has the Hermite handle's bits")
    with MultiSimulation(n, shards, eps2=R.EPS2) as m:
        m.init(b, v)
        m.set_params(1e-3, R.G)
        multi = m.list_force(rows, bodies=(0, n), phi=True) + m.list_force(c["plists"], points=c["pts"], phi=True)
        bits(multi, single, "%d shards" % shards)
        with pytest.raises(NBodyError) as e:
            m.list_force(rows, bodies=(0, n), jerk=True)
        assert e.value.code == 1 and "jerk" in str(e.value) and "nb_multi_list_force" in str(e.value)
        with pytest.raises(NBodyError) as e:
            m.list_force(rows[:301], bodies=(n - 300, 301))              # row n exists in the padded system, not in the caller's
        assert e.value.code == 1 and "first_body" in str(e.value) and "nb_multi_list_force" in str(e.value)
        m.simulate(2)


# ---- 9. errors ---------------------------------------------------------------------------------

def test_every_invalid_request_is_an_ordinary_error():
    b = load_golden32("plummer1024_bodies0")
    v = load_golden32("plummer1024_vel0")
    L = capi.load_library()
    one = np.zeros((1, 4), np.float32)
    out = np.zeros((1, 4), np.float32)
    row = np.arange(8, dtype=np.uint32)[None, :]
    P = lambda a: a.ctypes.data_as(C.c_void_p)

    def raw(s, **kw):
        req = capi.nb_list_force_request()
        req.struct_size = C.sizeof(capi.nb_list_force_request)
        req.m, req.cap = 1, 8
        req.points, req.list, req.accel = P(one), P(row), P(out)
        for name, val in kw.items():
            setattr(req, name, val)
        rc = L.nb_list_force(s._h, C.byref(req))
        return rc, L.nb_last_error(s._h).decode()

    with Simulation(1024) as s:
        with pytest.raises(NBodyError) as e:             # nothing uploaded
            s.list_force(row, points=one)
        assert e.value.code == 4 and "upload" in str(e.value) and "nb_list_force" in str(e.value)
        s.init(b, v)
        with pytest.raises(NBodyError) as e:             # no parameters
            s.list_force(row, points=one)
        assert e.value.code == 4 and "nb_set_params" in str(e.value) and "nb_list_force" in str(e.value)
        s.set_params(1e-3, 1.0)
        with pytest.raises(NBodyError) as e:             # the jerk on a leapfrog handle
            s.list_force(row, bodies=(0, 1), jerk=True)
        assert e.value.code == 4 and "Hermite" in str(e.value) and "nb_list_force" in str(e.value)
        AT = capi.NB_LISTF_AT_BODIES
        for kw, word in ((dict(struct_size=72), "struct_size"), (dict(struct_size=88), "struct_size"), (dict(m=0), "m must"),
                         (dict(flags=2), "flags"), (dict(flags=8), "flags"), (dict(flags=1 << 31), "flags"), (dict(list=None), "list is NULL"),
                         (dict(cap=0), "cap must"), (dict(cap=4097), "cap must"), (dict(cap=0xffffffff), "cap must"), (dict(reserved=1), "reserved"),
                         (dict(accel=None), "all NULL"), (dict(points=None), "points is NULL"), (dict(flags=AT), "points must be NULL"),
                         (dict(flags=AT, points=None, point_vel=P(one)), "point_vel must be NULL"),
                         (dict(point_vel=P(one)), "point_vel must be NULL"), (dict(jerk=P(out)), "point_vel is NULL"),
                         (dict(flags=AT, points=None, first_body=1024), "first_body"),
                         (dict(flags=AT, points=None, first_body=0xffffffff, m=2), "first_body")):
            rc, msg = raw(s, **kw)
            assert rc == 1 and "nb_list_force" in msg and word in msg, (kw, rc, msg)
        assert L.nb_list_force(s._h, None) == 1
        for m, cap, word in ((0, 8, "m must"), (1, 0, "cap must"), (1, 4097, "cap must")):
            with pytest.raises(NBodyError) as e:
                s.list_force_shape(m, cap)
            assert e.value.code == 1 and word in str(e.value) and "nb_list_force_shape" in str(e.value)
        assert raw(s)[0] == 0                                            # and the same request without a fault is served
        assert raw(s, flags=AT, points=None, first_body=1023)[0] == 0 and raw(s, accel=None, phi=P(out))[0] == 0
        s.simulate(2)                                                    # ... and the handle still steps
    with Simulation(1024, integrator="hermite4") as s:
        s.init(b, v)
        s.set_params(1e-3, 1.0)
        rc, msg = raw(s, jerk=P(out))
        assert rc == 1 and "point_vel is NULL" in msg
        assert raw(s, jerk=P(out), point_vel=P(one))[0] == 0 and raw(s, flags=AT, points=None, jerk=P(out))[0] == 0
