"""GPU tests of nb_split_lists: nb_split_force's four sums and nb_neighbor_lists' rows from one pass over the pairs.

The yardsticks are the two calls that exist -- nb_split_force for the sums, nb_neighbor_lists for the rows, both unchanged -- and
an integer brute force on the CPU; never the new call against itself.  Wherever nb_split_lists_shape reports nb_split_force_shape's
(batch, chunks, j_per_chunk) the sums are compared as BYTES; the rows and the counts are compared as bytes whatever the shapes are.
The inputs are the census inputs of tests/split_force_ref.py (jittered lattice; no pair within 1e-6 of its radius, so a membership
matrix computed in fp64 on the stored rows is the device's in both precisions)."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden32, torch
import census_ref
import list_force_ref
import split_force_ref as R
from nbody3d_amd import MultiSimulation, Simulation, capi, ic
from nbody3d_amd.capi import NBodyError

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f64": np.float64}
PRECS = ["f32", "f64"]
NONE = 0xffffffff
SUMS = R.OUTPUTS


def handle(b, v=None, precision="f32", G=R.G, dt=1e-3, eps2=R.EPS2, **kw):
    s = Simulation(len(b), precision=precision, eps2=eps2, **kw)
    s.init(b.astype(DT[precision]), (np.zeros_like(b) if v is None else v).astype(DT[precision]))
    s.set_params(dt, G)
    return s


def hermite(b, v, precision="f32", **kw):
    return handle(b, v, precision, integrator="hermite4", **kw)


def same_shape(s, m, cap):
    a, b = s.split_lists_shape(m, cap), s.split_force_shape(m)
    return a == b


def rows_of(member, cap, own=None):
    """(rows (m, cap) uint32, count (m,) uint32) of a membership matrix: ascending j, the cap smallest, padded; own[k] left out."""
    member = member.copy()
    if own is not None:
        member[np.arange(len(member)), own] = False
    rows = np.full((len(member), cap), NONE, np.uint32)
    for k, line in enumerate(member):
        j = np.nonzero(line)[0][:cap]
        rows[k, :len(j)] = j
    return rows, member.sum(1).astype(np.uint32)


def against_both(s, cap, what, sums_as_bits=True, **kw):
    """One request through nb_split_lists, nb_split_force and nb_neighbor_lists: the shape first, then bytes."""
    got = s.split_lists(cap=cap, **kw)
    m = len(got["count"])
    if sums_as_bits:
        assert same_shape(s, m, cap), (what, s.split_lists_shape(m, cap), s.split_force_shape(m))
    want = s.split_force(**kw)
    lkw = {k: v for k, v in kw.items() if k in ("points", "bodies", "radius", "radii")}
    lists, count = s.neighbor_lists(cap=cap, **lkw)
    assert set(got) == set(want) | {"list", "count"}, what
    assert got["list"].shape == (m, cap) and got["list"].tobytes() == lists.tobytes(), (what, "list")
    assert got["count"].tobytes() == count.tobytes(), (what, "count")
    if sums_as_bits:
        for name in want:
            assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), (what, name)
    return got


# ---- 1. bits against both calls ----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["hermite", "leapfrog"])
@pytest.mark.parametrize("precision", PRECS)
def test_bits_against_both_calls(precision, kind):
    c = R.census_input(1025, 2.4)
    dt = DT[precision]
    make = hermite if kind == "hermite" else handle
    names = SUMS if kind == "hermite" else SUMS[:2]
    for n in (1, 2, 255, 256, 257, 771, 1025):
        b, v = c["b"][:n], c["v"][:n]
        with make(b, v, precision) as s:
            got = against_both(s, 24, "n %d" % n, bodies=(0, n), radius=c["radius"])
            assert [k for k in got if k in SUMS] == list(names)
            assert (got["list"][got["list"] != NONE] < n).all() and not (got["list"] == np.arange(n)[:, None]).any()
            if n == 1:
                assert got["count"][0] == 0 and (got["list"] == NONE).all()
            if n != 1025:
                continue
            rpw = s.split_lists_shape(n, 24)["rows_per_workgroup"]
            assert rpw == s.split_force_shape(n)["rows_per_workgroup"]
            for m in sorted({1, 63, 64, 65, rpw - 1, rpw + 1} - {0}):
                for first in (0, n - m):
                    against_both(s, 24, "m %d first_body %d" % (m, first), bodies=(first, m), radius=c["radius"])
            pkw = dict(point_vel=c["pv"].astype(dt)) if kind == "hermite" else {}
            against_both(s, 24, "points", points=c["pts"].astype(dt), radius=c["radius"], **pkw)
            h = float(dt(c["radius"]))
            filled = against_both(s, 24, "filled radii", bodies=(0, n), radii=np.full(n, h, dt))
            for k in got:
                assert filled[k].tobytes() == got[k].tobytes(), ("scalar radius against a filled radii", k)
            alt = np.where(np.arange(n) % 2 == 0, 0.0, 100.0).astype(dt)
            mixed = against_both(s, 24, "radii 0 next to radii that cover everybody", bodies=(0, n), radii=alt)
            assert not mixed["count"][0::2].any() and (mixed["count"][1::2] == n - 1).all()
            assert (mixed["list"][0::2] == NONE).all() and not mixed["accel_irr"][0::2].any() and not mixed["accel_reg"][1::2].any()


# ---- 2. cap ------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECS)
def test_cap(precision):
    n = 1025
    c = R.census_input(n, 2.4)
    member = c["ref"]["member"]
    own = np.arange(n)
    got = {}
    with hermite(c["b"], c["v"], precision) as s:
        for cap in (1, 24, 100):
            got[cap] = against_both(s, cap, "cap %d" % cap, bodies=(0, n), radius=c["radius"])
            rows, count = rows_of(member, cap, own)
            assert got[cap]["list"].tobytes() == rows.tobytes() and got[cap]["count"].tobytes() == count.tobytes(), cap
        count = got[1]["count"]
        assert (count > 24).any() and (count > 1).any()                                # some rows overflow, and they hold the cap smallest (above)
        for small, big in ((1, 24), (1, 100), (24, 100)):
            assert np.array_equal(got[big]["list"][:, :small], got[small]["list"])      # the first c entries, for every cap >= c
        # rows of exactly cap next to empty rows: an even body's radius lies between its cap-th and its (cap + 1)-th neighbour
        cap = 24
        x = np.asarray(c["b"], np.float64)[:, :3]
        d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(2))
        d[own, own] = np.inf
        ds = np.sort(d, 1)
        gap_ok = ds[:, cap] / ds[:, cap - 1] > 1.0 + 1e-4
        radii = np.where((own % 2 == 0) & gap_ok, 0.5 * (ds[:, cap - 1] + ds[:, cap]), 0.0)
        assert (radii > 0).sum() > 400
        full = against_both(s, cap, "full rows next to empty ones", bodies=(0, n), radii=radii.astype(DT[precision]))
        assert (full["count"][radii > 0] == cap).all() and not full["count"][radii == 0].any()
        assert (full["list"][radii > 0] != NONE).all() and (full["list"][radii == 0] == NONE).all()


# ---- 3. several j-chunks -----------------------------------------------------------------------

def safe_radius(x, xt, r):
    """r, nudged up until no pair lies within 1e-5 (relative, in d2) of it: binary32 then decides as fp64 does."""
    d2 = ((x[None, :, :] - xt[:, None, :]) ** 2).sum(2)
    for k in range(100):
        h = np.float64(np.float32(r * (1.0 + 1e-3 * k)))
        if np.abs(d2 / (h * h) - 1.0).min() > 1e-5:
            return float(h), d2 < h * h
    raise AssertionError("no safe radius")


@pytest.mark.parametrize("precision", PRECS)
def test_several_j_chunks(precision):
    n, m = 4099, 64
    first = n - m
    c = R.census_input(n, 2.4)
    x = np.asarray(c["b"], np.float64)[:, :3]
    radius, member = safe_radius(x, x[first:], 5.0 * R.SPACING)
    own = np.arange(first, n)
    with hermite(c["b"], c["v"], precision) as s:
        shape = s.split_lists_shape(m, 24)
        print(shape)
        assert shape["chunks"] >= 2 and shape["chunks"] * shape["j_per_chunk"] >= n
        per = shape["j_per_chunk"]
        mem = member.copy()
        mem[np.arange(m), own] = False
        by_chunk = np.add.reduceat(mem.astype(np.int64), np.arange(0, n, per), axis=1)                 # (m, chunks): members per chunk
        # per row: the first two chunks that hold a member
        order = [np.nonzero(r)[0] for r in by_chunk]
        c0 = np.array([by_chunk[k, o[0]] if len(o) else 0 for k, o in enumerate(order)])
        c1 = np.array([by_chunk[k, o[1]] if len(o) > 1 else 0 for k, o in enumerate(order)])
        k1 = int(np.argmax(c0))
        k2 = int(np.argmax(c1))
        cap_a = int(c0[k1]) - 1                      # below the first chunk's member count of row k1
        cap_b = int(c0[k2] + (c1[k2] + 1) // 2)      # cuts inside the second chunk of row k2
        assert cap_a >= 1 and c1[k2] >= 2 and c0[k2] < cap_b < c0[k2] + c1[k2]
        print("caps", cap_a, cap_b, "counts", by_chunk.sum(1).min(), by_chunk.sum(1).max())
        for cap in (cap_a, cap_b, 24, int(by_chunk.sum(1).max()) + 3):
            got = against_both(s, cap, "%d chunks, cap %d" % (shape["chunks"], cap), bodies=(first, m), radius=radius)
            rows, count = rows_of(member, cap, own)
            assert got["list"].tobytes() == rows.tobytes() and got["count"].tobytes() == count.tobytes(), cap


# ---- 4. the three guards -----------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECS)
def test_rows_past_the_range_are_nobodys_members(precision):
    """n = 300 leaves rows past the range in the last tile; they are staged at the ORIGIN.  The bodies are moved away from it, and a
    point at the origin has nobody inside its radius: no index >= n, count <= n, and an empty row for that point."""
    n = 300
    c = R.census_input(1025, 2.4)
    dt = DT[precision]
    b = np.array(c["b"][:n])
    b[:, :3] += 5.0 - b[:, :3].min()
    pts = np.zeros((70, 4), dt)
    pts[1:, :3] = b[:69, :3] + 0.01
    with handle(b, c["v"][:n], precision) as s:
        for kw in (dict(radius=2.0), dict(radii=np.where(np.arange(70) % 2 == 0, 2.0, 100.0).astype(dt))):
            got = against_both(s, 24, "a point at the origin", points=pts, **kw)
            assert got["count"][0] == 0 and (got["list"][0] == NONE).all()
            assert (got["list"][got["list"] != NONE] < n).all() and (got["count"] <= n).all()
        big = against_both(s, 512, "everybody", points=pts, radius=100.0)
        assert (big["count"] == n).all() and (big["list"][:, :n] == np.arange(n)).all() and (big["list"][:, n:] == NONE).all()


@pytest.mark.parametrize("precision", PRECS)
def test_clamped_lanes_do_not_disturb_the_last_point(precision):
    n = 1025
    c = R.census_input(n, 2.4)
    with handle(c["b"], c["v"], precision) as s:
        m = s.split_lists_shape(n, 8)["rows_per_workgroup"] + 1
        for first in (0, n - m):
            got = against_both(s, 8, "m = rpw + 1", bodies=(first, m), radius=100.0)        # every lane, the clamped ones too, has members everywhere
            want = np.array([[j for j in range(9) if j != first + k][:8] for k in range(m)], np.uint32)
            assert np.array_equal(got["list"], want) and (got["count"] == n - 1).all()


@pytest.mark.parametrize("precision", PRECS)
def test_two_bodies_on_one_position(precision):
    n = 257
    c = R.census_input(1025, 2.4)
    b, v = np.array(c["b"][:n]), np.array(c["v"][:n])
    b[200, :3] = b[5, :3]
    with hermite(b, v, precision) as s:
        got = against_both(s, 256, "two bodies on one position", bodies=(0, n), radius=c["radius"])
    for k, other in ((5, 200), (200, 5)):
        row = got["list"][k][:got["count"][k]]
        assert other in row and k not in row
    assert not (got["list"] == np.arange(n)[:, None]).any()


# ---- 5. exact membership -----------------------------------------------------------------------

LAT = 9
LAT_EPS2 = 18.0


@pytest.mark.parametrize("precision", PRECS)
def test_exact_membership_on_the_lattice(precision):
    """Integer coordinates: d2 is exact in both precisions, the membership is int64 arithmetic's: 4 d2 < (2 h)^2.  Radius 3 leaves the
    pairs at d2 = 9 out, nextafter(3) takes them in."""
    dt = DT[precision]
    g = np.arange(LAT)
    xi = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    n = len(xi)
    b = np.zeros((n, 4), np.float32)
    b[:, :3], b[:, 3] = xi, 1.0 / n
    v = census_ref.velocities(n, 3)
    q = np.array([-1, 2, 5, 9])
    pi = np.stack(np.meshgrid(q, q, q, indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    pts = np.zeros((64, 4), dt)
    pts[:, :3] = pi
    pv = list_force_ref.point_velocities(64, 3).astype(dt)
    up = float(np.nextafter(dt(3), dt(np.inf)))
    alt = np.array([1, 2, 2.5, 3])
    cases = [("radius 3", dict(radius=3.0), lambda m: np.full(m, 36)), ("nextafter(3)", dict(radius=up), lambda m: np.full(m, 37)),
             ("radii 1, 2, 2.5, 3", None, lambda m: np.array([4, 16, 25, 36])[np.arange(m) % 4])]
    with hermite(b, v, precision, eps2=LAT_EPS2) as s:
        for what, kw, h2x4 in cases:
            for probes, pint, args, own in (("bodies", xi, dict(bodies=(0, n)), np.arange(n)), ("points", pi, dict(points=pts, point_vel=pv), None)):
                m = len(pint)
                d2 = ((xi[None, :, :] - pint[:, None, :]) ** 2).sum(2)
                member = 4 * d2 < h2x4(m)[:, None]
                assert (d2 == 9).any(1).all()
                rkw = dict(radii=alt[np.arange(m) % 4].astype(dt)) if kw is None else kw
                for cap in (7, 128):
                    got = against_both(s, cap, "%s, %s, cap %d" % (what, probes, cap), **args, **rkw)
                    rows, count = rows_of(member, cap, own)
                    assert got["list"].tobytes() == rows.tobytes() and got["count"].tobytes() == count.tobytes(), (what, probes, cap)


# ---- 6. two batches ----------------------------------------------------------------------------

def test_two_batches():
    """An f64 handle, m = batch + 300 arbitrary points against n = 300: the rows (around the seam and everywhere else) are
    nb_neighbor_lists'; the sums are nb_split_force's bits where the two calls cut the request alike, and are held to
    tests/test_split_force_gpu.py::test_two_batches' tolerances on the same sample of rows otherwise."""
    n, precision, cap = 300, "f64", 8
    c = R.census_input(1025, 2.4)
    b, v, dt = c["b"][:n], c["v"][:n], DT[precision]
    with handle(b, v, precision) as s:
        batch = s.split_lists_shape(1 << 30, cap)["batch"]
        m = batch + 300
        alike = same_shape(s, m, cap) and same_shape(s, 300, cap)
        print("batch", batch, "m", m, "the same cut as nb_split_force:", alike)
        pts = R.points(n, m, 11).astype(dt)
        got = against_both(s, cap, "two batches", sums_as_bits=alike, points=pts, radius=c["radius"])
    seam = np.arange(batch - 300, m)
    member = R.membership(b, np.asarray(pts[seam], np.float64)[:, :3], np.full(len(seam), np.float64(dt(c["radius"]))))
    rows, count = rows_of(member, cap)
    assert np.array_equal(got["list"][seam], rows) and np.array_equal(got["count"][seam], count)
    assert all(np.isfinite(got[k]).all() and not got[k][:, 3].any() for k in SUMS[:2])
    if not alike:
        pick = np.unique(np.concatenate([np.arange(300), seam, np.random.default_rng(4).integers(0, m, 1000)]))
        ref = R.split_ref(b, None, radius=c["radius"], pts=pts[pick], dtype=dt, terms=False)
        err = R.errors({k: got[k][pick] for k in SUMS[:2]}, ref)
        print("errors", err)
        assert all(e <= R.TOL_F64 for e in err.values()), err


# ---- 7. invariants -----------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECS)
def test_same_request_same_bits_and_host_against_device_pointers(precision):
    c = R.census_input(1025, 2.4)
    n, dt, cap = 1025, DT[precision], 24
    tt = torch.float64 if precision == "f64" else torch.float32
    with hermite(c["b"], c["v"], precision) as s:
        one = against_both(s, cap, "at the bodies", bodies=(0, n), radius=c["radius"])
        two = s.split_lists(bodies=(0, n), radius=c["radius"], cap=cap)
        assert all(one[k].tobytes() == two[k].tobytes() for k in one)
        pone = against_both(s, cap, "at the points", points=c["pts"].astype(dt), point_vel=c["pv"].astype(dt), radius=c["radius"])
        dev = torch.device("cuda", torch.cuda.current_device())
        dp, dv = torch.from_numpy(c["pts"].astype(dt)).to(dev), torch.from_numpy(c["pv"].astype(dt)).to(dev)
        mp = len(c["pts"])

        def outs(m):
            o = {name: torch.empty((m, 4), dtype=tt, device=dev) for name in SUMS}
            o["list"] = torch.full((m, cap), 7, dtype=torch.int32, device=dev)      # (never set beforehand by the call: every element is written)
            o["count"] = torch.empty((m,), dtype=torch.int32, device=dev)
            return o
        po, bo = outs(mp), outs(n)
        torch.cuda.current_stream(dev).synchronize()
        s.split_lists_device(mp, po["list"].data_ptr(), cap, po["count"].data_ptr(), points_ptr=dp.data_ptr(), point_vel_ptr=dv.data_ptr(),
                             radius=c["radius"], **{name + "_ptr": po[name].data_ptr() for name in SUMS})
        s.split_lists_device(0, bo["list"].data_ptr(), cap, bo["count"].data_ptr(), bodies=(0, n), radius=c["radius"],
                             **{name + "_ptr": bo[name].data_ptr() for name in SUMS})
        s.sync()
        for o, w, what in ((po, pone, "points"), (bo, one, "bodies")):
            for k in w:
                assert o[k].cpu().numpy().tobytes() == w[k].tobytes(), ("host against device pointers", what, k)


@pytest.mark.parametrize("kind", ["hermite", "block", "leapfrog"])
def test_stepping_is_bit_identical_around_a_call_and_a_stepped_handle_answers_as_a_fresh_twin(kind):
    n = 1024
    b, v = ic.plummer(n, seed=21)
    kw = {} if kind == "leapfrog" else {"integrator": "hermite4"}
    pts = np.ascontiguousarray(b[:200] + np.float32(0.01))
    pv = None if kind == "leapfrog" else np.ascontiguousarray(v[:200])

    def ask(s):
        return (against_both(s, 16, kind, bodies=(n // 3, 300), radius=0.2), against_both(s, 16, kind, points=pts, point_vel=pv, radius=0.3))

    def run(query):
        with handle(b, v, G=1.0, **kw) as s:
            if kind == "block":
                s.set_block_steps()
            fresh = ask(s) if query else None
            s.simulate(3)
            got = ask(s) if query else None
            state = s.read()
            s.simulate(3)
            return s.read(), state, fresh, got

    plain, mixed = run(False), run(True)
    for x, y in zip(plain[0], mixed[0]):
        assert x.tobytes() == y.tobytes()
    state, fresh, got = mixed[1:]
    with handle(state[0], state[1], G=1.0, **kw) as t:
        want = ask(t)
    for g, w, f in zip(got, want, fresh):
        assert all(g[k].tobytes() == w[k].tobytes() for k in g), kind
        assert all(g[k].tobytes() != f[k].tobytes() for k in SUMS[:2])         # and not the answers of the state before the steps


@pytest.mark.parametrize("shards", [2, 3])
def test_multi_handles(shards):
    n, sp, cap = 1025, 2.4, 24                                            # ragged: the padded system has rows past n, at the origin
    c = R.census_input(n, sp)
    with handle(c["b"], c["v"]) as s:
        want = s.split_lists(bodies=(0, n), radius=c["radius"], cap=cap), s.split_lists(c["pts"], radius=c["radius"], cap=cap)
        far = s.neighbor_lists(np.zeros((1, 4), np.float32), radius=100.0, cap=2048)
    with MultiSimulation(n, shards, eps2=R.EPS2) as m:
        m.init(c["b"], c["v"])
        m.set_params(1e-3, R.G)
        got = m.split_lists(bodies=(0, n), radius=c["radius"], cap=cap), m.split_lists(c["pts"], radius=c["radius"], cap=cap)
        for g, w in zip(got, want):
            assert g["list"].tobytes() == w["list"].tobytes() and g["count"].tobytes() == w["count"].tobytes()
        lists, count = m.neighbor_lists(bodies=(0, n), radius=c["radius"], cap=cap)
        assert got[0]["list"].tobytes() == lists.tobytes() and got[0]["count"].tobytes() == count.tobytes()
        sums = m.split_force(bodies=(0, n), radius=c["radius"])
        ref = c["ref"]
        e = R.entry(n, sp)
        err = R.errors({k: got[0][k] for k in SUMS[:2]}, ref)
        assert all(err[k] <= e[k + "_tol"] for k in err), err
        if all(got[0][k].tobytes() == sums[k].tobytes() for k in sums):
            print("%d shards: the sums are nb_multi_split_force's bits" % shards)
        one = m.split_lists(np.zeros((1, 4), np.float32), radius=100.0, cap=2048)      # the padding rows are nobody's members
        assert one["count"][0] == n == far[1][0] and one["list"].tobytes() == far[0].tobytes()
        with pytest.raises(NBodyError) as ex:
            m.split_lists(bodies=(0, n), radius=c["radius"], jerk=True)
        assert ex.value.code == 1 and "jerk" in str(ex.value) and "nb_multi_split_lists" in str(ex.value)
        with pytest.raises(NBodyError) as ex:
            m.split_lists(bodies=(n - 300, 301), radius=c["radius"])
        assert ex.value.code == 1 and "first_body" in str(ex.value) and "nb_multi_split_lists" in str(ex.value)
        m.simulate(2)


def test_every_invalid_request_is_an_ordinary_error():
    b = load_golden32("plummer1024_bodies0")
    v = load_golden32("plummer1024_vel0")
    L = capi.load_library()
    one = np.zeros((1, 4), np.float32)
    out = np.zeros((1, 4), np.float32)
    lst = np.zeros((1, 4), np.uint32)
    cnt = np.zeros(1, np.uint32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)

    def raw(s, **kw):
        req = capi.nb_split_lists_request()
        req.struct_size = C.sizeof(capi.nb_split_lists_request)
        req.m, req.radius, req.cap = 1, 0.5, 4
        req.points, req.accel_irr, req.list = P(one), P(out), P(lst)
        for name, val in kw.items():
            setattr(req, name, val)
        rc = L.nb_split_lists(s._h, C.byref(req))
        return rc, L.nb_last_error(s._h).decode()

    with Simulation(1024) as s:
        with pytest.raises(NBodyError) as e:             # nothing uploaded
            s.split_lists(one, radius=0.5)
        assert e.value.code == 4 and "upload" in str(e.value) and "nb_split_lists" in str(e.value)
        s.init(b, v)
        with pytest.raises(NBodyError) as e:             # no parameters
            s.split_lists(one, radius=0.5)
        assert e.value.code == 4 and "nb_set_params" in str(e.value) and "nb_split_lists" in str(e.value)
        s.set_params(1e-3, 1.0)
        with pytest.raises(NBodyError) as e:             # the jerk on a leapfrog handle
            s.split_lists(bodies=(0, 1), radius=0.5, jerk=True)
        assert e.value.code == 4 and "Hermite" in str(e.value) and "nb_split_lists" in str(e.value)
        AT = capi.NB_SPLIT_AT_BODIES
        for kw, word in ((dict(struct_size=80), "struct_size"), (dict(struct_size=112), "struct_size"), (dict(m=0), "m must"),
                         (dict(flags=2), "flags"), (dict(flags=8), "flags"), (dict(flags=1 << 31), "flags"),
                         (dict(accel_irr=None), "all NULL"), (dict(accel_irr=None), "nb_neighbor_lists"),
                         (dict(points=None), "points is NULL"), (dict(flags=AT), "points must be NULL"),
                         (dict(flags=AT, points=None, point_vel=P(one)), "point_vel must be NULL"),
                         (dict(point_vel=P(one)), "point_vel must be NULL"), (dict(jerk_irr=P(out)), "point_vel is NULL"),
                         (dict(jerk_reg=P(out)), "point_vel is NULL"),
                         (dict(list=None), "list is NULL"), (dict(cap=0), "cap"), (dict(cap=4097), "cap"), (dict(reserved=1), "reserved"),
                         (dict(flags=AT, points=None, first_body=1024), "first_body"),
                         (dict(flags=AT, points=None, first_body=0xffffffff, m=2), "first_body"),
                         (dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=float("nan")), "radius"),
                         (dict(radius=-1.0, radii=P(one)), "radius")):
            rc, msg = raw(s, **kw)
            assert rc == 1 and "nb_split_lists" in msg and word in msg, (kw, rc, msg)
        assert L.nb_split_lists(s._h, None) == 1
        for args, word in (((0, 4), "m must"), ((1, 0), "cap"), ((1, 4097), "cap")):
            with pytest.raises(NBodyError) as e:
                s.split_lists_shape(*args)
            assert e.value.code == 1 and word in str(e.value) and "nb_split_lists_shape" in str(e.value)
        assert raw(s)[0] == 0                                            # and the same request without a fault is served
        assert raw(s, flags=AT, points=None, first_body=1023)[0] == 0 and raw(s, accel_irr=None, accel_reg=P(out))[0] == 0
        assert raw(s, radius=0.0, radii=P(one))[0] == 0 and not out.any() and (lst == NONE).all()      # radii[0] = 0: no member
        assert raw(s, count=P(cnt), radius=100.0)[0] == 0 and cnt[0] == 1024 and list(lst[0]) == [0, 1, 2, 3]
        assert s.neighbor_scheme_fused is False                          # no scheme on this handle: 0 with NB_OK
        s.simulate(2)                                                    # ... and the handle still steps
    with Simulation(1024, integrator="hermite4") as s:
        s.init(b, v)
        s.set_params(1e-3, 1.0)
        rc, msg = raw(s, jerk_irr=P(out))
        assert rc == 1 and "point_vel is NULL" in msg
        assert raw(s, jerk_reg=P(out), point_vel=P(one))[0] == 0 and raw(s, flags=AT, points=None, jerk_irr=P(out))[0] == 0


# ---- 8. the scheme -----------------------------------------------------------------------------

def scheme_run(n, prec, cap, radius, flags, steps=4):
    b0, v0 = ic.plummer(n, seed=31)
    with Simulation(n, precision=prec, integrator="hermite4", flags=flags) as sim:
        sim.init(b0, v0)
        sim.set_params(1.0 / 512, 1.0)
        sim.set_neighbor_scheme(cap=cap, substeps=2, radius=radius)
        fused = sim.neighbor_scheme_fused
        err = None
        try:
            start = sim.download_neighbor_scheme(cap)
            sim.simulate(steps)
        except NBodyError as e:
            err = (e.code, str(e))
            start = None
        out = [x.tobytes() for x in sim.read()] + [sim.read_jerk().tobytes()] if err is None else []
        if err is None:
            d = sim.download_neighbor_scheme(cap)
            out += [d[k].tobytes() for k in sorted(d)] + [start[k].tobytes() for k in sorted(start)]
        return fused, err, out, sim.neighbor_scheme_stats()


@pytest.mark.parametrize("cap", [24, 100])
@pytest.mark.parametrize("n", [771, 1025])
@pytest.mark.parametrize("prec", PRECS)
def test_the_scheme_gives_the_same_bytes_on_both_routes(prec, n, cap):
    b0, v0 = ic.plummer(n, seed=31)
    with Simulation(n, precision=prec, integrator="hermite4") as sim:      # the largest of these radii whose rows fit cap at the start
        sim.init(b0, v0)
        sim.set_params(1.0 / 512, 1.0)
        for r in (0.4, 0.3, 0.2, 0.15, 0.1, 0.07, 0.05):
            _, count = sim.neighbor_lists(bodies=(0, n), cap=cap, radius=r)
            if count.max() <= cap - cap // 6:                             # (room for what four steps add)
                break
        assert 0 < count.max() <= cap - cap // 6
    one = scheme_run(n, prec, cap, r, 0)
    two = scheme_run(n, prec, cap, r, capi.NB_FLAG_AC_TWO_CALLS)
    print("scheme %s N=%d cap %d radius %.3g:" % (prec, n, cap, r), one[3])
    assert one[0] is True and two[0] is False
    assert one[1] is None and two[1] is None, (one[1], two[1])
    assert len(one[2]) == 16 and one[2] == two[2]
    assert one[3] == two[3] and one[3]["regular_steps"] == 4 and one[3]["builds"] == 5 and one[3]["overflowed"] == 0


@pytest.mark.parametrize("prec", PRECS)
def test_an_overflow_behaves_alike_on_both_routes(prec):
    """At the start (radius 0.3 at cap 2: the triggering call fails, the state is kept) and at a regular time (two clumps closing)."""
    n = 771
    one = scheme_run(n, prec, 2, 0.3, 0)
    two = scheme_run(n, prec, 2, 0.3, capi.NB_FLAG_AC_TWO_CALLS)
    assert one[0] is True and two[0] is False
    assert one[1] is not None and one[1] == two[1] and one[1][0] == 4 and "overflow" in one[1][1]
    assert one[3] == two[3] and one[3]["overflowed"] > 0 and one[3]["regular_steps"] == 0

    rng = np.random.default_rng(9)                                       # two cold clumps of 32 bodies, 1 apart, closing at 8
    b = np.zeros((64, 4), np.float32)
    v = np.zeros((64, 4), np.float32)
    b[:, :3] = rng.normal(0, 0.05, (64, 3))
    b[32:, 0] += 1.0
    b[:, 3] = 1e-6
    v[:32, 0], v[32:, 0] = 4.0, -4.0
    res = []
    for flags in (0, capi.NB_FLAG_AC_TWO_CALLS):
        with Simulation(64, precision=prec, integrator="hermite4", flags=flags) as sim:
            sim.init(b, v)
            sim.set_params(1.0 / 64, 1.0)
            sim.set_neighbor_scheme(radius=0.5, substeps=4, cap=40)
            fused, done, err = sim.neighbor_scheme_fused, 0, None
            try:
                for done in range(16):
                    sim.simulate(1)
            except NBodyError as e:
                err = (e.code, str(e))
            res.append((fused, done, err, [x.tobytes() for x in sim.read()], sim.neighbor_scheme_stats()))
    assert res[0][0] is True and res[1][0] is False
    assert res[0][2] is not None and res[0][2][0] == 4 and "overflow" in res[0][2][1]
    assert res[0][1:] == res[1][1:]
