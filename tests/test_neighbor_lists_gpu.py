"""GPU tests of nb_neighbor_lists: which bodies lie inside a radius of each point, as rows of `cap` ascending indices.

On an integer lattice ([-8, 8]^3: dense enough for rows of dozens of members and for truncation) every difference, product and sum
is exact in binary32, so list and count must EQUAL the int64 brute force of tests/neighbor_lists_ref.py.  On a real distribution:
every j with fp64 d2 < h^2 (1 - tol) is listed, none with d2 >= h^2 (1 + tol), tol = 1e-6 for f32 and 1e-14 for f64 (the bounds of
tests/test_neighbors_gpu.py: 5 * 2^-24 = 3e-7 per distance), the rows ascend, the padding is 0xffffffff and membership is symmetric
(the d2 expression is bitwise symmetric under i <-> j)."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden32, torch
from neighbor_lists_ref import NONE, lattice_lists
from nbody3d_amd import MultiSimulation, Simulation, capi, ic
from nbody3d_amd.capi import NBodyError

pytestmark = pytest.mark.gpu

TOL = {"f32": 1e-6, "f64": 1e-14}
DT = {"f32": np.float32, "f64": np.float64}
SIZES = [1, 2, 7, 255, 256, 257, 1023, 1025, 5000]
CAPS = [1, 16, 128]
REF_CAP = 512                         # the reference rows are computed once at this width: a narrower row is its first entries


def lattice_bodies(n, seed, dtype=np.float32, avoid_origin=False):
    """n bodies at integer coordinates in [-8, 8]^3; from n = 20 on about 5 % of them are moved onto another body."""
    rng = np.random.default_rng(seed)
    b = np.zeros((n, 4), dtype)
    b[:, :3] = rng.integers(-8, 9, (n, 3))
    if avoid_origin:
        b[(b[:, :3] == 0).all(1), 0] = 1
    if n >= 20:
        dup = rng.choice(n, max(1, n // 20), replace=False)
        src = rng.integers(0, n, len(dup))
        b[dup, :3] = b[src, :3]
    b[:, 3] = 1.0 / n
    return b


def lattice_points(b, m, seed):
    """m lattice points; every tenth one coincides with a body."""
    rng = np.random.default_rng(seed)
    p = np.zeros((m, 4), b.dtype)
    p[:, :3] = rng.integers(-8, 9, (m, 3))
    on = np.arange(0, m, 10)
    p[on, :3] = b[rng.integers(0, len(b), len(on)), :3]
    return p


def handle(b, v=None, precision="f32", G=1.0, dt=1e-3, **kw):
    s = Simulation(len(b), precision=precision, **kw)
    s.init(b, np.zeros_like(b) if v is None else v)
    s.set_params(dt, G)
    return s


def same(got, want, cap, what):
    """got = (lists, count) of a request with rows of `cap`; want = the reference at REF_CAP (or at cap itself)."""
    lists, count = got[0], got[1]
    rl, rc = want
    assert lists.dtype == np.uint32 and lists.shape == (len(rc), cap), (what, lists.shape)
    assert count.dtype == np.uint32 and np.array_equal(count, rc), (what, "count", np.flatnonzero(count != rc)[:5])
    w = min(cap, rl.shape[1])
    bad = np.flatnonzero((lists[:, :w] != rl[:, :w]).any(1))
    assert len(bad) == 0, (what, "rows", bad[:5], lists[bad[0]], rl[bad[0]])
    if cap > w:                                  # wider than the reference: no row may hold more than the reference can show
        assert rc.max() <= w and np.all(lists[:, w:] == NONE), what


_ref = {}


def reference(n):
    """Bodies, points, radii and brute-force rows for one lattice size, computed once (float64 arrays: cast per precision)."""
    if n not in _ref:
        b = lattice_bodies(n, n, np.float64)
        pts = lattice_points(b, 1500, 77 + n)
        radii = np.random.default_rng(n).integers(1, 5, 1500)
        own = lattice_lists(b, b, np.full(n, 3), REF_CAP, skip0=0)
        at = lattice_lists(b, pts, radii, REF_CAP)
        assert own[1].max() <= 128 and at[1].max() <= REF_CAP            # cap = 128 holds every row of the bodies' query
        for a in own + at:
            a.setflags(write=False)
        _ref[n] = (b, pts, radii, own, at)
    return _ref[n]


_full5000 = {}


def full_query_5000(precision):
    """The AT_BODIES queries at N = 5000 that several tests look at, run once per precision."""
    if precision not in _full5000:
        b = reference(5000)[0].astype(DT[precision])
        with handle(b, precision=precision) as s:
            out = {cap: s.neighbor_lists(bodies=(0, 5000), radius=3, cap=cap) for cap in CAPS}
            out["part"] = s.neighbor_lists(bodies=(1000, 100), radius=3, cap=128, nearest=True)
            out["full"] = s.neighbor_lists(bodies=(0, 5000), radius=3, cap=128, nearest=True)
            out["nbr"] = s.neighbors(bodies=(0, 5000), radius=3)
            out["shape"] = s.neighbor_lists_shape(5000, 128)
        _full5000[precision] = out
    return _full5000[precision]


# ---- 1. exact answers on the lattice -----------------------------------------------------------

def test_the_lattice_has_the_density_the_cases_rely_on():
    for n, mean, most in ((257, 3.7, 10), (1025, 16.3, 33), (5000, 78.9, 121)):
        count = reference(n)[3][1]
        assert abs(count.mean() - mean) < 0.05 and count.max() == most, (n, count.mean(), count.max())
    assert 0.4 < (reference(1025)[3][1] > 16).mean() < 0.55 and (reference(5000)[3][1] > 16).mean() > 0.99


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_lattice_rows_are_exact(n, precision, cap):
    dt = DT[precision]
    b64, pts64, radii, own, at = reference(n)
    b, pts = b64.astype(dt), pts64.astype(dt)
    if n == 5000:
        out = full_query_5000(precision)
        print("N = 5000 %s: %r" % (precision, out["shape"]))
        assert out["shape"]["chunks"] >= 2 and out["shape"]["j_per_chunk"] % 256 == 0       # rows are stitched across j-chunks
        same(out[cap], own, cap, "bodies")
        with handle(b, precision=precision) as s:
            same(s.neighbor_lists(pts, radii=radii.astype(dt), cap=cap), at, cap, "points")
        return
    with handle(b, precision=precision) as s:
        got = s.neighbor_lists(bodies=(0, n), radius=3, cap=cap, nearest=True)
        same(got, own, cap, "bodies")
        nbr = s.neighbors(bodies=(0, n), radius=3)
        for x, y in zip((got[2], got[3], got[1]), nbr):                  # index, dist2, count: nb_neighbors' bytes
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        if n == 1:
            assert got[0][0, 0] == NONE and got[1][0] == 0 and got[2][0] == NONE and got[3][0] == np.inf
        got = s.neighbor_lists(pts, radii=radii.astype(dt), cap=cap, nearest=True)
        same(got, at, cap, "points")
        nbr = s.neighbors(pts, radii=radii.astype(dt))
        for x, y in zip((got[2], got[3], got[1]), nbr):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_nearest_and_count_are_the_bytes_of_nb_neighbors(precision):
    out = full_query_5000(precision)
    lists, count, index, dist2 = out["full"]
    for x, y in zip((index, dist2, count), out["nbr"]):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    b = load_golden32("plummer1024_bodies0").astype(DT[precision])
    with handle(b, precision=precision) as s:
        lists, count, index, dist2 = s.neighbor_lists(bodies=(0, 1024), radius=0.3, cap=128, nearest=True)
        for x, y in zip((index, dist2, count), s.neighbors(bodies=(0, 1024), radius=0.3)):
            assert x.tobytes() == y.tobytes()
    print("plummer1024 h = 0.3 %s: mean count %.1f, max %d" % (precision, count.mean(), count.max()))
    assert count.max() <= 128


# ---- 2. a real distribution: rounding bounds, order, padding, symmetry -------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_plummer_rows_within_the_rounding_bounds(precision):
    dt, tol, h, cap = DT[precision], TOL[precision], 0.3, 128
    b = load_golden32("plummer1024_bodies0").astype(dt)
    n = len(b)
    with handle(b, precision=precision) as s:
        lists, count = s.neighbor_lists(bodies=(0, n), radius=h, cap=cap)
    x = b[:, :3].astype(np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(d2, np.inf)
    h2 = float(dt(h)) ** 2
    member = np.zeros((n, n), bool)
    kept = lists != NONE
    rows = np.repeat(np.arange(n), kept.sum(1))
    assert lists[kept].max() < n
    member[rows, lists[kept]] = True
    assert count.max() <= cap and np.array_equal(count, kept.sum(1))           # nothing truncated: count == the entries of the row
    assert np.array_equal(kept, np.arange(cap)[None, :] < count[:, None])      # the padding sits behind the members, all of it NONE
    wide = lists.astype(np.int64)
    assert np.all((wide[:, 1:] > wide[:, :-1]) | ~kept[:, 1:])                  # strictly ascending
    missed = (d2 < h2 * (1 - tol)) & ~member
    extra = (d2 >= h2 * (1 + tol)) & member
    print("plummer1024 %s: mean %.1f max %d; missed %d, extra %d (tol %.0e)" % (precision, count.mean(), count.max(), missed.sum(), extra.sum(), tol))
    assert not missed.any() and not extra.any()
    assert not member.diagonal().any() and np.array_equal(member, member.T)     # j in row i <=> i in row j


# ---- 3. independence of m, of the sub-range, of cap ---------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_sub_range_and_narrower_cap_have_the_bits_of_the_full_request(precision):
    out = full_query_5000(precision)
    for x, y in zip(out["full"], out["part"]):
        assert x[1000:1100].tobytes() == y.tobytes()
    assert np.array_equal(out[128][0][:, :16], out[16][0]) and np.array_equal(out[128][0][:, :1], out[1][0])
    assert out[128][1].tobytes() == out[16][1].tobytes() == out[1][1].tobytes()


# ---- 4. batches --------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,m", [("f32", 300000), ("f64", 70000)])
def test_large_m_goes_through_in_batches(precision, m):
    b = reference(257)[0].astype(DT[precision])
    pts = lattice_points(b, m, 10)
    radii = np.random.default_rng(4).integers(1, 5, m)
    with handle(b, precision=precision) as s:
        shape = s.neighbor_lists_shape(m, 4)
        assert shape["batch"] < m, shape                         # more than one batch
        got = s.neighbor_lists(pts, radii=radii.astype(DT[precision]), cap=4)
    same(got, lattice_lists(b, pts, radii, 4), 4, "m = %d" % m)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_the_widest_rows(precision):
    """cap = 4096: rows of 16 KiB.  The batch obeys batch x cap x 4 <= 256 MiB; the answers do not depend on it."""
    b64, pts64, radii, _, at = reference(257)
    b = b64.astype(DT[precision])
    m, cap, limit = 2049, 4096, 256 << 20
    pts = np.concatenate([pts64, pts64[:m - 1500]]).astype(DT[precision])
    rad = np.concatenate([radii, radii[:m - 1500]])
    want = tuple(np.concatenate([a, a[:m - 1500]]) for a in at)
    with handle(b, precision=precision) as s:
        small, big = s.neighbor_lists_shape(m, cap), s.neighbor_lists_shape(70000, cap)
        print(precision, small, big)
        for shape in (small, big):
            assert shape["batch"] * cap * 4 <= limit, shape
        assert big["batch"] < 70000 and big["batch"] % (256 if precision == "f64" else 1024) == 0
        assert s.neighbor_lists_shape(70000, 4)["batch"] >= big["batch"]
        got = s.neighbor_lists(pts, radii=rad.astype(DT[precision]), cap=cap)
    same(got, want, cap, "cap = 4096")


def test_a_host_request_with_wide_rows_is_staged_batch_by_batch():
    """m = 70,000 rows of cap = 4096 (1.1 GB on the host) go through a staging buffer of at most 256 MiB."""
    b64 = reference(257)[0]
    b = b64.astype(np.float32)
    m, cap = 70000, 4096
    with handle(b) as s:
        shape = s.neighbor_lists_shape(m, cap)
        assert shape["batch"] * cap * 4 <= 256 << 20 and shape["batch"] < m, shape
        pts = lattice_points(b, m, 12)
        lists, count = s.neighbor_lists(pts, radius=3, cap=cap)
    rl, rc = lattice_lists(b64, pts, np.full(m, 3), 64)
    assert rc.max() <= 64 and np.array_equal(count, rc) and np.array_equal(lists[:, :64], rl)
    assert lists[:, 64:].min() == NONE


# ---- 5. device pointers ------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_device_pointer_form_equals_the_host_form(precision):
    assert torch is not None
    dt = DT[precision]
    b64, pts64, radii, _, _ = reference(1025)
    b, pts, rad = b64.astype(dt), pts64.astype(dt), radii.astype(dt)
    tt = torch.float64 if precision == "f64" else torch.float32
    stream = torch.cuda.Stream()
    cap = 16
    with handle(b, precision=precision, stream=stream.cuda_stream) as s:
        hp = s.neighbor_lists(pts, radii=rad, cap=cap, nearest=True)
        hb = s.neighbor_lists(bodies=(100, 900), radius=3, cap=cap, nearest=True)
        with torch.cuda.stream(stream):
            tp, tr = torch.from_numpy(pts).to("cuda"), torch.from_numpy(rad).to("cuda")
            outs = []
            for m in (1500, 900):
                outs.append((torch.full((m, cap), 7, device="cuda", dtype=torch.int32), torch.full((m,), 7, device="cuda", dtype=torch.int32),
                             torch.full((m,), 7, device="cuda", dtype=torch.int32), torch.full((m,), 7.0, device="cuda", dtype=tt)))
            s.neighbor_lists_device(tp.data_ptr(), 1500, outs[0][0].data_ptr(), cap, outs[0][1].data_ptr(), outs[0][2].data_ptr(),
                                    outs[0][3].data_ptr(), radii_ptr=tr.data_ptr())
            s.neighbor_lists_device(None, 0, outs[1][0].data_ptr(), cap, outs[1][1].data_ptr(), outs[1][2].data_ptr(),
                                    outs[1][3].data_ptr(), bodies=(100, 900), radius=3)
        stream.synchronize()
        for host, dev in ((hp, outs[0]), (hb, outs[1])):
            for x, y in zip(host, dev):
                assert x.tobytes() == y.cpu().numpy().tobytes()
            assert (host[1] > cap).any() and (host[1] < cap).any()               # truncated rows and padded rows, both defined


# ---- 6. the state is untouched -----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["symmetric", "hermite"])
def test_stepping_is_bit_identical_with_a_list_call_in_between(kind):
    n = 8192 if kind == "symmetric" else 1025
    b, v = ic.plummer(n, seed=21)
    kw = {"integrator": "hermite4"} if kind == "hermite" else {}

    def run(query):
        with handle(b, v, G=0.37, **kw) as s:
            s.simulate(3)
            if query:
                lists, count = s.neighbor_lists(bodies=(0, n), radius=0.1, cap=16)
                assert count.max() > 0
            s.simulate(3)
            return s.read() + (s.variant,)

    plain, mixed = run(False), run(True)
    print(kind, plain[3])
    if kind == "symmetric":
        assert "sym" in plain[3], plain[3]
    for x, y in zip(plain[:3], mixed[:3]):
        assert x.tobytes() == y.tobytes()


# ---- 7. shards ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shards", [2, 3])
def test_multi_handles_list_only_the_callers_rows(shards):
    n = 5000
    b = lattice_bodies(n, 5001, np.float32, avoid_origin=True)       # no body AT the origin, where the padding rows sit
    pts = lattice_points(b, 600, 5)
    pts[0, :3] = 0
    radii = np.random.default_rng(6).integers(1, 5, 600)
    radii[0] = 4
    with handle(b) as s:
        single = s.neighbor_lists(bodies=(0, n), radius=3, cap=128, nearest=True) + s.neighbor_lists(pts, radii=radii.astype(np.float32), cap=16, nearest=True)
    same(single[4:6], lattice_lists(b, pts, radii, 16), 16, "single, points")
    with MultiSimulation(n, shards) as m:
        m.init(b, np.zeros_like(b))
        m.set_params(1e-3, 1.0)
        multi = m.neighbor_lists(bodies=(0, n), radius=3, cap=128, nearest=True) + m.neighbor_lists(pts, radii=radii.astype(np.float32), cap=16, nearest=True)
        for lists in (multi[0], multi[4]):
            assert lists[lists != NONE].max() < n                    # never a padding row
        for x, y in zip(single, multi):
            assert x.tobytes() == y.tobytes()
        with pytest.raises(NBodyError) as e:
            m.neighbor_lists(bodies=(n - 300, 301), radius=3)        # row n exists in the padded system, not in the caller's
        assert e.value.code == 1 and "first_body" in str(e.value) and "nb_multi_neighbor_lists" in str(e.value)
        m.simulate(2)


# ---- 8. errors ---------------------------------------------------------------------------------

def test_every_invalid_request_is_an_ordinary_error():
    b = load_golden32("plummer1024_bodies0")
    v = load_golden32("plummer1024_vel0")
    L = capi.load_library()
    one = np.zeros((1, 4), np.float32)
    rad = np.ones(1, np.float32)
    lst = np.zeros(8, np.uint32)

    def raw(s, **kw):
        req = capi.nb_neighbor_list_request()
        req.struct_size = C.sizeof(capi.nb_neighbor_list_request)
        req.m = 1
        req.points = one.ctypes.data_as(C.c_void_p)
        req.list = lst.ctypes.data_as(C.c_void_p)
        req.cap = 8
        req.radius = 0.5
        for k, val in kw.items():
            setattr(req, k, val)
        rc = L.nb_neighbor_lists(s._h, C.byref(req))
        return rc, L.nb_last_error(s._h).decode()

    rptr = rad.ctypes.data_as(C.c_void_p)
    with Simulation(1024) as s:
        with pytest.raises(NBodyError) as e:             # nothing uploaded
            s.neighbor_lists(one, radius=0.5)
        assert e.value.code == 4 and "upload" in str(e.value) and "nb_neighbor_lists" in str(e.value)
        s.init(b, v)
        assert s.neighbor_lists(one, radius=0.5)[1][0] > 0        # nb_set_params is not required
        for kw, word in ((dict(bodies=(0, 0), radius=1.0), "m must"), (dict(bodies=(1000, 25), radius=1.0), "first_body"),
                         (dict(points=one, bodies=(0, 1), radius=1.0), "points must be NULL"), (dict(radius=1.0), "points is NULL"),
                         (dict(points=one, radius=-1.0), "radius"), (dict(points=one, radius=float("nan")), "radius"),
                         (dict(points=one, radius=0.0), "need radii or radius"), (dict(points=one), "need radii or radius"),
                         (dict(points=one, radius=1.0, cap=0), "cap"), (dict(points=one, radius=1.0, cap=4097), "cap")):
            with pytest.raises(NBodyError) as e:
                s.neighbor_lists(**kw)
            assert e.value.code == 1 and word in str(e.value), (kw, str(e.value))
        with pytest.raises(NBodyError) as e:
            s.neighbor_lists(np.zeros((0, 4), np.float32), radius=1.0)
        assert e.value.code == 1
        with pytest.raises(NBodyError) as e:
            s.neighbor_lists_shape(10, 0)
        assert e.value.code == 1 and "cap" in str(e.value)
        AT = capi.NB_NBR_AT_BODIES
        for kw, word in ((dict(struct_size=72), "struct_size"), (dict(struct_size=88), "struct_size"), (dict(flags=2), "flags"),
                         (dict(flags=8), "flags"), (dict(flags=1 << 31), "flags"), (dict(m=0), "m must"),
                         (dict(list=None), "list"), (dict(points=None), "points is NULL"), (dict(flags=AT), "points must be NULL"),
                         (dict(flags=AT, points=None, first_body=1024), "first_body"),
                         (dict(flags=AT, points=None, first_body=0xffffffff, m=2), "first_body"),
                         (dict(cap=0), "cap"), (dict(cap=4097), "cap"), (dict(reserved=1), "reserved"),
                         (dict(radius=0.0), "need radii or radius"), (dict(radius=-0.5), "radius"), (dict(radius=float("nan")), "radius"),
                         (dict(radii=rptr, radius=-1.0), "radius")):
            rc, msg = raw(s, **kw)
            assert rc == 1 and "nb_neighbor_lists" in msg and word in msg, (kw, rc, msg)
        assert L.nb_neighbor_lists(s._h, None) == 1
        assert raw(s)[0] == 0                                          # and the same request without a fault is served
        assert raw(s, radii=rptr, radius=0.0)[0] == 0 and raw(s, cap=1)[0] == 0
        s.set_params(1e-3, 1.0)
        s.simulate(2)                                                  # ... and the handle still steps


# ---- 9. all close pairs ------------------------------------------------------------------------

def test_all_close_pairs_are_the_brute_force_pairs():
    b = reference(1025)[0].astype(np.float32)
    x = b[:, :3].astype(np.int64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2)
    i, j = np.nonzero(np.triu(d2 < 9, 1))
    with handle(b) as s:
        pairs = s.all_close_pairs(3, cap=64)
        assert pairs.dtype == np.uint32 and np.array_equal(pairs, np.stack([i, j], 1))
        with pytest.raises(ValueError):
            s.all_close_pairs(3, cap=16)                               # half the rows hold more than 16
