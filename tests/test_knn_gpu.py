"""GPU tests of nb_knn: the k nearest bodies of each point, rows of k (index, dist2) in the order (d2 ascending, then j ascending).

On an integer lattice ([-8, 8]^3 with 5 % duplicated positions: equal distances and d2 = 0 neighbours everywhere) every difference,
product and sum is exact in binary32, so index and dist2 must EQUAL the int64 brute force of tests/knn_ref.py, padding included.  On
a real distribution: the rows ascend in (d2, j), each dist2 is within tol of the fp64 d2 of its index and no body outside a row has an
fp64 d2 below d_k (1 - tol), tol = 1e-6 for f32 and 1e-14 for f64 (the bounds of tests/test_neighbors_gpu.py: 5 * 2^-24 = 3e-7 per
distance).  Column 0 is nb_neighbors' answer and the members of a radius are nb_neighbor_lists' rows, bit for bit: the three calls
share one d2 expression."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden32, torch
from knn_ref import NONE, lattice_knn
from nbody3d_amd import MultiSimulation, Simulation, capi, ic
from nbody3d_amd.capi import NBodyError

pytestmark = pytest.mark.gpu

TOL = {"f32": 1e-6, "f64": 1e-14}
DT = {"f32": np.float32, "f64": np.float64}
SIZES = [1, 2, 7, 255, 256, 257, 1023, 1025, 5000]
KS = [1, 6, 32, 64]
M_PTS = 1500


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


def same(got, want, k, what, rows=None):
    """got = (index, dist2) of a request for k neighbours; want = the reference at k = 64 (a shorter row is its first entries)."""
    index, dist2 = got
    ri, rd = want[0][:, :k], want[1][:, :k]
    if rows is not None:
        index, dist2 = index[rows], dist2[rows]
    assert index.dtype == np.uint32 and index.shape == ri.shape, (what, index.shape, ri.shape)
    bad = np.flatnonzero((index != ri).any(1))
    assert len(bad) == 0, (what, "index rows", bad[:5], index[bad[0]], ri[bad[0]])
    bad = np.flatnonzero((dist2.astype(np.float64) != rd).any(1))
    assert len(bad) == 0, (what, "dist2 rows", bad[:5], dist2[bad[0]], rd[bad[0]])


_ref = {}


def reference(n):
    """Bodies, points and brute-force rows (k = 64) for one lattice size, computed once (float64 arrays: cast per precision)."""
    if n not in _ref:
        b = lattice_bodies(n, n, np.float64)
        pts = lattice_points(b, M_PTS, 77 + n)
        own = lattice_knn(b, b, 64, skip0=0)
        at = lattice_knn(b, pts, 64)
        for a in own + at:
            a.setflags(write=False)
        _ref[n] = (b, pts, own, at)
    return _ref[n]


_full5000 = {}


def full_query_5000(precision):
    """The AT_BODIES queries at N = 5000 that several tests look at, run once per precision."""
    if precision not in _full5000:
        b = reference(5000)[0].astype(DT[precision])
        with handle(b, precision=precision) as s:
            out = {k: s.knn(bodies=(0, 5000), k=k) for k in KS}
            out["part"] = s.knn(bodies=(1000, 100), k=64)
            out["nbr"] = s.neighbors(bodies=(0, 5000))
            out["shape"] = s.knn_shape(5000, 64)
        _full5000[precision] = out
    return _full5000[precision]


# ---- 1. exact answers on the lattice -----------------------------------------------------------

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_lattice_rows_are_exact(n, precision, k):
    dt = DT[precision]
    b64, pts64, own, at = reference(n)
    b, pts = b64.astype(dt), pts64.astype(dt)
    if n == 5000:
        out = full_query_5000(precision)
        print("N = 5000 %s: %r" % (precision, out["shape"]))
        assert out["shape"]["chunks"] >= 2 and out["shape"]["j_per_chunk"] % 256 == 0       # rows are merged across j-chunks
        same(out[k], own, k, "bodies")
        with handle(b, precision=precision) as s:
            same(s.knn(pts, k=k), at, k, "points")
        return
    with handle(b, precision=precision) as s:
        got = s.knn(bodies=(0, n), k=k)
        assert got[1].dtype == dt
        same(got, own, k, "bodies")
        if n - 1 < k:                                                    # short rows: padded, all of them defined
            assert np.all(got[0][:, n - 1:] == NONE) and np.all(np.isposinf(got[1][:, n - 1:]))
        got = s.knn(pts, k=k)
        same(got, at, k, "points")
        if n < k:
            assert np.all(got[0][:, n:] == NONE) and np.all(np.isposinf(got[1][:, n:])) and np.all(got[0][:, :n] != NONE)
        only_index = s.knn(pts, k=k, dist2=False)
        assert only_index[1] is None and only_index[0].tobytes() == got[0].tobytes()


# ---- 2. independence of k, of the sub-range -----------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_shorter_rows_and_sub_ranges_have_the_bits_of_the_full_request(precision):
    out = full_query_5000(precision)
    for k in (1, 6, 32):
        for x, y in zip(out[64], out[k]):
            assert np.ascontiguousarray(x[:, :k]).tobytes() == y.tobytes(), k
    for x, y in zip(out[64], out["part"]):
        assert x[1000:1100].tobytes() == y.tobytes()


# ---- 3. against nb_neighbors and nb_neighbor_lists ----------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_column_0_is_the_bytes_of_nb_neighbors(precision):
    out = full_query_5000(precision)
    for k in KS:
        for x, y in zip(out[k], out["nbr"][:2]):
            assert x.dtype == y.dtype and np.ascontiguousarray(x[:, 0]).tobytes() == y.tobytes(), k
    b = load_golden32("plummer1024_bodies0").astype(DT[precision])
    pts = np.random.default_rng(3).normal(0, 1, (300, 4)).astype(DT[precision])
    with handle(b, precision=precision) as s:
        for kw in (dict(bodies=(0, 1024)), dict(points=pts)):
            nbr = s.neighbors(**kw)
            for k in (1, 32):
                got = s.knn(k=k, **kw)
                for x, y in zip(got, nbr[:2]):
                    assert np.ascontiguousarray(x[:, 0]).tobytes() == y.tobytes(), (k, list(kw))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_the_members_of_a_radius_are_the_rows_of_nb_neighbor_lists(precision):
    dt = DT[precision]
    b = load_golden32("plummer1024_bodies0").astype(dt)
    n = len(b)
    x = b[:, :3].astype(np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(d2, np.inf)
    h = float(np.sqrt(np.sort(d2, axis=None)[10 * n]))                  # the radius that gives a mean count of 10
    with handle(b, precision=precision) as s:
        lists, count = s.neighbor_lists(bodies=(0, n), radius=h, cap=128)
        index, dist2 = s.knn(bodies=(0, n), k=32)
    rows = np.flatnonzero(count <= 32)
    print("plummer1024 %s: h = %.4f, mean count %.2f, %d rows with count <= 32" % (precision, h, count.mean(), len(rows)))
    assert 9.5 < count.mean() < 10.5 and len(rows) > n // 2
    for r in rows:
        c = int(count[r])
        assert np.sort(index[r, :c]).tobytes() == lists[r, :c].tobytes(), r
        hh = dt(h) * dt(h)
        assert np.all(dist2[r, :c] < hh) and (c == 32 or dist2[r, c] >= hh), r


# ---- 4. a real distribution: order and rounding bounds ------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name", ["plummer1024", "galaxy_ref"])
def test_rows_within_the_rounding_bounds(name, precision):
    dt, tol, k = DT[precision], TOL[precision], 32
    b = load_golden32(name + "_bodies0").astype(dt)
    n = len(b)
    with handle(b, precision=precision) as s:
        index, dist2 = s.knn(bodies=(0, n), k=k)
    assert index.max() < n and not (index == np.arange(n)[:, None]).any()
    assert all(len(set(row)) == k for row in index.tolist())                     # k different bodies
    d = dist2.astype(np.float64)
    j = index.astype(np.int64)
    step_d, step_j = np.diff(d, axis=1), np.diff(j, axis=1)
    assert np.all((step_d > 0) | ((step_d == 0) & (step_j > 0)))                # ascending in (d2, j)
    x = b[:, :3].astype(np.float64)
    full = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(full, np.inf)
    true = np.take_along_axis(full, j, axis=1)
    err = np.abs(d - true) / np.where(true > 0, true, 1.0)
    outside = full.copy()
    np.put_along_axis(outside, j, np.inf, axis=1)
    missed = outside < (d[:, k - 1] * (1 - tol))[:, None]
    print("%s %s: worst dist2 error %.2e, bodies missed %d (tol %.0e)" % (name, precision, err.max(), missed.sum(), tol))
    assert err.max() <= tol
    assert not missed.any()


# ---- 5. batches --------------------------------------------------------------------------------

def batches(s, m, k):
    """The (first row, rows) of the batches an m-point request goes through: nb_knn_shape's batch, the last one what is left."""
    batch = s.knn_shape(m, k)["batch"]
    return [(b0, min(batch, m - b0)) for b0 in range(0, m, batch)]


def batch_rows(m, cuts, seed):
    """4,096 rows at random plus the first and the last row of every batch."""
    edges = [r for b0, rows in cuts for r in (b0, b0 + rows - 1)]
    sample = np.random.default_rng(seed).choice(m, 4096, replace=False)
    return np.unique(np.concatenate([sample, edges]))


@pytest.mark.parametrize("extra", [1, 1025])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_large_m_goes_through_in_batches(precision, extra):
    b64 = reference(257)[0]
    b = b64.astype(DT[precision])
    k = 32
    with handle(b, precision=precision) as s:
        batch = s.knn_shape(1 << 22, k)["batch"]
        assert batch == (65536 if precision == "f64" else 262144)
        m = batch + extra
        cuts = batches(s, m, k)
        assert cuts == [(0, batch), (batch, extra)], cuts               # more than one batch
        pts = lattice_points(b, m, 10)
        got = s.knn(pts, k=k)
    rows = batch_rows(m, cuts, 5)
    same(got, lattice_knn(b64, pts[rows], k), k, "m = %d" % m, rows=rows)


def test_the_memory_rule_cuts_the_batch_for_wide_rows():
    """k = 64 against 6,144 bodies in 3 j-chunks: 3 x 262,144 x 64 x 8 bytes are more than 256 MiB, so the batch is halved."""
    n, k, limit = 6144, 64, 256 << 20
    b64 = lattice_bodies(n, 6144, np.float64)
    b = b64.astype(np.float32)
    with handle(b) as s:
        narrow, wide = s.knn_shape(300000, 6), s.knn_shape(300000, k)
        print(narrow, wide)
        assert narrow["batch"] == 262144 and narrow["chunks"] * narrow["batch"] * k * 8 > limit
        assert wide["batch"] < narrow["batch"] and wide["batch"] % 1024 == 0 and wide["chunks"] == narrow["chunks"] >= 2
        assert wide["chunks"] * wide["batch"] * k * 8 <= limit
        m = 300000
        cuts = batches(s, m, k)
        print(cuts)
        assert cuts[0] == (0, wide["batch"]) and len(cuts) >= 3
        assert s.knn_shape(m, k) == wide and [rows for _, rows in cuts] == [131072, 131072, 37856]
        pts = lattice_points(b, m, 12)
        got = s.knn(pts, k=k)
    rows = batch_rows(m, cuts, 6)
    same(got, lattice_knn(b64, pts[rows], k), k, "k = 64, m = %d" % m, rows=rows)


# ---- 6. device pointers ------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_device_pointer_form_equals_the_host_form(precision):
    assert torch is not None
    dt = DT[precision]
    b64, pts64, _, _ = reference(1025)
    b, pts = b64.astype(dt), pts64.astype(dt)
    tt = torch.float64 if precision == "f64" else torch.float32
    stream = torch.cuda.Stream()
    k = 6
    with handle(b, precision=precision, stream=stream.cuda_stream) as s:
        hp = s.knn(pts, k=k)
        hb = s.knn(bodies=(100, 900), k=k)
        with torch.cuda.stream(stream):
            tp = torch.from_numpy(pts).to("cuda")
            outs = [(torch.full((m, k), 7, device="cuda", dtype=torch.int32), torch.full((m, k), 7.0, device="cuda", dtype=tt))
                    for m in (M_PTS, 900, 900)]
            s.knn_device(tp.data_ptr(), M_PTS, k, outs[0][0].data_ptr(), outs[0][1].data_ptr())
            s.knn_device(None, 0, k, outs[1][0].data_ptr(), outs[1][1].data_ptr(), bodies=(100, 900))
            s.knn_device(None, 0, k, None, outs[2][1].data_ptr(), bodies=(100, 900))       # dist2 only: index is not written
        stream.synchronize()
        for host, dev in ((hp, outs[0]), (hb, outs[1])):
            for x, y in zip(host, dev):
                assert x.tobytes() == y.cpu().numpy().tobytes()
        assert outs[2][1].cpu().numpy().tobytes() == hb[1].tobytes() and bool((outs[2][0] == 7).all())


# ---- 7. the state is untouched -----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["symmetric", "fused", "hermite"])
def test_stepping_is_bit_identical_with_a_knn_call_in_between(kind):
    n = 4096 if kind == "symmetric" else 1024
    b, v = ic.plummer(n, seed=21)
    kw = {"integrator": "hermite4"} if kind == "hermite" else {"force_variant": 708013} if kind == "symmetric" else {}

    def run(query):
        with handle(b, v, G=0.37, **kw) as s:
            s.simulate(3)
            if query:
                index, dist2 = s.knn(bodies=(0, n), k=6)
                assert index.max() < n and np.isfinite(dist2).all()
                s.knn(b[:100], k=64)
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
def test_multi_handles_return_only_the_callers_rows(shards):
    n = 1000
    b = lattice_bodies(n, 1001, np.float32, avoid_origin=True)       # no body AT the origin, where the padding rows sit
    pts = lattice_points(b, 600, 5)
    pts[0, :3] = 0
    with handle(b) as s:
        single = s.knn(bodies=(0, n), k=32) + s.knn(pts, k=64)
    same(single[2:], lattice_knn(b, pts, 64), 64, "single, points")
    with MultiSimulation(n, shards) as m:
        m.init(b, np.zeros_like(b))
        m.set_params(1e-3, 1.0)
        multi = m.knn(bodies=(0, n), k=32) + m.knn(pts, k=64)
        for index in (multi[0], multi[2]):
            assert index.max() < n                                   # never a padding row (and no row is short)
        for x, y in zip(single, multi):
            assert x.tobytes() == y.tobytes()
        with pytest.raises(NBodyError) as e:
            m.knn(bodies=(n - 300, 301), k=6)                        # row n exists in the padded system, not in the caller's
        assert e.value.code == 1 and "first_body" in str(e.value) and "nb_multi_knn" in str(e.value)
        m.simulate(2)


# ---- 9. errors ---------------------------------------------------------------------------------

def test_every_invalid_request_is_an_ordinary_error():
    b = load_golden32("plummer1024_bodies0")
    v = load_golden32("plummer1024_vel0")
    L = capi.load_library()
    one = np.zeros((1, 4), np.float32)
    idx = np.zeros(8, np.uint32)

    def raw(s, **kw):
        req = capi.nb_knn_request()
        req.struct_size = C.sizeof(capi.nb_knn_request)
        req.m = 1
        req.points = one.ctypes.data_as(C.c_void_p)
        req.index = idx.ctypes.data_as(C.c_void_p)
        req.k = 8
        for name, val in kw.items():
            setattr(req, name, val)
        rc = L.nb_knn(s._h, C.byref(req))
        return rc, L.nb_last_error(s._h).decode()

    with Simulation(1024) as s:
        with pytest.raises(NBodyError) as e:             # nothing uploaded
            s.knn(one)
        assert e.value.code == 4 and "upload" in str(e.value) and "nb_knn" in str(e.value)
        s.init(b, v)
        assert s.knn(one)[0][0, 0] < 1024                # nb_set_params is not required
        for kw, word in ((dict(bodies=(0, 0)), "m must"), (dict(bodies=(1000, 25)), "first_body"),
                         (dict(points=one, bodies=(0, 1)), "points must be NULL"), (dict(), "points is NULL"),
                         (dict(points=one, k=0), "k must"), (dict(points=one, k=65), "k must")):
            with pytest.raises(NBodyError) as e:
                s.knn(**kw)
            assert e.value.code == 1 and word in str(e.value) and "nb_knn" in str(e.value), (kw, str(e.value))
        with pytest.raises(NBodyError) as e:
            s.knn(np.zeros((0, 4), np.float32))
        assert e.value.code == 1
        for k in (0, 65):
            with pytest.raises(NBodyError) as e:
                s.knn_shape(10, k)
            assert e.value.code == 1 and "k must" in str(e.value) and "nb_knn_shape" in str(e.value)
        with pytest.raises(NBodyError) as e:
            s.knn_shape(0, 6)
        assert e.value.code == 1 and "m must" in str(e.value)
        AT = capi.NB_NBR_AT_BODIES
        for kw, word in ((dict(struct_size=40), "struct_size"), (dict(struct_size=56), "struct_size"), (dict(flags=2), "flags"),
                         (dict(flags=8), "flags"), (dict(flags=1 << 31), "flags"), (dict(m=0), "m must"),
                         (dict(index=None), "both NULL"), (dict(points=None), "points is NULL"), (dict(flags=AT), "points must be NULL"),
                         (dict(flags=AT, points=None, first_body=1024), "first_body"),
                         (dict(flags=AT, points=None, first_body=0xffffffff, m=2), "first_body"),
                         (dict(k=0), "k must"), (dict(k=65), "k must"), (dict(k=0xffffffff), "k must"), (dict(reserved=1), "reserved")):
            rc, msg = raw(s, **kw)
            assert rc == 1 and "nb_knn" in msg and word in msg, (kw, rc, msg)
        assert L.nb_knn(s._h, None) == 1
        assert raw(s)[0] == 0                                          # and the same request without a fault is served
        assert raw(s, k=1)[0] == 0 and raw(s, flags=AT, points=None, first_body=1023)[0] == 0
        s.set_params(1e-3, 1.0)
        s.simulate(2)                                                  # ... and the handle still steps


# ---- 10. the density helpers -------------------------------------------------------------------

def test_local_density_and_density_center():
    b64, _, own, _ = reference(1025)
    with handle(b64.astype(np.float32)) as s:
        rho = s.local_density(6)
    want = capi.density_from_knn(b64.astype(np.float32), own[0][:, :6], own[1][:, :6])      # the masses as the handle holds them
    assert rho.dtype == np.float64 and rho.shape == (1025,) and not np.isnan(want).any()
    assert np.array_equal(rho, want)
    b, v = ic.plummer(4096, seed=7)
    with handle(b, v) as s:
        c = s.density_center(6)
        assert np.isnan(Simulation.local_density(s, 64)).sum() == 0
    print("density centre of plummer(4096, seed=7):", c)
    assert c.shape == (3,) and np.linalg.norm(c) < 0.05
    with handle(b64[:5].astype(np.float32)) as s:
        assert np.isnan(s.local_density(6)).all()                      # n - 1 < k: no body has a 6th neighbour


# ---- 11. the shape of a request ----------------------------------------------------------------

STATS_CHILD = """
import ctypes as C, json, sys
import numpy as np
sys.path[:0] = [%(tests)r]
import conftest                                     # torch first, the paths
from nbody3d_amd import Simulation, capi
from test_knn_gpu import lattice_bodies, lattice_points
L = capi.load_library()
L.nb_tuning_knn_stats.argtypes = [C.c_void_p, C.c_int]
L.nb_tuning_knn_stats.restype = None
out = {}
for precision, n, m, k in (("f32", 6144, 300000, 64), ("f64", 257, 66561, 32)):
    dt = np.float64 if precision == "f64" else np.float32
    b = lattice_bodies(n, n, dt)
    with Simulation(n, precision=precision) as s:
        s.init(b, np.zeros_like(b))
        shape = s.knn_shape(m, k)
        L.nb_tuning_knn_stats(None, 1)
        s.knn(lattice_points(b, m, 12), k=k)
        c = (C.c_uint64 * 5)()
        L.nb_tuning_knn_stats(c, 1)
        out[precision] = {"shape": shape, "m": m, "point_chunk_rows": int(c[0])}
print(json.dumps(out))
"""


def test_every_batch_of_a_request_runs_the_chunks_of_its_shape():
    """The calibration build counts the (point, chunk) rows its passes leave: chunks x m when every batch of a cut request -- the
    last, shorter one included -- runs against the chunks nb_knn_shape reports, more when a later batch is cut into its own."""
    import json
    import os
    import subprocess
    import sys
    from conftest import PKG, ROOT
    env = dict(os.environ, NB_ENGINE_LIB=os.path.join(PKG, "csrc", "libnbody3d_hip_tuning.so"), NB_KNN_STATS="1")
    p = subprocess.run([sys.executable, "-c", STATS_CHILD % {"tests": os.path.join(ROOT, "tests")}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    print(res)
    for precision, r in res.items():
        assert r["shape"]["batch"] < r["m"], r                          # more than one batch
        assert r["point_chunk_rows"] == r["shape"]["chunks"] * r["m"], (precision, r)
    assert res["f32"]["shape"]["chunks"] == 3 and res["f32"]["shape"]["batch"] == 131072


def test_few_points_against_millions_of_bodies():
    """One point block against 4,194,304 bodies: nb_neighbors' rule would cut j into 2,048 chunks; nb_knn keeps at most 512 (its
    merge holds 64 bytes of LDS per chunk) and serves the request -- 64 neighbours at d2 = 0 and 1 on a lattice that dense, so the
    order is decided by j across every chunk."""
    n, k = 1 << 22, 64
    b = lattice_bodies(n, 22, np.float32)
    pts = lattice_points(b, 2, 23)
    with Simulation(n, layer_budget_mib=1) as s:
        s.init(b, np.zeros_like(b))
        shape, nbr = s.knn_shape(2, k), s.neighbors_shape(2)
        print(shape, nbr)
        assert nbr["chunks"] > 512 and 256 < shape["chunks"] <= 512 and shape["j_per_chunk"] % 256 == 0
        assert shape["chunks"] * shape["j_per_chunk"] >= n
        got = s.knn(pts, k=k) + s.knn(bodies=(n - 2, 2), k=k)
    same(got[:2], lattice_knn(b, pts, k), k, "points")
    same(got[2:], lattice_knn(b, b[n - 2:], k, skip0=n - 2), k, "bodies")
