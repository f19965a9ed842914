"""GPU tests of nb_neighbors: the nearest body of each point, its squared distance and the number of bodies inside a radius.

On an integer lattice ([-64, 64]^3) every difference, product and sum is exact in binary32, so index, dist2 and count must EQUAL
the int64 brute force of tests/neighbors_ref.py -- the smallest index among the many equal distances included.  On the real
distributions: d2_64(j*) <= (1 + tol) min_j d2_64(j), |dist2 - d2_64(j*)| <= tol d2_64(j*), and the count between the brute-force
counts at h^2 (1 -+ tol); tol = 1e-6 for f32 (three differences, three squares, two sums: 5 * 2^-24 = 3e-7 per candidate, so two
candidates can swap inside 6e-7), 1e-14 for f64."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import load_golden32, torch
from neighbors_ref import NONE, check_float, lattice_ref
from nbody3d_amd import MultiSimulation, Simulation, capi, ic
from nbody3d_amd.capi import NBodyError

pytestmark = pytest.mark.gpu

TOL = {"f32": 1e-6, "f64": 1e-14}
DT = {"f32": np.float32, "f64": np.float64}
SIZES = [1, 2, 7, 255, 256, 257, 1023, 1025, 5000]


def lattice_bodies(n, seed, dtype=np.float32, avoid_origin=False):
    """n bodies at integer coordinates in [-64, 64]^3; from n = 20 on about 5 % of them sit exactly on another body."""
    rng = np.random.default_rng(seed)
    b = np.zeros((n, 4), dtype)
    b[:, :3] = rng.integers(-64, 65, (n, 3))
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
    p[:, :3] = rng.integers(-64, 65, (m, 3))
    on = np.arange(0, m, 10)
    p[on, :3] = b[rng.integers(0, len(b), len(on)), :3]
    return p


def handle(b, v=None, precision="f32", G=1.0, dt=1e-3, **kw):
    s = Simulation(len(b), precision=precision, **kw)
    s.init(b, np.zeros_like(b) if v is None else v)
    s.set_params(dt, G)
    return s


def same(got, want, what):
    index, dist2, count = got
    ri, rd, rc = want
    assert index.dtype == np.uint32 and np.array_equal(index, ri), (what, "index", np.flatnonzero(index != ri)[:5])
    assert np.array_equal(dist2.astype(np.float64), rd), (what, "dist2", np.flatnonzero(dist2 != rd)[:5])
    if rc is None:
        assert count is None
    else:
        assert count.dtype == np.uint32 and np.array_equal(count, rc), (what, "count", np.flatnonzero(count != rc)[:5])


_full5000 = {}


def full_query_5000(precision):
    """The AT_BODIES query over all rows at N = 5000 and its brute force, computed once per precision."""
    if precision not in _full5000:
        b = lattice_bodies(5000, 5000, DT[precision])
        with handle(b, precision=precision) as s:
            got = s.neighbors(bodies=(0, 5000), radius=3)
            part = s.neighbors(bodies=(1000, 100), radius=3)
            shape = s.neighbors_shape(5000)
        _full5000[precision] = (b, got, part, shape, lattice_ref(b, b, np.full(5000, 3), skip0=0))
    return _full5000[precision]


# ---- 1. exact answers on the lattice -----------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_lattice_answers_are_exact(n, precision):
    dt = DT[precision]
    if n == 5000:
        b, got, _, shape, want = full_query_5000(precision)
        print("N = 5000 %s: %r" % (precision, shape))
        assert shape["chunks"] >= 2 and shape["j_per_chunk"] % 256 == 0          # more than one j-chunk: the reduce kernel decides ties
        same(got, want, "bodies")
        with handle(b, precision=precision) as s:
            pts = lattice_points(b, 1500, 77)
            radii = np.random.default_rng(3).integers(1, 7, 1500)
            got = s.neighbors(pts, radii=radii.astype(dt))
        same(got, lattice_ref(b, pts, radii), "points")
        return
    b = lattice_bodies(n, n, dt)
    with handle(b, precision=precision) as s:
        got = s.neighbors(bodies=(0, n), radius=3)
        assert got[1].dtype == dt
        if n == 1:
            assert got[0][0] == NONE and got[1][0] == np.inf and got[2][0] == 0
        same(got, lattice_ref(b, b, np.full(n, 3), skip0=0), "bodies")
        pts = lattice_points(b, 1500, 77 + n)
        radii = np.random.default_rng(n).integers(1, 7, 1500)
        got = s.neighbors(pts, radii=radii.astype(dt))
        want = lattice_ref(b, pts, radii)
        same(got, want, "points")
        on = np.arange(0, 1500, 10)
        assert np.all(got[1][on] == 0)                          # a coinciding body is found at d2 = 0
        index, dist2, count = s.neighbors(pts[:40])              # no radius: no count, the same nearest
        assert count is None and np.array_equal(index, want[0][:40]) and np.array_equal(dist2, want[1][:40])


# ---- 2. batching, independence of m ------------------------------------------------------------

@pytest.mark.parametrize("precision,m", [("f32", 300000), ("f64", 70000)])
def test_large_m_goes_through_in_batches(precision, m):
    b = lattice_bodies(257, 9, DT[precision])
    pts = lattice_points(b, m, 10)
    radii = np.random.default_rng(4).integers(1, 7, m)
    with handle(b, precision=precision) as s:
        shape = s.neighbors_shape(m)
        assert shape["batch"] < m, shape                         # more than one batch
        got = s.neighbors(pts, radii=radii.astype(DT[precision]))
    same(got, lattice_ref(b, pts, radii), "m = %d" % m)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_sub_range_has_the_bits_of_the_full_request(precision):
    _, full, part, _, _ = full_query_5000(precision)
    for x, y in zip(full, part):
        assert x[1000:1100].tobytes() == y.tobytes()


# ---- 3. real distributions ---------------------------------------------------------------------

def distribution(name):
    if name == "plummer40002":
        return ic.plummer(40002, seed=5)[0]
    return load_golden32(name + "_bodies0")


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name", ["plummer1024", "disk771", "galaxy_ref", "plummer40002"])
def test_real_distributions_within_the_rounding_bounds(name, precision):
    dt, tol = DT[precision], TOL[precision]
    b = distribution(name).astype(dt)
    n = len(b)
    rng = np.random.default_rng(11)
    lo, hi = b[:, :3].min(0), b[:, :3].max(0)
    h = dt(0.05 * float(np.sqrt(((hi - lo).astype(np.float64) ** 2).sum())))
    pts = np.zeros((512, 4), dt)
    pts[:, :3] = lo + (hi - lo) * rng.random((512, 3))
    radii = (h * (0.5 + rng.random(512))).astype(dt)
    with handle(b, precision=precision) as s:
        index, dist2, count = s.neighbors(bodies=(0, n), radius=h)
        pi, pd, pc = s.neighbors(pts, radii=radii)
    rows = np.arange(n) if n <= 2048 else np.sort(rng.choice(n, 512, replace=False))
    worst = [0.0, 0.0, 0]
    for r in (rows if n > 2048 else [None]):                  # sampled rows one by one (their own row is left out by index)
        sel = slice(0, n) if r is None else slice(r, r + 1)
        w = check_float(b, b[sel], index[sel], dist2[sel], count[sel], np.full(len(b[sel]), h), tol, skip0=0 if r is None else r)
        worst = [max(x, y) for x, y in zip(worst, w)]
    wp = check_float(b, pts, pi, pd, pc, radii, tol)
    print("%s %s: bodies nearest %.3g dist2 %.3g count %d; points nearest %.3g dist2 %.3g count %d (tol %.0e)"
          % ((name, precision) + tuple(worst) + tuple(wp) + (tol,)))
    assert worst[0] <= tol and worst[1] <= tol and worst[2] == 0, worst
    assert wp[0] <= tol and wp[1] <= tol and wp[2] == 0, wp


# ---- 4. the state is untouched -----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["fused", "symmetric", "hermite", "block"])
def test_stepping_is_bit_identical_with_neighbour_calls_in_between(kind):
    n = 20000 if kind == "symmetric" else 1024
    b, v = ic.plummer(n, seed=21)
    pts = np.zeros((100, 4), np.float32)
    pts[:, :3] = np.random.default_rng(1).normal(0, 1, (100, 3))
    kw = {"integrator": "hermite4"} if kind in ("hermite", "block") else {}

    def run(query):
        with handle(b, v, G=0.37, **kw) as s:
            if kind == "block":
                s.set_block_steps()
            for k in range(6):                               # single steps
                s.step()
                if query:
                    s.neighbors(pts, radius=0.3)
                    s.neighbors(bodies=(k, 17))
            for k in range(2):                               # chunks that replay the captured graphs
                s.simulate(32 if kind in ("fused", "symmetric") else 4)
                if query:
                    s.neighbors(bodies=(0, n), radius=0.1)
            return s.read() + (s.variant,)

    plain, mixed = run(False), run(True)
    print(kind, plain[3])
    if kind == "fused":
        assert "fused" in plain[3] or "direct" in plain[3], plain[3]
    if kind == "symmetric":
        assert "sym" in plain[3], plain[3]
    for x, y in zip(plain[:3], mixed[:3]):
        assert x.tobytes() == y.tobytes()


def test_same_request_same_bits():
    b, v = ic.plummer(5000, seed=8)
    with handle(b, v) as s:
        outs = [s.neighbors(bodies=(100, 3000), radius=0.05) for _ in range(2)]
    for x, y in zip(*outs):
        assert x.tobytes() == y.tobytes()


# ---- 5. device pointers ------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_device_pointer_form_equals_the_host_form(precision):
    assert torch is not None
    dt = DT[precision]
    b = ic.plummer(3000, seed=4)[0].astype(dt)
    rng = np.random.default_rng(2)
    pts = np.zeros((1500, 4), dt)
    pts[:, :3] = rng.normal(0, 1, (1500, 3))
    radii = (0.05 + 0.2 * rng.random(1500)).astype(dt)
    tt = torch.float64 if precision == "f64" else torch.float32
    stream = torch.cuda.Stream()
    with handle(b, precision=precision, stream=stream.cuda_stream) as s:
        hp = s.neighbors(pts, radii=radii)
        hb = s.neighbors(bodies=(1000, 2000), radius=0.1)
        with torch.cuda.stream(stream):
            tp, tr = torch.from_numpy(pts).to("cuda"), torch.from_numpy(radii).to("cuda")
            outs = []
            for m in (1500, 2000):
                outs.append((torch.full((m,), 7, device="cuda", dtype=torch.int32), torch.full((m,), 7.0, device="cuda", dtype=tt),
                             torch.full((m,), 7, device="cuda", dtype=torch.int32)))
            s.neighbors_device(tp.data_ptr(), 1500, outs[0][0].data_ptr(), outs[0][1].data_ptr(), outs[0][2].data_ptr(), radii_ptr=tr.data_ptr())
            s.neighbors_device(None, 0, outs[1][0].data_ptr(), outs[1][1].data_ptr(), outs[1][2].data_ptr(), bodies=(1000, 2000), radius=0.1)
        stream.synchronize()
        for host, dev in ((hp, outs[0]), (hb, outs[1])):
            for x, y in zip(host, dev):
                assert x.tobytes() == y.cpu().numpy().tobytes()


# ---- 6. shards ---------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_shard_and_multi_handles_see_only_the_callers_rows(precision):
    n = 5000
    dt = DT[precision]
    b = lattice_bodies(n, 5001, dt, avoid_origin=True)       # no body AT the origin: a padding row would tie with it
    pts = lattice_points(b, 600, 5)
    pts[0, :3] = 0                                           # the origin: where the zero-mass padding rows of a multi handle sit
    radii = np.random.default_rng(6).integers(1, 7, 600)
    radii[0] = 6
    want_b = lattice_ref(b, b, np.full(n, 3), skip0=0)
    want_p = lattice_ref(b, pts, radii)
    assert want_p[1][0] > 0
    with handle(b, precision=precision) as s:
        single = s.neighbors(bodies=(0, n), radius=3), s.neighbors(pts, radii=radii.astype(dt))
    same(single[0], want_b, "single, bodies")
    same(single[1], want_p, "single, points")
    with handle(b, precision=precision, shard=(1024, 2048)) as s:
        for x, y in zip(single[0], s.neighbors(bodies=(0, n), radius=3)):
            assert x.tobytes() == y.tobytes()
        for x, y in zip(single[1], s.neighbors(pts, radii=radii.astype(dt))):
            assert x.tobytes() == y.tobytes()
    with MultiSimulation(n, 3, precision=precision) as m:
        m.init(b, np.zeros_like(b))
        m.set_params(1e-3, 1.0)
        mb = m.neighbors(bodies=(0, n), radius=3)
        mp = m.neighbors(pts, radii=radii.astype(dt))
        assert mb[0].max() < n and mp[0].max() < n               # never a padding row
        for x, y in zip(single[0] + single[1], mb + mp):
            assert x.tobytes() == y.tobytes()
        assert mp[0][0] == want_p[0][0] and mp[1][0] == want_p[1][0] and mp[2][0] == want_p[2][0]     # the point at the origin
        tail = m.neighbors(bodies=(n - 300, 300), radius=3)
        for x, y in zip(single[0], tail):
            assert x[n - 300:].tobytes() == y.tobytes()
        with pytest.raises(NBodyError) as e:
            m.neighbors(bodies=(n - 300, 301))                   # row n exists in the padded system, not in the caller's
        assert e.value.code == 1 and "first_body" in str(e.value) and "nb_multi_neighbors" in str(e.value)
        m.simulate(2)


# ---- 7. errors ---------------------------------------------------------------------------------

def test_every_invalid_request_is_an_ordinary_error():
    b = load_golden32("plummer1024_bodies0")
    v = load_golden32("plummer1024_vel0")
    L = capi.load_library()
    one = np.zeros((1, 4), np.float32)
    rad = np.ones(1, np.float32)
    idx = np.zeros(1, np.uint32)
    cnt = np.zeros(1, np.uint32)

    def raw(s, **kw):
        req = capi.nb_neighbor_request()
        req.struct_size = C.sizeof(capi.nb_neighbor_request)
        req.m = 1
        req.points = one.ctypes.data_as(C.c_void_p)
        req.index = idx.ctypes.data_as(C.c_void_p)
        for k, val in kw.items():
            setattr(req, k, val)
        rc = L.nb_neighbors(s._h, C.byref(req))
        return rc, L.nb_last_error(s._h).decode()

    cptr, rptr = cnt.ctypes.data_as(C.c_void_p), rad.ctypes.data_as(C.c_void_p)
    with Simulation(1024) as s:
        with pytest.raises(NBodyError) as e:             # nothing uploaded
            s.neighbors(one)
        assert e.value.code == 4 and "upload" in str(e.value) and "nb_neighbors" in str(e.value)
        s.init(b, v)
        assert s.neighbors(one)[0][0] < 1024             # nb_set_params is not required
        for kw, word in ((dict(bodies=(0, 0)), "m must"), (dict(bodies=(1000, 25)), "first_body"),
                         (dict(points=one, bodies=(0, 1)), "points must be NULL"), (dict(), "points is NULL"),
                         (dict(points=one, radius=-1.0), "radius"), (dict(points=one, radius=float("nan")), "radius"),
                         (dict(points=one, radius=0.0), "count needs")):
            with pytest.raises(NBodyError) as e:
                s.neighbors(**kw)
            assert e.value.code == 1 and word in str(e.value), (kw, str(e.value))
        with pytest.raises(NBodyError) as e:
            s.neighbors(np.zeros((0, 4), np.float32))
        assert e.value.code == 1
        AT = capi.NB_NBR_AT_BODIES
        for kw, word in ((dict(struct_size=56), "struct_size"), (dict(struct_size=72), "struct_size"), (dict(flags=2), "flags"),
                         (dict(flags=8), "flags"), (dict(flags=1 << 31), "flags"), (dict(m=0), "m must"),
                         (dict(index=None), "all NULL"), (dict(points=None), "points is NULL"), (dict(flags=AT), "points must be NULL"),
                         (dict(flags=AT, points=None, first_body=1024), "first_body"),
                         (dict(flags=AT, points=None, first_body=0xffffffff, m=2), "first_body"),
                         (dict(count=cptr), "count needs"), (dict(count=cptr, radius=0.0), "count needs"),
                         (dict(radius=-0.5), "radius"), (dict(radius=float("nan")), "radius"),
                         (dict(count=cptr, radii=rptr, radius=-1.0), "radius")):
            rc, msg = raw(s, **kw)
            assert rc == 1 and "nb_neighbors" in msg and word in msg, (kw, rc, msg)
        assert L.nb_neighbors(s._h, None) == 1
        assert raw(s)[0] == 0                                          # and the same request without a fault is served
        assert raw(s, count=cptr, radii=rptr)[0] == 0 and raw(s, count=cptr, radius=0.5)[0] == 0
        s.set_params(1e-3, 1.0)
        s.simulate(2)                                                  # ... and the handle still steps


# ---- 8. close pairs ----------------------------------------------------------------------------

def test_close_pairs_returns_exactly_the_planted_pairs():
    n, k, sep, radius = 2048, 20, 1e-4, 3e-4
    b, v = ic.plummer(n, seed=13)
    rng = np.random.default_rng(14)
    rows = rng.choice(n, 2 * k, replace=False)
    first, second = rows[:k], rows[k:]
    u = rng.normal(0, 1, (k, 3))
    u /= np.sqrt((u * u).sum(1))[:, None]
    b[second, :3] = b[first, :3] + (sep * u).astype(np.float32)
    planted = sorted((int(min(i, j)), int(max(i, j))) for i, j in zip(first, second))
    x = b[:, :3].astype(np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2)
    close = sorted((int(i), int(j)) for i, j in zip(*np.nonzero(d2 < (2 * radius) ** 2)) if i < j)
    assert close == planted                                          # nothing else in the sphere comes near the radius
    with handle(b, v) as s:
        pairs, pd2 = s.close_pairs(radius)
    assert pairs.dtype == np.uint32 and [tuple(p) for p in pairs.tolist()] == planted
    want = d2[pairs[:, 0], pairs[:, 1]]                              # fp64 on the stored rows: the differences are exact, 3e-7 for the rest
    assert np.all(np.abs(pd2.astype(np.float64) - want) <= 1e-6 * want) and np.all(np.abs(np.sqrt(want) - sep) <= 0.05 * sep)


# ---- 9. Node -----------------------------------------------------------------------------------

def test_node_neighbors_on_the_gpu():
    import shutil
    import subprocess
    from conftest import ROOT
    node = shutil.which("node")
    if node is None:
        pytest.skip("node not installed")
    p = subprocess.run([node, os.path.join(ROOT, "tests", "js", "node_neighbors_tests.js"), "gpu"], capture_output=True, text=True, timeout=600)
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert line, "node produced no result: rc=%d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(line[-1])
    failed = {k: r for k, r in res["results"].items() if not r["pass"]}
    assert res["ok"] and p.returncode == 0, failed
    assert res["results"]["gpu_neighbors_bodies_vs_double_loop"]["pass"] and res["results"]["gpu_neighbors_points_vs_double_loop"]["pass"]
