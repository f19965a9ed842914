"""GPU tests of nb_field_eval (ABI 2.4): acceleration and potential of a handle's bodies at arbitrary points, and at the bodies
themselves with the self pair left out inside the loop.

Metric, per point k: max_c |a[k, c] - ref[k, c]| / max_c |ref[k, c]| and |phi[k] - ref| / |ref|, `ref` a numpy fp64 direct sum
over the uploaded (f32 or f64) rows.  Bounds: 2e-5 for f32, 1e-12 for f64 handles and for NB_FIELD_F64 (tests/test_sym_gpu.py's).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden32, torch
from nbody3d_amd import MultiSimulation, Simulation, capi, ic
from nbody3d_amd.capi import NBodyError

pytestmark = pytest.mark.gpu

TOL32, TOL64 = 2e-5, 1e-12
EPS2 = 1e-4


def tol_of(precision, f64=False):
    return TOL64 if (precision == "f64" or f64) else TOL32


def ref_field(b, pts, G=1.0, eps2=EPS2, skip=None):
    """fp64 direct sum of the rows `b` (as uploaded) at `pts`; skip[k] = row left out of point k's sums."""
    x = np.asarray(b)[:, :3].astype(np.float64)
    m = np.asarray(b)[:, 3].astype(np.float64)
    p = np.asarray(pts)[:, :3].astype(np.float64)
    acc, phi = np.zeros((len(p), 3)), np.zeros(len(p))
    blk = max(1, 4000000 // len(x))
    for k0 in range(0, len(p), blk):
        d = x[None, :, :] - p[k0:k0 + blk, None, :]
        y = 1.0 / np.sqrt((d * d).sum(2) + eps2)
        w = np.broadcast_to(m, y.shape).copy()
        if skip is not None:
            kk = np.arange(k0, min(k0 + blk, len(p)))
            w[kk - k0, np.asarray(skip)[kk]] = 0.0
        acc[k0:k0 + blk] = G * ((w * y * y * y)[:, :, None] * d).sum(1)
        phi[k0:k0 + blk] = -G * (w * y).sum(1)
    return acc, phi


def errors(a, f, ra, rf):
    ea = (np.abs(a[:, :3].astype(np.float64) - ra).max(1) / np.abs(ra).max(1)).max() if a is not None else 0.0
    ef = (np.abs(f.astype(np.float64) - rf) / np.abs(rf)).max() if f is not None else 0.0
    return float(ea), float(ef)


def check(a, f, ra, rf, tol, what=""):
    ea, ef = errors(a, f, ra, rf)
    print("%s: worst accel %.3g, worst phi %.3g (bound %.0e)" % (what, ea, ef, tol))
    assert ea <= tol and ef <= tol, (what, ea, ef)
    if a is not None:
        assert np.all(a[:, 3] == 0)


def points_for(b, m, seed):               # b: (n, 4) float32 bodies
    rng = np.random.default_rng(seed); n = len(b); h = m // 2
    lo, hi = b[:, :3].min(0), b[:, :3].max(0)
    sig = 0.05 * float(np.sqrt((b[:, :3].astype(np.float64) ** 2).sum(1)).mean())
    near = b[rng.integers(0, n, h), :3] + rng.normal(0, sig, (h, 3)).astype(np.float32)
    box = (lo + (hi - lo) * rng.random((m - h, 3))).astype(np.float32)
    return np.concatenate([near, box]).astype(np.float32)


def fixture(name):
    if name == "plummer65536":
        return ic.plummer(65536, seed=97) + (1.0,)
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))[name]
    return load_golden32(name + "_bodies0"), load_golden32(name + "_vel0"), man["G"]


def handle(b, v, precision="f32", G=1.0, dt=1e-3, **kw):
    s = Simulation(len(b), precision=precision, **kw)
    s.init(b, v)
    s.set_params(dt, G)
    return s


# ---- 1. known answers ------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_known_answers(precision):
    tol = tol_of(precision)
    G, eps2 = 0.37, 2.5e-3
    b = np.array([[-1.0, 0, 0, 2.0], [3.0, 0, 0, 5.0]], np.float32)
    v = np.zeros_like(b)
    with Simulation(2, precision=precision, eps2=eps2) as s:
        s.init(b, v)
        s.set_params(1e-3, G)
        # a point on the axis of two bodies: closed form
        a, f = s.field(np.array([[0.5, 0, 0]]))
        r0, r1 = 1.5 ** 2 + eps2, 2.5 ** 2 + eps2
        ax = G * (2.0 * -1.5 / r0 ** 1.5 + 5.0 * 2.5 / r1 ** 1.5)
        ph = -G * (2.0 / np.sqrt(r0) + 5.0 / np.sqrt(r1))
        assert abs(a[0, 0] - ax) <= tol * abs(ax) and a[0, 1] == 0 and a[0, 2] == 0 and a[0, 3] == 0
        assert abs(f[0] - ph) <= tol * abs(ph)
        # a point ON body 1: exactly nothing from it in accel, -G m / sqrt(eps2) in phi
        a, f = s.field(np.array([[3.0, 0, 0]]))
        r0 = 16.0 + eps2
        assert abs(a[0, 0] - G * 2.0 * -4.0 / r0 ** 1.5) <= tol * abs(G * 2.0 * 4.0 / r0 ** 1.5) and a[0, 1] == 0 and a[0, 2] == 0
        ph = -G * (2.0 / np.sqrt(r0) + 5.0 / np.sqrt(eps2))
        assert abs(f[0] - ph) <= tol * abs(ph)
        # only one output asked for: the other is None, the values are the same
        a2, f2 = s.field(np.array([[3.0, 0, 0]]), phi=False)
        a3, f3 = s.field(np.array([[3.0, 0, 0]]), accel=False)
        assert f2 is None and a3 is None
        assert abs(a2[0, 0] - a[0, 0]) <= tol * abs(a[0, 0]) and abs(f3[0] - f[0]) <= tol * abs(f[0])
        # G scales both outputs linearly
        s.set_params(1e-3, 2 * G)
        a4, f4 = s.field(np.array([[3.0, 0, 0]]))
        assert abs(a4[0, 0] - 2 * a[0, 0]) <= tol * abs(2 * a[0, 0]) and abs(f4[0] - 2 * f[0]) <= tol * abs(2 * f[0])


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_self_exclusion_happens_inside_the_loop(precision):
    """A body of mass 1e7 between two of mass 1, G = 1: its own term would be -1e7 / sqrt(eps2) = -1e9; subtracted afterwards it
    would leave an error of order 30 in a potential of -2."""
    tol = tol_of(precision)
    b = np.array([[0, 0, 0, 1e7], [1, 0, 0, 1], [-1, 0, 0, 1]], np.float32)
    with handle(b, np.zeros_like(b), precision) as s:
        a, f = s.field(bodies=(0, 3))
        want = -2.0 / np.sqrt(1.0 + EPS2)
        assert abs(f[0] - want) <= tol * abs(want), f
        assert np.all(a[0] == 0)                       # the two unit masses cancel exactly
        ra, rf = ref_field(b, b, skip=[0, 1, 2])
        check(a[1:], f, ra[1:], rf, tol, "three bodies")
    gb, gv, G = fixture("galaxy_ref")
    if precision == "f64":
        gb, gv = gb.astype(np.float64), gv.astype(np.float64)
    assert gb[0, 3] == 1e7 and gb[408, 3] == 1e7
    with handle(gb, gv, precision, G=G) as s:
        for row in (0, 408):
            a, f = s.field(bodies=(row, 1))
            ra, rf = ref_field(gb, gb[row:row + 1], G=G, skip=[row])
            check(a, f, ra, rf, tol, "galaxy_ref row %d" % row)


# ---- 2. arbitrary points ---------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name", ["plummer1024", "galaxy_ref", "disk771", "cube1000", "plummer65536"])
def test_arbitrary_points_match_the_fp64_sum(name, precision):
    b, v, G = fixture(name)
    bb, vv = (b.astype(np.float64), v.astype(np.float64)) if precision == "f64" else (b, v)
    with handle(bb, vv, precision, G=G) as s:
        for seed in (11, 12):
            for m in (1, 63, 64, 65, 1000, 4097):
                pts = points_for(b, m, seed)
                a, f = s.field(pts)
                assert a.shape == (m, 4) and f.shape == (m,) and a.dtype == s.dtype and f.dtype == s.dtype
                ra, rf = ref_field(bb, pts, G=G)
                check(a, f, ra, rf, tol_of(precision), "%s %s m=%d seed=%d" % (name, precision, m, seed))


# ---- 3. AT_BODIES == the engine's own accelerations --------------------------------------------

@pytest.mark.parametrize("case", ["disk771", "plummer40002", "plummer40002_716013", "plummer1024_fused", "disk771_f64", "plummer40002_f64"])
def test_at_bodies_equals_the_accelerations_of_the_next_step(case):
    precision = "f64" if case.endswith("_f64") else "f32"
    if case.startswith("disk771"):
        b, v, G = fixture("disk771")
    elif case.startswith("plummer1024"):
        b, v, G = fixture("plummer1024")
    else:
        b, v = ic.plummer(40002, seed=5)
        G = 1.0
    if precision == "f64":
        b, v = b.astype(np.float64), v.astype(np.float64)
    kw = {"force_variant": 716013} if case.endswith("716013") else {}
    with handle(b, v, precision, G=G, dt=1e-4, **kw) as s:
        print(case, s.variant)
        if case.endswith("716013"):
            assert "sym" in s.variant
        if case.endswith("fused"):
            assert "fused" in s.variant or "direct" in s.variant, s.variant
        a, f = s.field(bodies=(0, len(b)))
        s.step()
        acc = s.read(bodies=False, vel=False)[2]         # a(x before the step)
    tol = tol_of(precision)
    ref = acc[:, :3].astype(np.float64)
    err = (np.abs(a[:, :3].astype(np.float64) - ref).max(1) / np.abs(ref).max(1)).max()
    print("%s: field vs step accelerations, worst %.3g" % (case, err))
    assert err <= tol, (case, err)


# ---- 4. potentials add up to the diagnostics ---------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n", [1024, 40002, 65536])
def test_potentials_add_up_to_the_diagnostics(n, precision):
    b, v = ic.plummer(n, seed=3)
    if precision == "f64":
        b, v = b.astype(np.float64), v.astype(np.float64)
    tol = tol_of(precision)
    with handle(b, v, precision, G=0.75) as s:
        ke, pe, _ = s.diagnostics()
        _, f = s.field(bodies=(0, n), accel=False)
        mine = 0.5 * (b[:, 3].astype(np.float64) * f.astype(np.float64)).sum()
        print("n=%d %s: potential energy %.15g vs diagnostics %.15g (%.3g)" % (n, precision, mine, pe, abs(mine - pe) / abs(pe)))
        assert abs(mine - pe) <= tol * abs(pe)
        kin, pot = s.body_energies()                     # right after init: vel and the positions belong to the same time
        assert kin.dtype == np.float64 and pot.dtype == np.float64 and kin.shape == (n,) and pot.shape == (n,)
        assert abs(kin.sum() - ke) <= tol * abs(ke)
        assert abs(pot.sum() - 2.0 * pe) <= tol * abs(2.0 * pe)


# ---- 5. sub-ranges -----------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("name", ["plummer1024", "galaxy_ref"])
def test_sub_ranges_of_bodies(name, precision):
    b, v, G = fixture(name)
    if precision == "f64":
        b, v = b.astype(np.float64), v.astype(np.float64)
    n = len(b)
    with handle(b, v, precision, G=G) as s:
        for first, count in ((0, 1), (n - 1, 1), (255, 3), (700, 700)):
            if first + count > n:
                with pytest.raises(NBodyError) as e:
                    s.field(bodies=(first, count))
                assert e.value.code == 1 and "first_body" in str(e.value)
                count = n - first
            a, f = s.field(bodies=(first, count))
            rows = np.arange(first, first + count)
            ra, rf = ref_field(b, b[rows], G=G, skip=rows)
            check(a, f, ra, rf, tol_of(precision), "%s %s bodies=(%d, %d)" % (name, precision, first, count))
        with pytest.raises(NBodyError) as e:
            s.field(bodies=(n, 1))
        assert e.value.code == 1


# ---- 6. the state is untouched -----------------------------------------------------------------

@pytest.mark.parametrize("n,G,kw", [(1024, 1.0, {}), (1024, 0.37, {}), (5000, 1.0, {}), (5000, 0.37, {}), (20000, 0.37, {}),
                                    (5000, 0.37, {"flags": capi.NB_FLAG_NO_SYM})])
def test_stepping_is_bit_identical_with_field_calls_in_between(n, G, kw):
    b, v = ic.plummer(n, seed=21)
    pts = points_for(b, 100, 11)

    def run(query):
        with handle(b, v, G=G, **kw) as s:
            for k in range(20):                          # single steps
                s.step()
                if query:
                    s.field(pts)
                    s.field(bodies=(k, 17), accel=(k & 1) == 0)
            for k in range(3):                           # chunks that replay the captured graphs
                s.simulate(32)
                if query:
                    s.field(bodies=(0, n))
                    s.field(pts, f64=True)
            return s.read() + (s.variant,)

    plain, mixed = run(False), run(True)
    print(n, G, plain[3])
    for x, y in zip(plain[:3], mixed[:3]):
        assert x.tobytes() == y.tobytes()


# ---- 7. determinism ----------------------------------------------------------------------------

def test_same_request_same_bits():
    b, v = ic.plummer(30000, seed=8)
    pts = points_for(b, 3000, 12)
    b2, v2 = ic.plummer(16384, seed=9)
    with handle(b, v) as s, handle(b2, v2) as other:
        outs = [s.field(pts) + s.field(bodies=(100, 5000))]
        outs.append(s.field(pts) + s.field(bodies=(100, 5000)))
        other.simulate(200)                              # its own stream: runs beside the request below
        outs.append(s.field(pts) + s.field(bodies=(100, 5000)))
        other.sync()
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert x.tobytes() == y.tobytes()


# ---- 8. NB_FIELD_F64 on an f32 handle ----------------------------------------------------------

@pytest.mark.parametrize("name", ["plummer1024", "galaxy_ref", "plummer65536"])
def test_fp64_audit_mode_on_an_f32_handle(name):
    b, v, G = fixture(name)
    with handle(b, v, G=G) as s:
        pts = points_for(b, 300, 11)
        a, f = s.field(pts, f64=True)
        assert a.dtype == np.float64 and f.dtype == np.float64
        ra, rf = ref_field(b, pts, G=G)
        check(a, f, ra, rf, TOL64, name + " f64 audit, points")
        rows = np.arange(200, 500)
        a, f = s.field(bodies=(200, 300), f64=True)
        ra, rf = ref_field(b, b[rows], G=G, skip=rows)
        check(a, f, ra, rf, TOL64, name + " f64 audit, bodies")


# ---- 9. device pointers ------------------------------------------------------------------------

@pytest.mark.parametrize("f64", [False, True])
def test_device_pointer_form_equals_the_host_form(f64):
    assert torch is not None
    b, v = ic.plummer(8192, seed=4)
    pts = np.concatenate([points_for(b, 1500, 11), np.zeros((1500, 1), np.float32)], axis=1)
    stream = torch.cuda.Stream()
    out_t = torch.float64 if f64 else torch.float32
    with handle(b, v, G=0.5, stream=stream.cuda_stream) as s:
        ha, hf = s.field(pts, f64=f64)
        hba, hbf = s.field(bodies=(1000, 2000), f64=f64)
        with torch.cuda.stream(stream):
            tp = torch.from_numpy(pts).to("cuda", non_blocking=False)
            ta = torch.full((1500, 4), 7.0, device="cuda", dtype=out_t)
            tf = torch.full((1500,), 7.0, device="cuda", dtype=out_t)
            tba = torch.full((2000, 4), 7.0, device="cuda", dtype=out_t)
            tbf = torch.full((2000,), 7.0, device="cuda", dtype=out_t)
            s.field_device(tp.data_ptr(), 1500, ta.data_ptr(), tf.data_ptr(), f64=f64)
            s.field_device(None, 0, tba.data_ptr(), tbf.data_ptr(), bodies=(1000, 2000), f64=f64)
            s.field_device(tp.data_ptr(), 1500, None, tf.data_ptr(), f64=f64)        # potential only: same bits in f64, same bound in f32
        stream.synchronize()
        assert ta.cpu().numpy().tobytes() == ha.tobytes()
        assert tba.cpu().numpy().tobytes() == hba.tobytes() and tbf.cpu().numpy().tobytes() == hbf.tobytes()
        assert np.abs(tf.cpu().numpy().astype(np.float64) - hf).max() <= (TOL64 if f64 else TOL32) * np.abs(hf).max()


# ---- 10. shards --------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_shard_and_multi_handles(precision):
    """After three steps: a shard handle and a two-shard system answer within the bounds of the fp64 sum over the rows they
    hold themselves (what read() returns); the row indices of a multi handle are the caller's unpadded ones."""
    b, v, G = fixture("plummer1024")
    if precision == "f64":
        b, v = b.astype(np.float64), v.astype(np.float64)
    tol = tol_of(precision)
    pts = points_for(b.astype(np.float32), 200, 11)
    with handle(b, v, precision, shard=(256, 512)) as s:
        s.simulate(3)
        now = s.read(vel=False, accel=False)[0]
        a, f = s.field(pts)
        check(a, f, *ref_field(now, pts), tol, "shard handle, points")
        rows = np.arange(300, 1000)
        a, f = s.field(bodies=(300, 700))
        check(a, f, *ref_field(now, now[rows], skip=rows), tol, "shard handle, bodies")
    n = 1000                                             # padded to whole blocks per shard inside the multi handle
    with MultiSimulation(n, 2, precision=precision) as m:
        m.init(b[:n], v[:n])
        m.set_params(1e-3, 1.0)
        m.simulate(3)
        now = m.read(vel=False, accel=False)[0]
        a, f = m.field(pts)
        check(a, f, *ref_field(now, pts), tol, "multi handle, points")
        rows = np.arange(n - 300, n)
        a, f = m.field(bodies=(n - 300, 300))
        check(a, f, *ref_field(now, now[rows], skip=rows), tol, "multi handle, bodies")
        with pytest.raises(NBodyError) as e:
            m.field(bodies=(n - 300, 301))               # row n exists in the padded system, not in the caller's
        assert e.value.code == 1 and "first_body" in str(e.value)

# ---- 11. errors --------------------------------------------------------------------------------

def test_every_invalid_request_is_an_ordinary_error():
    b, v, _ = fixture("plummer1024")
    L = capi.load_library()
    one = np.zeros((1, 4), np.float32)
    out = np.zeros((1, 4), np.float32)

    def raw(s, **kw):
        req = capi.nb_field_request()
        req.struct_size = C.sizeof(capi.nb_field_request)
        req.m = 1
        req.points = one.ctypes.data_as(C.c_void_p)
        req.accel = out.ctypes.data_as(C.c_void_p)
        for k, val in kw.items():
            setattr(req, k, val)
        rc = L.nb_field_eval(s._h, C.byref(req))
        return rc, L.nb_last_error(s._h).decode()

    with Simulation(1024) as s:
        with pytest.raises(NBodyError) as e:             # nothing uploaded
            s.field(one)
        assert e.value.code == 4 and "upload" in str(e.value)
        s.init(b, v)
        with pytest.raises(NBodyError) as e:             # no parameters
            s.field(one)
        assert e.value.code == 4 and "nb_set_params" in str(e.value)
        s.set_params(1e-3, 1.0)
        for kw, word in ((dict(points=one, accel=False, phi=False), "accel and phi"), (dict(bodies=(0, 0)), "m must"),
                         (dict(bodies=(1000, 25)), "first_body"), (dict(points=one, bodies=(0, 1)), "points must be NULL"),
                         (dict(), "points is NULL")):
            with pytest.raises(NBodyError) as e:
                s.field(**kw)
            assert e.value.code == 1 and word in str(e.value), (kw, str(e.value))
        with pytest.raises(NBodyError) as e:
            s.field(np.zeros((0, 4), np.float32))
        assert e.value.code == 1
        for kw, word in ((dict(struct_size=24), "struct_size"), (dict(struct_size=48), "struct_size"), (dict(flags=8), "flags"),
                         (dict(flags=1 << 31), "flags"), (dict(m=0), "m must"), (dict(accel=None), "accel and phi"),
                         (dict(points=None), "points is NULL"), (dict(flags=capi.NB_FIELD_AT_BODIES), "points must be NULL"),
                         (dict(flags=capi.NB_FIELD_AT_BODIES, points=None, first_body=1024), "first_body"),
                         (dict(flags=capi.NB_FIELD_AT_BODIES, points=None, first_body=0xffffffff, m=2), "first_body")):
            rc, msg = raw(s, **kw)
            assert rc == 1 and "nb_field_eval" in msg and word in msg, (kw, rc, msg)
        assert L.nb_field_eval(s._h, None) == 1
        assert raw(s)[0] == 0                                          # and the same request without a fault is served
        s.simulate(2)                                                  # ... and the handle still steps


# ---- 12. / 13. large N ---------------------------------------------------------------------------

def test_two_million_bodies_single_rows_audit():
    """The audit use: single rows of a 2 M-body system on a handle that was never stepped, f32 within a flat 2e-5 of the fixture's
    fp64 sums (a design that lets one register take the whole sum is 1e-4 off), the fp64 mode within 1e-12."""
    n = 2000000
    b, v = ic.plummer(n, seed=7)
    case = [c for c in json.load(open(os.path.join(GOLDEN, "large_n_row_spread.json")))["cases"] if c["n"] == n][0]
    with handle(b, v, flags=capi.NB_FLAG_NO_SYM) as s:
        for row in (0, 1, 999999, 1234567, 1999999):
            want = np.array(case["rows"][str(row)]["a_f64"])
            a, f = s.field(bodies=(row, 1))
            e32 = np.abs(a[0, :3] - want).max() / np.abs(want).max()
            a64, f64 = s.field(bodies=(row, 1), f64=True)
            e64 = np.abs(a64[0, :3] - want).max() / np.abs(want).max()
            print("row %d: f32 %.3g, fp64 mode %.3g, phi f32 vs fp64 mode %.3g" % (row, e32, e64, abs(f[0] - f64[0]) / abs(f64[0])))
            assert e32 <= TOL32 and e64 <= TOL64, (row, e32, e64)
            assert abs(f[0] - f64[0]) <= TOL32 * abs(f64[0])


def test_few_points_against_a_million_bodies():
    n, m = 1048576, 1024
    b, v = ic.plummer(n, seed=3)
    rng = np.random.default_rng(11)
    lo, hi = b[:, :3].min(0), b[:, :3].max(0)
    pts = (lo + (hi - lo) * rng.random((m, 3))).astype(np.float32)
    with handle(b, v, flags=capi.NB_FLAG_NO_SYM) as s:
        a, f = s.field(pts)
        a64, f64 = s.field(pts[:64], f64=True)
    pick = np.arange(0, m, 32)
    ra, rf = ref_field(b, pts[pick])
    check(a[pick], f[pick], ra, rf, TOL32, "m = 1,024 against N = 1,048,576")
    check(a64[pick[:2]], f64[pick[:2]], ra[:2], rf[:2], TOL64, "the same, fp64 mode")


# ---- 14. Node ----------------------------------------------------------------------------------

def test_node_field_on_the_gpu():
    import shutil
    import subprocess
    from conftest import ROOT
    node = shutil.which("node")
    if node is None:
        pytest.skip("node not installed")
    p = subprocess.run([node, os.path.join(ROOT, "tests", "js", "node_field_tests.js"), "gpu"], capture_output=True, text=True, timeout=600)
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert line, "node produced no result: rc=%d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(line[-1])
    failed = {k: r for k, r in res["results"].items() if not r["pass"]}
    assert res["ok"] and p.returncode == 0, failed
    assert res["results"]["gpu_field_points_vs_double_loop"]["pass"] and res["results"]["gpu_field_bodies_vs_double_loop"]["pass"]
