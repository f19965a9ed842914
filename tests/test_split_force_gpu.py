"""GPU tests of nb_split_force: the regular and the irregular force+jerk of every point in one pass.

The census inputs of tests/split_force_ref.py (jittered lattice, radii of 1.6 / 2.4 spacings, at the bodies and at 300 points) are
held to the tolerances recorded in tests/golden/split_force_census.json -- 8 x the worst row error of a binary32 restatement, on the
metric |got - ref|_2 / sum |term|_2 taken over the terms of EACH sum, where one pair on the wrong side of the radius shows in both
sums --, f64 handles to 1e-12 on the same metric.  The launch-edge cases run on the first n rows of the input (1025, 2.4 spacings)
-- the same pairs, sums no longer than its sums -- and are held to that input's tolerances: on this metric a sum's error is at most
(the rounding of one term) + (terms in one chain) x 2^-24, both relative to sum |term|, so a sum of fewer terms from the same pairs
stays inside the bound measured for the longer ones (tests/test_list_force_gpu.py argues the same way).  The promises about bits
are checked as bits."""
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
INPUTS = [(n, sp) for n in R.SIZES for sp in R.SPACINGS]
ACCEL = R.OUTPUTS[:2]


def handle(b, v=None, precision="f32", G=R.G, dt=1e-3, eps2=R.EPS2, **kw):
    s = Simulation(len(b), precision=precision, eps2=eps2, **kw)
    s.init(b.astype(DT[precision]), (np.zeros_like(b) if v is None else v).astype(DT[precision]))
    s.set_params(dt, G)
    return s


def hermite(b, v, precision="f32", **kw):
    return handle(b, v, precision, integrator="hermite4", **kw)


def tols(precision, n=1025, spacings=2.4, pre=""):
    if precision == "f64":
        return {name: R.TOL_F64 for name in R.OUTPUTS}
    e = R.entry(n, spacings)
    return {name: e[pre + name + "_tol"] for name in R.OUTPUTS}


def hold(got, ref, tol, what):
    """Every output that was returned within its tolerance on the row metric; a sum without a term exactly zero (row_err asserts
    it); .w of every row 0."""
    err = R.errors(got, ref)
    print(what, "errors:", {k: "%.3g" % e for k, e in err.items()}, "tolerances:", {k: "%.3g" % tol[k] for k in err})
    assert set(err) == set(got)
    for name, e in err.items():
        assert e <= tol[name], (what, name, e, tol[name])
        assert not got[name][:, 3].any(), (what, name)


def bits(x, y, what):
    assert set(x) == set(y), what
    for name in x:
        assert x[name].dtype == y[name].dtype and x[name].tobytes() == y[name].tobytes(), (what, name)


# ---- 1. census ---------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("n,spacings", INPUTS)
def test_census(n, spacings, precision):
    c = R.census_input(n, spacings)
    dt = DT[precision]
    pts, pv = c["pts"].astype(dt), c["pv"].astype(dt)
    ref, pref = c["ref"], c["pref"]            # (the stored rows are binary32 in both precisions: one reference serves both)
    tol, ptol = tols(precision, n, spacings), tols(precision, n, spacings, "pt_")
    with hermite(c["b"], c["v"], precision) as s:
        got = s.split_force(bodies=(0, n), radius=c["radius"])
        assert list(got) == list(R.OUTPUTS)
        hold(got, ref, tol, "at the bodies, Hermite")
        hold(s.split_force(pts, point_vel=pv, radius=c["radius"]), pref, ptol, "at the points, Hermite")
    with handle(c["b"], c["v"], precision) as s:
        got = s.split_force(bodies=(0, n), radius=c["radius"])
        assert list(got) == list(ACCEL)
        hold(got, ref, tol, "at the bodies, leapfrog")
        hold(s.split_force(pts, radius=c["radius"]), pref, ptol, "at the points, leapfrog")
    none = pref["member"].sum(1) == 0            # (at 1.6 spacings some points have no member: row_err has held them to == 0)
    print("points without a member:", int(none.sum()))


# ---- 2. the boundary, exactly ------------------------------------------------------------------

LAT = 9
LAT_EPS2 = 18.0     # |term| = m r / (r^2 + eps2)^(3/2) peaks at r = sqrt(eps2 / 2) = 3: with equal masses the d2 = 9 shell holds a row's largest terms


def lattice_input():
    g = np.arange(LAT)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    b = np.zeros((LAT ** 3, 4), np.float32)
    b[:, :3] = xyz
    b[:, 3] = 1.0 / LAT ** 3
    v = census_ref.velocities(LAT ** 3, 3)
    q = np.array([-1, 2, 5, 9])
    pxyz = np.stack(np.meshgrid(q, q, q, indexing="ij"), -1).reshape(-1, 3)
    pts = np.zeros((64, 4), np.float32)
    pts[:, :3] = pxyz
    return b, v, xyz.astype(np.int64), pts, pxyz.astype(np.int64), list_force_ref.point_velocities(64, 3)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_the_boundary_is_exact(precision):
    """Integer coordinates: d2 is exact in both precisions, so the membership is int64 arithmetic's: 4 d2 < (2 h)^2.  radius 3 leaves
    the pairs at d2 = 9 -- (3, 0, 0), (2, 2, 1) ... -- out, nextafter(3) takes them in.  The tolerance is the restatement's own error on
    this very input x 8 (computed here, on the CPU), and the shell pairs hold far more than that of either sum."""
    dt = DT[precision]
    b, v, xi, pts, pi, pv = lattice_input()
    n = len(b)
    up = float(np.nextafter(dt(3), dt(np.inf)))
    alt = np.array([1, 2, 2.5, 3])
    cases = [("radius 3", dict(radius=3.0), lambda m: np.full(m, 36)), ("nextafter(3)", dict(radius=up), lambda m: np.full(m, 37)),
             ("radii 1, 2, 2.5, 3", None, lambda m: np.array([4, 16, 25, 36])[np.arange(m) % 4])]
    with hermite(b, v, precision, eps2=LAT_EPS2) as s:
        for what, kw, h2x4 in cases:
            for probes, pint, args in (("bodies", xi, dict(bodies=(0, n))), ("points", pi, dict(points=pts.astype(dt), point_vel=pv.astype(dt)))):
                m = len(pint)
                d2 = ((xi[None, :, :] - pint[:, None, :]) ** 2).sum(2)
                member = 4 * d2 < h2x4(m)[:, None]
                rkw = dict(radii=alt[np.arange(m) % 4]) if kw is None else kw
                fkw = {} if probes == "bodies" else dict(pts=pts, pvel=pv)
                ref = R.split_ref(b, v, eps2=LAT_EPS2, member=member, dtype=dt, **fkw)
                r32 = R.errors(R.split_f32(b, v, eps2=LAT_EPS2, member=member, **fkw), ref)
                tol = {k: R.TOL_F64 if precision == "f64" else R.TOL_FACTOR * e for k, e in r32.items()}
                shell = d2 == 9
                assert shell.any(1).all() and (member[shell].all() if what == "nextafter(3)" else not member[shell].any())
                if probes == "bodies":
                    assert np.allclose(ref["tn"].max(1), np.where(shell, ref["tn"], 0).max(1), rtol=1e-12)      # the row's largest terms
                for name in ACCEL:                                        # one shell pair on the wrong side shows in either sum
                    scale = ref[name + "_scale"][:, None]
                    share = np.where(shell & (scale > 0), ref["tn"] / np.where(scale > 0, scale, 1), np.inf).min()
                    assert share >= 8 * R.TOL_FACTOR * r32[name], (what, probes, name, share)
                hold(s.split_force(**args, **rkw), ref, tol, "%s, %s" % (what, probes))


# ---- 3. against the entry points that exist ----------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_against_list_force_the_force_jerk_pass_and_field_eval(precision):
    """Each check on the row metric with the sum of the two recorded tolerances (f64: 2 x 1e-12).  The two sums together are judged on
    the scale of the whole row, where their error is at most the larger of their two tolerances."""
    n, sp = 1025, 2.4
    c = R.census_input(n, sp)
    ref = c["ref"]
    st = tols(precision, n, sp)
    f64 = precision == "f64"
    le = list_force_ref.entry(n, sp)
    pe = census_ref.entry("accel", n)
    with hermite(c["b"], c["v"], precision) as s:
        got = s.split_force(bodies=(0, n), radius=c["radius"])
        rows, cnt = s.neighbor_lists(bodies=(0, n), radius=c["radius"], cap=list_force_ref.CAP)
        assert int(cnt.max()) <= list_force_ref.CAP and np.array_equal(cnt, ref["member"].sum(1) - 1)
        la, lj, _ = s.list_force(rows, bodies=(0, n), count=cnt, jerk=True)
        full_a, full_j = s.read()[2], s.read_jerk()
        every = s.split_force(bodies=(0, n), radius=100.0)
        nothing = s.split_force(bodies=(0, n), radii=np.zeros(n))
    for kind, other, otol in (("accel", la, le["a_tol"]), ("jerk", lj, le["jerk_tol"])):
        err = R.row_err(got[kind + "_irr"][:, :3], other[:, :3].astype(np.float64), ref[kind + "_irr_scale"])[1]
        tol = 2 * R.TOL_F64 if f64 else st[kind + "_irr"] + otol
        print("%s_irr against nb_list_force: %.3g (tolerance %.3g)" % (kind, err, tol))
        assert err <= tol
    for kind, other, otol in (("accel", full_a, pe["tol"]), ("jerk", full_j, pe["jerk_tol"])):
        both = got[kind + "_irr"][:, :3].astype(np.float64) + got[kind + "_reg"][:, :3].astype(np.float64)
        scale = ref[kind + "_irr_scale"] + ref[kind + "_reg_scale"]
        err = R.row_err(both, other[:, :3].astype(np.float64), scale)[1]
        tol = 2 * R.TOL_F64 if f64 else max(st[kind + "_irr"], st[kind + "_reg"]) + otol
        print("%s_irr + %s_reg against the force+jerk pass: %.3g (tolerance %.3g)" % (kind, kind, err, tol))
        assert err <= tol
    for name in ("accel_reg", "jerk_reg"):
        assert not every[name].any(), name              # the radius covers everything: == 0
        assert every[name.replace("reg", "irr")].any()
    for name in ("accel_irr", "jerk_irr"):
        assert not nothing[name].any(), name            # radii all 0: == 0
    with handle(c["b"], c["v"], precision) as s:
        got = s.split_force(bodies=(0, n), radius=c["radius"])
        fa, _ = s.field(bodies=(0, n))
        assert not s.split_force(bodies=(0, n), radius=100.0)["accel_reg"].any()
        assert not s.split_force(bodies=(0, n), radii=np.zeros(n))["accel_irr"].any()
    both = got["accel_irr"][:, :3].astype(np.float64) + got["accel_reg"][:, :3].astype(np.float64)
    err = R.row_err(both, fa[:, :3].astype(np.float64), ref["accel_irr_scale"] + ref["accel_reg_scale"])[1]
    tol = 2 * R.TOL_F64 if f64 else max(st["accel_irr"], st["accel_reg"]) + pe["tol"]
    print("accel_irr + accel_reg against nb_field_eval: %.3g (tolerance %.3g)" % (err, tol))
    assert err <= tol


# ---- 4. the edges of the launch ----------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_sizes_around_every_edge_of_the_launch(precision):
    """The first n rows of the input (1025, 2.4 spacings), n around the tile edge (256) and the first-level flush (1,024 terms); m
    around the wave (64) and one workgroup's points (rows_per_workgroup from the shape call), first_body != 0."""
    c = R.census_input(1025, 2.4)
    tol = tols(precision)
    for n in (1, 2, 255, 256, 257, 1023, 1025):
        b, v = c["b"][:n], c["v"][:n]
        with hermite(b, v, precision) as s:
            shape = s.split_force_shape(n)
            rpw = shape["rows_per_workgroup"]
            assert rpw in (256, 512, 1024) and shape["batch"] == n and shape["chunks"] >= 1 and shape["j_per_chunk"] % 256 == 0
            got = s.split_force(bodies=(0, n), radius=c["radius"])
            hold(got, R.split_ref(b, v, radius=c["radius"]), tol, "n %d" % n)
            if n == 1:
                assert all(not x.any() for x in got.values())           # the own row alone: everything 0
            if n == 1025:
                for m in sorted({1, 63, 64, 65, rpw - 1, rpw + 1} - {0}):
                    for first in (0, n - m):
                        hold(s.split_force(bodies=(first, m), radius=c["radius"]), R.split_ref(b, v, radius=c["radius"], first=first, m=m), tol,
                             "m %d first_body %d" % (m, first))


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_more_than_one_j_chunk(precision):
    c = R.census_input(4099, 2.4)
    m, first = 64, 4099 - 64
    with hermite(c["b"], c["v"], precision) as s:
        shape = s.split_force_shape(m)
        print(shape)
        assert shape["chunks"] >= 2 and shape["chunks"] * shape["j_per_chunk"] >= 4099
        got = s.split_force(bodies=(first, m), radius=c["radius"])
    ref = {k: (x[first:] if isinstance(x, np.ndarray) and len(x) == 4099 else x) for k, x in c["ref"].items()}
    hold(got, ref, tols(precision, 4099, 2.4), "%d j-chunks" % shape["chunks"])


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_two_batches(precision):
    """m = batch + 300 arbitrary points against n = 300 (the first rows of the input (1025, 2.4 spacings)); the reference covers the
    first rows, the rows around the seam, the last rows and a random sample."""
    n = 300
    c = R.census_input(1025, 2.4)
    b, v, dt = c["b"][:n], c["v"][:n], DT[precision]
    with handle(b, v, precision) as s:
        batch = s.split_force_shape(1 << 30)["batch"]
        m = batch + 300
        assert s.split_force_shape(m)["batch"] == batch and batch % s.split_force_shape(m)["rows_per_workgroup"] == 0
        pts = R.points(n, m, 11).astype(dt)
        got = s.split_force(pts, radius=c["radius"])
    assert all(np.isfinite(x).all() and not x[:, 3].any() for x in got.values())
    rows = np.unique(np.concatenate([np.arange(300), np.arange(batch - 300, m), np.random.default_rng(4).integers(0, m, 1000)]))
    ref = R.split_ref(b, None, radius=c["radius"], pts=pts[rows], dtype=dt, terms=False)
    hold({k: x[rows] for k, x in got.items()}, ref, tols(precision, pre="pt_"), "%d points in two batches of at most %d" % (m, batch))


# ---- 5. bits -----------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_same_request_same_bits(precision):
    c = R.census_input(1025, 2.4)
    n, dt = 1025, DT[precision]
    tt = torch.float64 if precision == "f64" else torch.float32
    with hermite(c["b"], c["v"], precision) as s:
        one = s.split_force(bodies=(0, n), radius=c["radius"])
        bits(s.split_force(bodies=(0, n), radius=c["radius"]), one, "the same request twice")
        h = float(dt(c["radius"]))
        bits(s.split_force(bodies=(0, n), radii=np.full(n, h, dt)), one, "scalar radius against a filled radii")
        pone = s.split_force(c["pts"].astype(dt), point_vel=c["pv"].astype(dt), radius=c["radius"])
        dev = torch.device("cuda", torch.cuda.current_device())
        dp, dv = torch.from_numpy(c["pts"].astype(dt)).to(dev), torch.from_numpy(c["pv"].astype(dt)).to(dev)
        outs = {name: torch.empty((len(c["pts"]), 4), dtype=tt, device=dev) for name in R.OUTPUTS}
        bouts = {name: torch.empty((n, 4), dtype=tt, device=dev) for name in R.OUTPUTS}
        torch.cuda.current_stream(dev).synchronize()
        s.split_force_device(len(c["pts"]), points_ptr=dp.data_ptr(), point_vel_ptr=dv.data_ptr(), radius=c["radius"],
                             **{name + "_ptr": t.data_ptr() for name, t in outs.items()})
        s.split_force_device(0, bodies=(0, n), radius=c["radius"], **{name + "_ptr": t.data_ptr() for name, t in bouts.items()})
        s.sync()
        bits({k: t.cpu().numpy() for k, t in outs.items()}, pone, "host against device pointers, at the points")
        bits({k: t.cpu().numpy() for k, t in bouts.items()}, one, "host against device pointers, at the bodies")


@pytest.mark.parametrize("kind", ["hermite", "block", "symmetric"])
def test_a_stepped_handle_answers_as_a_fresh_twin_loaded_with_its_state(kind):
    n = 4096 if kind == "symmetric" else 1024
    b, v = ic.plummer(n, seed=21)
    kw = {"force_variant": 708013} if kind == "symmetric" else {"integrator": "hermite4"}
    pts = np.ascontiguousarray(b[:200] + np.float32(0.01))
    pv = np.ascontiguousarray(v[:200])
    jerk = kind != "symmetric"
    ask = lambda s: (s.split_force(bodies=(n // 3, 300), radius=0.2), s.split_force(pts, point_vel=pv if jerk else None, radius=0.3))
    with handle(b, v, G=1.0, **kw) as s:
        if kind == "block":
            s.set_block_steps()
        fresh = ask(s)
        s.simulate(3)
        got = ask(s)
        state = s.read()
        if kind == "symmetric":
            assert "sym" in s.variant, s.variant
    twin_kw = {"force_variant": 1, "jsplit": 1} if kind == "symmetric" else {"integrator": "hermite4"}
    with handle(state[0], state[1], G=1.0, **twin_kw) as t:
        want = ask(t)
    for g, w, f in zip(got, want, fresh):
        bits(g, w, kind)
        assert all(g[k].tobytes() != f[k].tobytes() for k in g)         # and not the answers of the state before the steps


# ---- 6. the state is untouched -----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["symmetric", "hermite", "block"])
def test_stepping_is_bit_identical_with_a_call_in_between(kind):
    n = 4096 if kind == "symmetric" else 1024
    b, v = ic.plummer(n, seed=21)
    kw = {"force_variant": 708013} if kind == "symmetric" else {"integrator": "hermite4"}

    def run(query):
        with handle(b, v, G=1.0, **kw) as s:
            if kind == "block":
                s.set_block_steps()
            s.simulate(3)
            if query:
                got = s.split_force(bodies=(0, n), radius=0.2)
                assert all(np.isfinite(x).all() for x in got.values()) and len(got) == (2 if kind == "symmetric" else 4)
                s.split_force(b[:100], radii=np.linspace(0.0, 0.5, 100), jerk=False)
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
def test_multi_handles(shards):
    n, sp = 1025, 2.4                                                    # ragged: the padded system has rows past n
    c = R.census_input(n, sp)
    with MultiSimulation(n, shards, eps2=R.EPS2) as m:
        m.init(c["b"], c["v"])
        m.set_params(1e-3, R.G)
        hold(m.split_force(bodies=(0, n), radius=c["radius"]), c["ref"], tols("f32", n, sp), "%d shards, at the bodies" % shards)
        hold(m.split_force(c["pts"], radius=c["radius"]), c["pref"], tols("f32", n, sp, "pt_"), "%d shards, at the points" % shards)
        with pytest.raises(NBodyError) as e:
            m.split_force(bodies=(0, n), radius=c["radius"], jerk=True)
        assert e.value.code == 1 and "jerk" in str(e.value) and "nb_multi_split_force" in str(e.value)
        with pytest.raises(NBodyError) as e:
            m.split_force(bodies=(n - 300, 301), radius=c["radius"])      # row n exists in the padded system, not in the caller's
        assert e.value.code == 1 and "first_body" in str(e.value) and "nb_multi_split_force" in str(e.value)
        m.simulate(2)


# ---- 8. errors ---------------------------------------------------------------------------------

def test_every_invalid_request_is_an_ordinary_error():
    b = load_golden32("plummer1024_bodies0")
    v = load_golden32("plummer1024_vel0")
    L = capi.load_library()
    one = np.zeros((1, 4), np.float32)
    out = np.zeros((1, 4), np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)

    def raw(s, **kw):
        req = capi.nb_split_force_request()
        req.struct_size = C.sizeof(capi.nb_split_force_request)
        req.m, req.radius = 1, 0.5
        req.points, req.accel_irr = P(one), P(out)
        for name, val in kw.items():
            setattr(req, name, val)
        rc = L.nb_split_force(s._h, C.byref(req))
        return rc, L.nb_last_error(s._h).decode()

    with Simulation(1024) as s:
        with pytest.raises(NBodyError) as e:             # nothing uploaded
            s.split_force(one, radius=0.5)
        assert e.value.code == 4 and "upload" in str(e.value) and "nb_split_force" in str(e.value)
        s.init(b, v)
        with pytest.raises(NBodyError) as e:             # no parameters
            s.split_force(one, radius=0.5)
        assert e.value.code == 4 and "nb_set_params" in str(e.value) and "nb_split_force" in str(e.value)
        s.set_params(1e-3, 1.0)
        with pytest.raises(NBodyError) as e:             # the jerk on a leapfrog handle
            s.split_force(bodies=(0, 1), radius=0.5, jerk=True)
        assert e.value.code == 4 and "Hermite" in str(e.value) and "nb_split_force" in str(e.value)
        AT = capi.NB_SPLIT_AT_BODIES
        for kw, word in ((dict(struct_size=72), "struct_size"), (dict(struct_size=88), "struct_size"), (dict(m=0), "m must"),
                         (dict(flags=2), "flags"), (dict(flags=8), "flags"), (dict(flags=1 << 31), "flags"),
                         (dict(accel_irr=None), "all NULL"), (dict(points=None), "points is NULL"), (dict(flags=AT), "points must be NULL"),
                         (dict(flags=AT, points=None, point_vel=P(one)), "point_vel must be NULL"),
                         (dict(point_vel=P(one)), "point_vel must be NULL"), (dict(jerk_irr=P(out)), "point_vel is NULL"),
                         (dict(jerk_reg=P(out)), "point_vel is NULL"),
                         (dict(flags=AT, points=None, first_body=1024), "first_body"),
                         (dict(flags=AT, points=None, first_body=0xffffffff, m=2), "first_body"),
                         (dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=float("nan")), "radius"),
                         (dict(radius=-1.0, radii=P(one)), "radius")):
            rc, msg = raw(s, **kw)
            assert rc == 1 and "nb_split_force" in msg and word in msg, (kw, rc, msg)
        assert L.nb_split_force(s._h, None) == 1
        with pytest.raises(NBodyError) as e:
            s.split_force_shape(0)
        assert e.value.code == 1 and "m must" in str(e.value) and "nb_split_force_shape" in str(e.value)
        assert raw(s)[0] == 0                                            # and the same request without a fault is served
        assert raw(s, flags=AT, points=None, first_body=1023)[0] == 0 and raw(s, accel_irr=None, accel_reg=P(out))[0] == 0
        assert raw(s, radius=0.0, radii=P(one))[0] == 0 and not out.any()      # radii[0] = 0: no member, accel_irr == 0
        s.simulate(2)                                                    # ... and the handle still steps
    with Simulation(1024, integrator="hermite4") as s:
        s.init(b, v)
        s.set_params(1e-3, 1.0)
        rc, msg = raw(s, jerk_irr=P(out))
        assert rc == 1 and "point_vel is NULL" in msg
        assert raw(s, jerk_reg=P(out), point_vel=P(one))[0] == 0 and raw(s, flags=AT, points=None, jerk_irr=P(out))[0] == 0
