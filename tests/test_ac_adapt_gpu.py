"""The neighbour scheme with radii that follow a target count and its bit-exact restore (Simulation.set_neighbor_adapt,
upload_neighbor_scheme) on the GPU: against a fixed-radii twin where the rule cannot move a radius (every new kernel tied to the tested
ones), against the restatement tests/ac_adapt_ref.py and the record tests/golden/ac_adapt.json, a start that rebuilds against the public
queries, the smallest shapes, the checkpoint, the cold collapse fixed radii cannot carry, and the ways back to a handle without it."""
import numpy as np
import pytest

from nbody3d_amd import Simulation, capi, ic

import ac_adapt_ref as A
import ac_ref as R
from ac_ref import EPS2, norm_err

pytestmark = pytest.mark.gpu

PRECS = ["f32", "f64"]
ULP32 = 2.0 ** -24         # one rounding of a stored binary32 value, relative
NS = A.SUBSTEPS


def hermite(n, prec, **kw):
    return Simulation(n, precision=prec, integrator="hermite4", **kw)


def state(sim, cap=None, radii=False):
    """Everything the handle can hand out, as bytes: (bodies, vel, accel), the jerk and, with cap, the scheme's own arrays (and `next`)."""
    out = [x.tobytes() for x in sim.read()] + [sim.read_jerk().tobytes()]
    if cap is not None:
        d = sim.download_neighbor_scheme(cap)
        out += [d[k].tobytes() for k in sorted(d)]
    if radii:
        out.append(sim.download_neighbor_radii()[1].tobytes())
    return out


def errs(sim, ref):
    b, v, a = sim.read()
    j = sim.read_jerk()
    return [norm_err(g[:, :3], w) for g, w in zip((b, v, a, j), ref)]


def started(prec, b0, v0, dt, G, scheme, adapt=None):
    sim = hermite(len(b0), prec)
    sim.init(b0, v0)
    sim.set_params(dt, G)
    sim.set_neighbor_scheme(**scheme)
    if adapt is not None:
        sim.set_neighbor_adapt(**adapt)
    return sim


def case_handle(prec, name, **adapt):
    """A handle set up as a case of the record: (sim, the case, the scheme's keywords, the adaptation's)."""
    e = A.record()["cases"][name]
    b0, v0, kw = A.case_args(e)
    scheme = dict(substeps=NS, cap=e["cap"], **R.radius_args(e["n"], e["per_body"], e["radius"]))
    ad = dict(target=e["target"], **adapt)
    return started(prec, b0, v0, e["dt"], e["G"], scheme, ad), e, scheme, ad


# ---- 1. grow_max = 1: a fixed-radii twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_body", [False, True])
@pytest.mark.parametrize("n", [771, 1025])
@pytest.mark.parametrize("prec", PRECS)
def test_grow_max_one_is_a_fixed_radii_twin_byte_for_byte(prec, n, per_body):
    """With g = 1 the rule cannot move a radius and nothing overflows: the adaptive branch of the start and of the regular time (the
    header from the counts alone, the correction behind the wait, the rule) must leave every bit the fixed-radii code leaves."""
    cap = 24
    b0, v0 = ic.plummer(n, seed=31)
    h = 0.1                                                              # (largest count 9, a member per row on average)
    kw = {"radii": (R.radii_pattern(n) * h).astype(np.float32 if prec == "f32" else np.float64)} if per_body else {"radius": h}
    scheme = dict(substeps=NS, cap=cap, **kw)
    with started(prec, b0, v0, R.DT, 1.0, scheme, dict(target=cap // 2, grow_max=1.0)) as sim, started(prec, b0, v0, R.DT, 1.0, scheme) as twin:
        sim.simulate(R.STEPS)
        twin.simulate(R.STEPS)
        st, tw = sim.neighbor_scheme_stats(), twin.neighbor_scheme_stats()
        built, nxt = sim.download_neighbor_radii()
        assert 0 < tw["max_count"] <= cap and tw["entries"] > 0
        assert state(sim, cap) == state(twin, cap)
        assert st == tw and sim.neighbor_adapt_stats() == dict(enabled=1, rebuilds=0, rows_shrunk=0, last_rebuilds=0)
        fixed = [x.tobytes() for x in twin.download_neighbor_radii()]
        assert [built.tobytes(), nxt.tobytes()] == fixed
        assert built.tobytes() == (kw["radii"] if per_body else np.full(n, h, sim.dtype)).tobytes()


# ---- 2. the recorded cases against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("prec,name", [(p, c) for c in sorted(A.CASES) for p in PRECS if p == "f64" or A.CASES[c]["f32"]])
def test_recorded_case_against_the_restatement(prec, name):
    """f64: every case.  f32: the cases whose initial radius was chosen so that a binary32 run decides every membership as the fp64
    one (n = 256); the margins of the others (>= 1e-9) carry fp64 only."""
    sim, e, _, _ = case_handle(prec, name)
    x, v, a, j, next64, next32, lst, cnt = A.recorded_state(name)
    with sim:
        sim.simulate(A.STEPS)
        got = errs(sim, (x, v, a, j))
        d = sim.download_neighbor_scheme(e["cap"])
        st = dict(sim.neighbor_scheme_stats(), **sim.neighbor_adapt_stats())
        nxt = sim.download_neighbor_radii()[1].astype(np.float64)
    print("%s %s: x %.3g v %.3g a %.3g j %.3g; %s" % (name, prec, *got, st))
    assert st == e["stats"], (st, e["stats"])
    assert d["list"].tobytes() == lst.tobytes() and d["count"].tobytes() == cnt.tobytes()
    for q, g in zip(A.QUANTITIES, got):
        assert g <= (1e-10 if prec == "f64" else 8 * e["f32_err"][q]), (q, g)
    if prec == "f64":
        rel = np.abs(nxt - next64) / np.where(next64 > 0, next64, 1.0)
        print("next: largest relative difference %.3g" % rel.max())
        assert rel.max() <= 1e-14 and ((nxt == 0) == (next64 == 0)).all()
    else:
        ulps = np.abs(nxt - next32) / np.spacing(next32.astype(np.float32)).astype(np.float64)
        print("next: largest difference %.3g binary32 ulp" % ulps.max())
        assert ulps.max() <= 1.0


# ---- 3. a start that rebuilds, against the public queries ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["recover256", "recover771"])
@pytest.mark.parametrize("prec", PRECS)
def test_a_start_with_rebuilds_is_the_queries_at_the_built_radii(prec, name):
    sim, e, _, _ = case_handle(prec, name)
    n, cap = e["n"], e["cap"]
    with sim:
        got = sim.download_neighbor_scheme(cap)
        st, ad = sim.neighbor_scheme_stats(), sim.neighbor_adapt_stats()
        built, nxt = sim.download_neighbor_radii()
        lists, count = sim.neighbor_lists(bodies=(0, n), cap=cap, radii=built)
        want = sim.split_force(bodies=(0, n), jerk=True, radii=built)
        a, j = sim.read(bodies=False, vel=False)[2], sim.read_jerk()
    print("start %s %s: %s %s" % (name, prec, st, ad))
    assert ad["rebuilds"] == ad["last_rebuilds"] >= 1 and ad["rows_shrunk"] >= ad["rebuilds"] and st["builds"] == 1 + ad["rebuilds"]
    assert st["overflowed"] == 0 and st["max_count"] == count.max() <= cap
    for k in ("accel_irr", "jerk_irr", "accel_reg", "jerk_reg"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["list"].tobytes() == lists.tobytes() and got["count"].tobytes() == count.tobytes()
    for tot, p, q in ((a, "accel_irr", "accel_reg"), (j, "jerk_irr", "jerk_reg")):
        assert tot.tobytes() == (want[p].astype(np.float64) + want[q].astype(np.float64)).astype(sim.dtype).tobytes()
    # the rule on the accepted counts, from the built radii (the restatement's own function; one rounding of the handle's precision)
    r = A.rule(built.astype(np.float64), count, e["target"], store=sim.dtype).astype(np.float64)
    assert np.abs(nxt - r).max() <= np.spacing(np.abs(r).astype(sim.dtype)).max()
    assert (built <= np.float64(R.radius_args(n, e["per_body"], e["radius"]).get("radius", np.inf))).all()


# ---- 4. the smallest shapes ----------------------------------------------------------------------------------------------------
def against_restatement(prec, b0, v0, G, dt, steps, scheme, adapt):
    """A handle against ac_adapt_ref on an input that is not in the record; the bounds of test_ac_scheme_gpu.against_restatement:
    f64 1e-10, f32 8 x the error of the binary32-storing restatement of THIS input and no less than 8 roundings.  Rows, counts and
    the stats of both structures exact; `next` within 1e-14 (f64) or one binary32 ulp of the binary32-storing restatement's (f32)."""
    kw = dict(scheme, **adapt)
    with started(prec, b0, v0, dt, G, scheme, adapt) as sim:
        sim.simulate(steps)
        d = sim.download_neighbor_scheme(scheme["cap"])
        st = dict(sim.neighbor_scheme_stats(), **sim.neighbor_adapt_stats())
        built, nxt = sim.download_neighbor_radii()
        ref = A.ac_adapt_ref(b0, v0, G, EPS2, dt, steps, **kw)
        got = errs(sim, A.totals(ref))
    if prec == "f64":
        bound, rn, tol = [1e-10] * 4, ref[10], 1e-14 * np.abs(ref[10])
    else:
        r32 = A.ac_adapt_ref(b0, v0, G, EPS2, dt, steps, store=np.float32, **kw)
        bound = [8 * max(norm_err(x, y), ULP32) for x, y in zip(A.totals(r32, np.float32), A.totals(ref))]
        rn, tol = r32[10], np.spacing(r32[10].astype(np.float32)).astype(np.float64)
    print("%s n=%d: x %.3g v %.3g a %.3g j %.3g (bounds %s); %s" % (prec, len(b0), *got, " ".join("%.3g" % x for x in bound), st))
    assert all(g <= w for g, w in zip(got, bound)), (got, bound)
    assert d["list"].tobytes() == ref[6].tobytes() and d["count"].tobytes() == ref[7].tobytes()
    assert st == ref[8], (st, ref[8])
    assert (np.abs(nxt.astype(np.float64) - rn) <= tol).all() and ((nxt == 0) == (rn == 0)).all()
    return d, built, nxt


@pytest.mark.parametrize("prec", PRECS)
def test_two_bodies(prec):
    b0 = np.array([[-0.25, 0.01, 0, 0.6], [0.25, 0, 0.02, 0.4]], np.float32)
    v0 = np.array([[0, -0.4, 0.05, 0], [0, 0.6, -0.075, 0]], np.float32)
    d, built, nxt = against_restatement(prec, b0, v0, 1.0, R.DT, A.STEPS, dict(radius=0.75, substeps=4, cap=2), dict(target=1))
    assert d["count"].tolist() == [1, 1]


@pytest.mark.parametrize("prec", PRECS)
def test_one_lane_past_a_workgroup(prec):
    """n = 257: the second workgroup of every row kernel holds one body."""
    b0, v0 = ic.plummer(257, seed=9)
    d, built, nxt = against_restatement(prec, b0, v0, 1.0, R.DT / 4, 3, dict(radius=0.15, substeps=2, cap=12), dict(target=4))
    assert 0 < d["count"].max() <= 12 and (nxt != built).any()


def nearest(b):
    x = np.asarray(b, np.float64)[:, :3]
    d = np.sqrt(((x[None] - x[:, None]) ** 2).sum(2))
    np.fill_diagonal(d, np.inf)
    return np.sort(d, axis=1)


@pytest.mark.parametrize("prec", PRECS)
def test_full_rows_next_to_rows_of_radius_zero_and_both_clamps(prec):
    """cap = 5, target 2: the even bodies below 20 hold exactly cap members, the odd ones have radius 0 -- and keep it through both
    clamps --, the rest start at three quarters of a full row's radius.  radius_min and radius_max are both reached."""
    cap = 5
    b0, v0 = ic.plummer(77, seed=6)
    d = nearest(b0)
    full = 0.5 * (d[:, cap - 1] + d[:, cap])
    radii = (0.75 * full).astype(np.float32)
    radii[:20:2] = full[:20:2]
    radii[1:20:2] = 0.0
    lo, hi = float(np.float32(np.median(radii[radii > 0]) * 0.9)), float(np.float32(np.median(radii[radii > 0]) * 1.1))
    with started(prec, b0, v0, R.DT / 16, 1.0, dict(radii=radii, substeps=2, cap=cap)) as plain:
        c0 = plain.download_neighbor_scheme(cap)["count"]
    assert (c0[:20:2] == cap).all() and (c0[1:20:2] == 0).all() and c0.max() == cap
    got, built, nxt = against_restatement(prec, b0, v0, 1.0, R.DT / 16, 2, dict(radii=radii, substeps=2, cap=cap),
                                          dict(target=2, radius_min=lo, radius_max=hi))
    zero = radii == 0
    assert (built[zero] == 0).all() and (nxt[zero] == 0).all() and (got["count"][zero] == 0).all()
    assert (got["accel_irr"][zero] == 0).all() and (got["jerk_irr"][zero] == 0).all()
    live = nxt[~zero]
    assert live.min() == np.asarray(lo, nxt.dtype) and live.max() == np.asarray(hi, nxt.dtype) and ((live > lo) & (live < hi)).any()


@pytest.mark.parametrize("prec", PRECS)
def test_rebuilds_exhausted_at_the_start_fail_the_call_and_leave_the_state(prec):
    """Every body holds all 76 others at any radius one shrink can reach: today's message, x and v untouched, and `next` too -- the
    next call finds what this one found."""
    b0, v0 = ic.plummer(77, seed=5)
    with started(prec, b0, v0, R.DT, 1.0, dict(radius=100.0, substeps=2, cap=8), dict(target=4, max_rebuilds=1)) as sim:
        msgs = []
        for call in (lambda: sim.simulate(1), lambda: sim.download_neighbor_radii(), lambda: sim.simulate(1)):
            with pytest.raises(capi.NBodyError) as e:
                call()
            assert e.value.code == 4, e.value
            msgs.append(str(e.value).split("neighbour list overflow", 1)[1])
        assert msgs[0] == msgs[1] == msgs[2] and msgs[0].startswith(": 77 rows hold more than cap members (largest count 76, cap 8)")
        st, ad = sim.neighbor_scheme_stats(), sim.neighbor_adapt_stats()
        assert (st["builds"], st["overflowed"], st["max_count"], st["regular_steps"]) == (6, 77, 76, 0)
        assert (ad["rebuilds"], ad["rows_shrunk"], ad["last_rebuilds"]) == (3, 3 * 77, 1)
        b, v, _ = sim.read(accel=False)
        assert b.tobytes() == b0.astype(sim.dtype).tobytes() and v.tobytes() == v0.astype(sim.dtype).tobytes()
        sim.set_neighbor_adapt(None)
        sim.set_neighbor_scheme(radius=100.0, substeps=2, cap=128)
        sim.simulate(1)


def runner_into_a_clump():
    """Twelve light bodies within 1e-3 (radius 0: rows that stay empty) and a runner 0.3 away with radius 0.1 that arrives 0.05 from
    them after one step of 1/64: its row then holds 12 at any radius >= 0.051, and one shrink of cbrt(1/12) from ~0.126 gives 0.055."""
    rng = np.random.default_rng(3)
    b = np.zeros((13, 4), np.float32)
    v = np.zeros((13, 4), np.float32)
    b[:12, :3] = rng.uniform(-5e-4, 5e-4, (12, 3))
    b[12, 0] = 0.3
    b[:, 3] = 1e-9
    v[12, 0] = -16.0
    radii = np.zeros(13, np.float32)
    radii[12] = 0.1
    return b, v, radii


@pytest.mark.parametrize("prec", PRECS)
def test_rebuilds_exhausted_at_a_regular_time_keep_the_step_and_stop_the_next(prec):
    b0, v0, radii = runner_into_a_clump()
    scheme, adapt = dict(radii=radii, substeps=2, cap=2), dict(target=1, max_rebuilds=1)
    with pytest.raises(A.Overflow) as ref:
        A.ac_adapt_ref(b0, v0, 1.0, EPS2, R.DT, 1, **dict(scheme, **adapt))
    assert "1 rows, largest count 12, cap 2" in str(ref.value)
    with started(prec, b0, v0, R.DT, 1.0, scheme, adapt) as sim, started(prec, b0, v0, R.DT, 1.0, dict(scheme, cap=16)) as twin:
        assert sim.download_neighbor_scheme(2)["count"].max() == 0
        with pytest.raises(capi.NBodyError) as e:
            sim.simulate(1)
        assert e.value.code == 4 and "neighbour list overflow: 1 rows hold more than cap members (largest count 12, cap 2)" in str(e.value)
        st, ad = sim.neighbor_scheme_stats(), sim.neighbor_adapt_stats()
        assert (st["regular_steps"], st["builds"], st["overflowed"], st["max_count"]) == (1, 3, 1, 12) and ad["last_rebuilds"] == 1
        twin.simulate(1)                                                  # no member anywhere during the step: the same arithmetic
        kept = [x.tobytes() for x in sim.read(accel=False)[:2]]
        assert kept == [x.tobytes() for x in twin.read(accel=False)[:2]] and kept[0] != b0.astype(sim.dtype).tobytes()
        with pytest.raises(capi.NBodyError) as again:
            sim.simulate(1)
        assert again.value.code == 4 and str(again.value) == str(e.value)
        assert kept == [x.tobytes() for x in sim.read(accel=False)[:2]]
        sim.set_neighbor_scheme(radii=radii, substeps=2, cap=16)         # as ever: setting the scheme again clears it (and adaptation)
        assert sim.neighbor_adapt_stats()["enabled"] == 0
        sim.simulate(1)


# ---- 5. the checkpoint ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fixed", "track256", "recover256", "recover771"])
@pytest.mark.parametrize("prec", PRECS)
def test_a_restored_handle_continues_bit_for_bit(prec, mode):
    """Three steps, the checkpoint into a fresh handle, three more on both: every array the handles can hand out is identical, with
    adaptation off, on, and across steps that rebuild (recover*: the record's last build rebuilt; asserted below on the copy)."""
    a, e, scheme, adapt = case_handle(prec, "track256" if mode == "fixed" else mode)
    if mode == "fixed":
        adapt = None
        a.set_neighbor_adapt(None)
    cap = e["cap"]
    with a, hermite(e["n"], prec) as b:
        a.simulate(3)
        ck = a.neighbor_scheme_checkpoint(cap)
        assert ck["adaptive"] == (adapt is not None)
        b.restore_neighbor_scheme(ck, scheme=scheme, adapt=adapt)
        assert b.neighbor_scheme_stats()["builds"] == 0                  # the upload counts no build: the start did not run
        assert state(b, cap, True) == state(a, cap, True)
        a.simulate(3)
        b.simulate(3)
        assert state(b, cap, True) == state(a, cap, True)
        assert [x.tobytes() for x in a.download_neighbor_radii()] == [x.tobytes() for x in b.download_neighbor_radii()]
        sb, ab = b.neighbor_scheme_stats(), b.neighbor_adapt_stats()
        assert sb["builds"] == 3 + ab["rebuilds"] and sb["regular_steps"] == 3
        if mode.startswith("recover"):
            assert ab["rebuilds"] >= 1
        # ... and a restore through (x, v) alone is NOT: the start's components are not the running ones
        if mode == "fixed":
            with started(prec, ck["bodies"], ck["vel"], ck["dt"], ck["G"], scheme) as c:
                assert c.download_neighbor_scheme(cap)["accel_irr"].tobytes() != ck["scheme"]["accel_irr"].tobytes()


@pytest.mark.parametrize("prec", PRECS)
def test_three_steps_at_once_one_by_one_and_restored_in_between(prec):
    (a, e, scheme, adapt), (b, _, _, _) = case_handle(prec, "recover256"), case_handle(prec, "recover256")
    cap = e["cap"]
    with a, b, hermite(e["n"], prec) as c:
        a.simulate(3)
        b.simulate(1)
        c.restore_neighbor_scheme(b.neighbor_scheme_checkpoint(cap), scheme=scheme, adapt=adapt)
        for _ in range(2):
            b.simulate(1)
            c.simulate(1)
        assert state(a, cap, True) == state(b, cap, True) == state(c, cap, True)
        assert a.neighbor_scheme_stats() == b.neighbor_scheme_stats() and a.neighbor_adapt_stats() == b.neighbor_adapt_stats()


@pytest.mark.parametrize("prec", PRECS)
def test_a_changed_dt_after_the_upload_runs_the_start(prec):
    a, e, scheme, adapt = case_handle(prec, "track256")
    cap, n = e["cap"], e["n"]
    with a, hermite(n, prec) as b:
        a.simulate(2)
        ck = a.neighbor_scheme_checkpoint(cap)
        b.restore_neighbor_scheme(ck, scheme=scheme, adapt=adapt)
        b.set_params(e["dt"] / 2, e["G"])
        got = b.download_neighbor_scheme(cap)
        assert b.neighbor_scheme_stats()["builds"] == 1
        built = b.download_neighbor_radii()[0]
        assert built.tobytes() == ck["radii"].tobytes()                  # the start is cut by the uploaded `next`
        want = b.split_force(bodies=(0, n), jerk=True, radii=built)
        assert all(got[k].tobytes() == want[k].tobytes() for k in want) and got["accel_irr"].tobytes() != ck["scheme"]["accel_irr"].tobytes()


def test_an_upload_is_checked_before_it_is_copied():
    a, e, scheme, adapt = case_handle("f32", "track256")
    cap, n = e["cap"], e["n"]
    with a, hermite(n, "f32") as b, Simulation(n) as leap:
        a.simulate(1)
        ck = a.neighbor_scheme_checkpoint(cap)
        arrays = dict(ck["scheme"], radii=ck["radii"])
        for sim, what in ((leap, "Hermite"), (b, "nb_set_neighbor_scheme")):          # a leapfrog handle, a handle without the scheme
            for call in (lambda: sim.upload_neighbor_scheme(**arrays), lambda: sim.set_neighbor_adapt(6), lambda: sim.download_neighbor_radii()):
                with pytest.raises(capi.NBodyError) as err:
                    call()
                assert err.value.code == 4 and what in str(err.value), str(err.value)
        b.set_neighbor_scheme(**scheme)
        b.set_neighbor_adapt(**adapt)
        for missing in ("nb_upload has not", "nb_set_params has not"):                                 # an upload before nb_upload / nb_set_params
            with pytest.raises(capi.NBodyError) as err:
                b.upload_neighbor_scheme(**arrays)
            assert err.value.code == 4 and missing in str(err.value), str(err.value)
            b.init(ck["bodies"], ck["vel"]) if missing.startswith("nb_upload") else b.set_params(ck["dt"], ck["G"])

        def rejected(field, **change):
            with pytest.raises(capi.NBodyError) as err:
                b.upload_neighbor_scheme(**dict(arrays, **change))
            assert err.value.code == 1 and "nb_upload_neighbor_scheme" in str(err.value) and field in str(err.value), str(err.value)
        count = arrays["count"].copy()
        count[5] = cap + 1
        rejected("count[5]", count=count)
        row = int(np.argmax(arrays["count"] > 0))
        for bad, field in ((n, "list[%d][0]" % row), (row, "list[%d][0]" % row)):     # not a body; the row's own body
            lst = arrays["list"].copy()
            lst[row, 0] = bad
            rejected(field, list=lst)
        for k, x in enumerate((-0.1, float("inf"), float("nan"))):
            r = arrays["radii"].copy()
            r[7 + k] = x
            rejected("radii[%d]" % (7 + k), radii=r)
        rejected("radii", radii=None)                                    # missing with adaptation on
        rejected("accel_reg", accel_reg=None)
        b.set_neighbor_adapt(None)
        rejected("radii")                                                # given with adaptation off
        for tgt, field in ((0, "target"), (cap // 2 + 1, "target")):
            with pytest.raises(capi.NBodyError) as err:
                b.set_neighbor_adapt(tgt)
            assert err.value.code == 1 and "nb_set_neighbor_adapt" in str(err.value) and field in str(err.value)
        assert b.neighbor_adapt_stats()["enabled"] == 0 and b.neighbor_scheme_stats()["builds"] == 0
        b.set_neighbor_adapt(**adapt)
        b.upload_neighbor_scheme(**arrays)                               # and the untouched arrays pass
        a.simulate(1)
        b.simulate(1)
        assert state(a, cap, True) == state(b, cap, True)


# ---- 6. the cold collapse ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_the_cold_collapse_runs_past_the_step_where_fixed_radii_overflow(prec):
    c = A.record()["collapse"]
    b0, v0 = A.fixture(c["fixture"])
    v0 = np.zeros_like(v0)
    scheme = dict(radius=c["radius"], substeps=NS, cap=c["cap"])
    e0 = A.energy(b0, v0, c["G"], EPS2)
    with started(prec, b0, v0, c["dt"], c["G"], scheme) as fixed, started(prec, b0, v0, c["dt"], c["G"], scheme, dict(target=c["target"])) as sim:
        with pytest.raises(capi.NBodyError) as err:
            fixed.simulate(c["steps"])
        done = fixed.neighbor_scheme_stats()["regular_steps"]
        assert err.value.code == 4 and "overflow" in str(err.value) and done <= c["steps"]
        worst = 0
        for _ in range(c["steps"]):
            sim.simulate(1)
            worst = max(worst, sim.neighbor_scheme_stats()["max_count"])
        st, ad = sim.neighbor_scheme_stats(), sim.neighbor_adapt_stats()
        b, v, _ = sim.read(accel=False)
    de = abs(A.energy(b, v, c["G"], EPS2) - e0) / abs(e0)
    print("collapse %s: fixed radii stop at regular step %d (the restatement: %d); adaptive to %d: |dE/E0| %.3g (the restatement: %.3g), %s %s"
          % (prec, done, c["K"], c["steps"], de, c["dE_" + prec], st, ad))
    assert st["regular_steps"] == c["steps"] and worst <= c["cap"] and st["overflowed"] == 0 and ad["rebuilds"] >= 1
    assert de <= 2 * c["dE_" + prec]


# ---- 7. back to a handle without it --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["adapt_off", "scheme_again"])
@pytest.mark.parametrize("prec", PRECS)
def test_switching_adaptation_off_leaves_a_handle_that_never_had_it(prec, how):
    a, e, scheme, _ = case_handle(prec, "recover256")
    cap = e["cap"]
    big = dict(scheme, cap=64, radius=0.12)
    with a:
        a.simulate(2)
        x, v, _ = a.read()
        if how == "adapt_off":                                           # the scheme's own radii (0.70: rows of 8 cannot hold them) are back
            a.set_neighbor_adapt(None)
            assert a.neighbor_adapt_stats() == dict(enabled=0, rebuilds=0, rows_shrunk=0, last_rebuilds=0)
            with pytest.raises(capi.NBodyError) as err:
                a.simulate(1)
            assert err.value.code == 4 and "overflow" in str(err.value)
        a.set_neighbor_scheme(**big)
        assert a.neighbor_adapt_stats()["enabled"] == 0
        a.simulate(2)
        with started(prec, x, v, e["dt"], e["G"], big) as fresh:
            fresh.simulate(2)
            assert state(a, 64) == state(fresh, 64) and a.neighbor_scheme_stats() == fresh.neighbor_scheme_stats()
            assert [r.tobytes() for r in a.download_neighbor_radii()] == [np.full(e["n"], 0.12, a.dtype).tobytes()] * 2


@pytest.mark.parametrize("prec", PRECS)
def test_queries_behind_adaptive_steps_equal_a_fresh_twin(prec):
    sim, e, _, _ = case_handle(prec, "recover256")
    n = e["n"]
    with sim, hermite(n, prec) as twin:
        sim.simulate(3)

        def ask(s):
            out = list(s.neighbors(bodies=(0, n), radius=0.3)) + list(s.knn(bodies=(0, n), k=6)) + list(s.field(bodies=(0, n)))
            out += list(s.neighbor_lists(bodies=(0, n), radius=0.1, cap=16))
            sp = s.split_force(bodies=(0, n), radius=0.3, jerk=True)
            return [np.asarray(x).tobytes() for x in out if x is not None] + [sp[k].tobytes() for k in sorted(sp)]
        got = ask(sim)
        x, v, _ = sim.read()
        twin.init(x, v)
        twin.set_params(e["dt"], e["G"])
        assert got == ask(twin)
        assert x.tobytes() != A.fixture("plummer256")[0].astype(sim.dtype).tobytes()


def test_setting_adaptation_runs_the_start_again_and_timing_reports_steps():
    sim, e, scheme, adapt = case_handle("f32", "track256")
    with sim:
        sim.simulate(1)
        builds = sim.neighbor_scheme_stats()["builds"]
        sim.set_neighbor_adapt(**adapt)                                  # with any argument: the start runs again, from the scheme's radii
        built = sim.download_neighbor_radii()[0]
        assert sim.neighbor_scheme_stats()["builds"] == builds + 1 and built.tobytes() == np.full(e["n"], e["radius"], np.float32).tobytes()
        sim.enable_timing(True)
        sim.simulate(3)
        force, integrate, exchange, launches = sim.step_times()
        assert launches == 3 and force > 0 and integrate == 0 and exchange == 0
