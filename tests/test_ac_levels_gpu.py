"""Block individual irregular steps inside the neighbour scheme (Simulation.set_neighbor_levels) on the GPU: the two frozen limits
against handles without levels, byte for byte; uploaded mixed levels and the recorded dynamic runs against the restatement
tests/ac_levels_ref.py and the record tests/golden/ac_levels.json; the bitwise invariants; the smallest shapes; the checkpoint; what
stales the levels; the queries behind stepped handles; every error; and the way back to a handle without levels."""
import functools

import numpy as np
import pytest

from nbody3d_amd import Simulation, capi, ic

import ac_levels_ref as LR
import ac_ref as R
from ac_ref import EPS2, norm_err

pytestmark = pytest.mark.gpu

PRECS = ["f32", "f64"]
ULP32 = 2.0 ** -24         # one rounding of a stored binary32 value, relative


def hermite(n, prec, **kw):
    return Simulation(n, precision=prec, integrator="hermite4", **kw)


def state(sim, cap=None, radii=False, levels=False):
    """Everything the handle can hand out, as bytes: (bodies, vel, accel), the jerk and, with cap, the scheme's own arrays."""
    out = [x.tobytes() for x in sim.read()] + [sim.read_jerk().tobytes()]
    if cap is not None:
        d = sim.download_neighbor_scheme(cap)
        out += [d[k].tobytes() for k in sorted(d)]
    if radii:
        out.append(sim.download_neighbor_radii()[1].tobytes())
    if levels:
        out.append(sim.download_neighbor_levels().tobytes())
    return out


def errs(sim, ref):
    b, v, a = sim.read()
    j = sim.read_jerk()
    return [norm_err(g[:, :3], w) for g, w in zip((b, v, a, j), ref)]


def started(prec, b0, v0, dt, G, scheme, adapt=None, levels=None):
    sim = hermite(len(b0), prec)
    sim.init(b0, v0)
    sim.set_params(dt, G)
    sim.set_neighbor_scheme(**scheme)
    if adapt is not None:
        sim.set_neighbor_adapt(**adapt)
    if levels is not None:
        sim.set_neighbor_levels(**levels)
    return sim


def plummer_case(n, prec, per_body):
    b0, v0 = ic.plummer(n, seed=31)
    h = 0.1                                                              # (largest count 9, a member per row on average)
    kw = {"radii": (R.radii_pattern(n) * h).astype(np.float32 if prec == "f32" else np.float64)} if per_body else {"radius": h}
    return b0, v0, kw


TWINS = [(771, 2.0 ** -8, True), (1025, 2.0 ** -6, False)]


# ---- 1. the two frozen limits: byte-for-byte twins -----------------------------------------------------------------------------
@pytest.mark.parametrize("adapt", [False, True])
@pytest.mark.parametrize("n,dt,per_body", TWINS)
@pytest.mark.parametrize("prec", PRECS)
def test_frozen_at_L_is_a_handle_without_levels_byte_for_byte(prec, n, dt, per_body, adapt):
    """dt is a power of two: every T(k) is exact and tau0 + hs of the shared kernel is the same number.  One body-step per body
    and tick: a missed or doubled one, a wrong h or a prediction from the wrong time changes bits."""
    cap = 24
    b0, v0, kw = plummer_case(n, prec, per_body)
    scheme = dict(substeps=8, cap=cap, **kw)
    ad = dict(target=cap // 2) if adapt else None
    with started(prec, b0, v0, dt, 1.0, scheme, ad, dict(min_level=3, frozen=True)) as sim, started(prec, b0, v0, dt, 1.0, scheme, ad) as twin:
        sim.simulate(3)
        twin.simulate(3)
        assert twin.neighbor_scheme_stats()["entries"] > 0
        assert state(sim, cap, adapt) == state(twin, cap, adapt)
        assert sim.neighbor_scheme_stats() == twin.neighbor_scheme_stats()
        ls = sim.neighbor_level_stats()
        assert (ls["enabled"], ls["regular_steps"], ls["ticks"], ls["block_steps"], ls["body_steps"], ls["clamped"], ls["finest_level"]) == (1, 3, 24, 24, 24 * n, 0, 3)
        assert (sim.download_neighbor_levels() == 3).all()
        assert twin.neighbor_level_stats() == dict(enabled=0, regular_steps=0, ticks=0, block_steps=0, body_steps=0, entries=0, clamped=0, finest_level=0)


@pytest.mark.parametrize("n,dt,per_body", TWINS)
@pytest.mark.parametrize("prec", PRECS)
def test_frozen_at_zero_is_a_handle_with_one_substep_byte_for_byte(prec, n, dt, per_body):
    """substeps = 8, every level 0: seven empty ticks and one step of dt per regular step -- the shared scheme at N_sub = 1."""
    cap = 24
    b0, v0, kw = plummer_case(n, prec, per_body)
    with started(prec, b0, v0, dt, 1.0, dict(substeps=8, cap=cap, **kw), None, dict(min_level=0, frozen=True)) as sim, \
            started(prec, b0, v0, dt, 1.0, dict(substeps=1, cap=cap, **kw)) as twin:
        sim.simulate(3)
        twin.simulate(3)
        assert state(sim, cap) == state(twin, cap)
        ls = sim.neighbor_level_stats()
        assert (ls["ticks"], ls["block_steps"], ls["body_steps"], ls["finest_level"]) == (24, 3, 3 * n, 0)
        assert sim.neighbor_scheme_stats()["substeps"] == 24 and twin.neighbor_scheme_stats()["substeps"] == 3


# ---- 2. uploaded mixed levels, frozen, against the restatement -----------------------------------------------------------------
MIXED_STEPS = 2


@functools.lru_cache(maxsize=None)
def mixed_ref(n, L):
    b0, v0, kw = plummer_case(n, "f32", n == 771)
    lev = (np.arange(n) % (L + 1)).astype(np.uint8)
    out = {}
    for store in (np.float64, np.float32):
        m = []
        out[store] = LR.ac_levels_ref(b0, v0, 1.0, EPS2, R.DT, MIXED_STEPS, L=L, cap=24, frozen=True, levels=lev, store=store, margins=m, **kw)
        assert min(m) >= 1e-5, (n, L, min(m))                             # no membership a rounding could flip
    return b0, v0, kw, lev, out


@pytest.mark.parametrize("L", [3, 6])
@pytest.mark.parametrize("n", [256, 771, 1025])
@pytest.mark.parametrize("prec", PRECS)
def test_uploaded_mixed_levels_against_the_restatement(prec, n, L):
    """l_i = i mod (L + 1): every tick has another active set.  f64 within 1e-10, f32 within 8 x the error of the binary32-storing
    restatement (no less than 8 roundings); block steps, body-steps, entries and ticks exact."""
    b0, v0, kw, lev, refs = mixed_ref(n, L)
    kw = {k: (np.asarray(x, np.float32 if prec == "f32" else np.float64) if k == "radii" else x) for k, x in kw.items()}
    ref, r32 = refs[np.float64], refs[np.float32]
    with started(prec, b0, v0, R.DT, 1.0, dict(substeps=2 ** L, cap=24, **kw), None, dict(min_level=0, frozen=True)) as sim:
        d0 = sim.download_neighbor_scheme(24)                             # runs the scheme's start: the upload needs it current
        sim.upload_neighbor_levels(lev)
        sim.simulate(MIXED_STEPS)
        got = errs(sim, R.totals(ref))
        ls, d = sim.neighbor_level_stats(), sim.download_neighbor_scheme(24)
        assert sim.download_neighbor_levels().tobytes() == lev.tobytes()
    bound = [1e-10] * 4 if prec == "f64" else [8 * max(norm_err(x, y), ULP32) for x, y in zip(R.totals(r32, np.float32), R.totals(ref))]
    print("mixed %s n=%d L=%d: x %.3g v %.3g a %.3g j %.3g (bounds %s); %s" % (prec, n, L, *got, " ".join("%.3g" % x for x in bound), ls))
    assert ls == ref[10], (ls, ref[10])
    assert ls["body_steps"] == MIXED_STEPS * LR.body_steps_of(lev, L) and ls["block_steps"] == ls["ticks"] == MIXED_STEPS * 2 ** L
    assert d["list"].tobytes() == ref[6].tobytes() and d["count"].tobytes() == ref[7].tobytes() and d0["count"].max() > 0
    assert all(g <= w for g, w in zip(got, bound)), (got, bound)


# ---- 3. dynamic levels ---------------------------------------------------------------------------------------------------------
def recorded_handle(prec, name, m):
    e = R.record()["fixtures"][name]
    b0, v0 = R.fixture(name)
    scheme = dict(substeps=2 ** LR.L_REC, cap=e["cap"], **R.radius_args(e["n"], e["per_body"], e["radius"]))
    return started(prec, b0, v0, e["dt"], e["G"], scheme, None, dict(min_level=m, eta=LR.ETA_REC)), e, scheme


@pytest.mark.parametrize("m", LR.MIN_LEVELS_REC)
@pytest.mark.parametrize("name", R.FIXTURES)
def test_recorded_dynamic_run_f64(name, m):
    """Every final level and every counter EQUAL, the state within 1e-10 (the record asserts that noise of 1e-12 on every list sum
    changes no level).  Empty ticks are part of every run: 88, 158 and 9 or 19 of 256 ticks have a due body."""
    ent = LR.record()["runs"]["%s_m%d" % (name, m)]
    sim, e, _ = recorded_handle("f64", name, m)
    with sim:
        sim.simulate(LR.STEPS_REC)
        got = errs(sim, LR.recorded_state(name, m))
        lev, ls, st = sim.download_neighbor_levels(), sim.neighbor_level_stats(), sim.neighbor_scheme_stats()
    print("%s min_level %d: x %.3g v %.3g a %.3g j %.3g; %s" % (name, m, *got, ls))
    assert lev.tolist() == ent["levels"], np.nonzero(lev != np.array(ent["levels"]))[0]
    assert ls == ent["level_stats"], (ls, ent["level_stats"])
    assert st == ent["scheme_stats"], (st, ent["scheme_stats"])
    assert all(g <= 1e-10 for g in got), got


@pytest.mark.parametrize("m", LR.MIN_LEVELS_REC)
@pytest.mark.parametrize("name", ["plummer256", "plummer1024"])
def test_dynamic_levels_f32_hold_their_invariants(name, m):
    """binary32 decisions are not pinned: step(3) = 3 x step(1), two handles agree, the levels stay inside
    [min_level, L], and the body-steps of every regular step lie where the levels allow: at least n 2^min_level, at most n 2^L.
    (A level may change at any tick inside a regular step, so the levels downloaded at the regular times bound the count and do
    not fix it; with frozen levels the count is exact: test_uploaded_mixed_levels_against_the_restatement.)"""
    L = LR.L_REC
    (a, e, _), (b, _, _) = recorded_handle("f32", name, m), recorded_handle("f32", name, m)
    n, cap = e["n"], e["cap"]
    with a, b:
        a.simulate(3)
        before = 0
        for _ in range(3):
            b.simulate(1)
            lev, ls = b.download_neighbor_levels(), b.neighbor_level_stats()
            assert m <= int(lev.min()) and int(lev.max()) <= L
            assert n * 2 ** m <= ls["body_steps"] - before <= n * 2 ** L
            before = ls["body_steps"]
        assert state(a, cap, False, True) == state(b, cap, False, True)
        assert a.neighbor_level_stats() == b.neighbor_level_stats() and a.neighbor_scheme_stats() == b.neighbor_scheme_stats()
        ls = a.neighbor_level_stats()
        assert ls["ticks"] == 3 * 2 ** L and 0 < ls["block_steps"] <= ls["ticks"] and ls["entries"] > 0 and ls["finest_level"] >= int(lev.max())
        print("%s f32 min_level %d: %s, final levels %s" % (name, m, ls, np.bincount(lev).tolist()))


@pytest.mark.parametrize("prec", PRECS)
def test_three_steps_at_once_one_by_one_and_on_a_second_handle_with_adaptation(prec):
    e = R.record()["fixtures"]["plummer256"]
    b0, v0 = R.fixture("plummer256")
    scheme, ad, lv = dict(substeps=8, cap=e["cap"], radius=e["radius"]), dict(target=4), dict(min_level=1)
    with started(prec, b0, v0, e["dt"], 1.0, scheme, ad, lv) as a, started(prec, b0, v0, e["dt"], 1.0, scheme, ad, lv) as b:
        a.simulate(3)
        for _ in range(3):
            b.simulate(1)
        assert state(a, e["cap"], True, True) == state(b, e["cap"], True, True)
        assert a.neighbor_level_stats() == b.neighbor_level_stats()


# ---- 4. small and edge shapes --------------------------------------------------------------------------------------------------
def against_restatement(prec, b0, v0, G, dt, steps, scheme, L, **lv):
    """A handle with dynamic levels against ac_levels_ref on an input that is not in the record.  f64: every level and counter
    equal, the state within 1e-10.  f32: the levels inside their range and the counters consistent (decisions are not pinned)."""
    with started(prec, b0, v0, dt, G, scheme, None, lv) as sim:
        sim.simulate(steps)
        lev, ls, d = sim.download_neighbor_levels(), sim.neighbor_level_stats(), sim.download_neighbor_scheme(scheme["cap"])
        dm = []
        ref = LR.ac_levels_ref(b0, v0, G, EPS2, dt, steps, L=L, dmargins=dm, **{k: x for k, x in scheme.items() if k != "substeps"}, **lv)
        got = errs(sim, R.totals(ref))
    print("%s n=%d: x %.3g v %.3g a %.3g j %.3g; %s; smallest decision margin %.3g" % (prec, len(b0), *got, ls, min(dm) if dm else np.inf))
    m = lv.get("min_level", 0)
    assert m <= int(lev.min()) and int(lev.max()) <= L and ls["ticks"] == steps * 2 ** L and 0 < ls["block_steps"] <= ls["ticks"]
    if prec == "f64":
        assert not dm or min(dm) >= 1e-9
        assert lev.tobytes() == ref[8].tobytes() and ls == ref[10], (ls, ref[10])
        assert d["list"].tobytes() == ref[6].tobytes() and d["count"].tobytes() == ref[7].tobytes()
        assert all(g <= 1e-10 for g in got), got
    return lev, ls, d


@pytest.mark.parametrize("prec", PRECS)
def test_two_bodies(prec):
    b0 = np.array([[-0.25, 0.01, 0, 0.6], [0.25, 0, 0.02, 0.4]], np.float32)
    v0 = np.array([[0, -0.4, 0.05, 0], [0, 0.6, -0.075, 0]], np.float32)
    lev, ls, d = against_restatement(prec, b0, v0, 1.0, R.DT, 4, dict(radius=0.75, substeps=4, cap=2), 2)
    assert d["count"].tolist() == [1, 1]


@pytest.mark.parametrize("prec", PRECS)
def test_one_lane_past_a_workgroup(prec):
    """n = 257: the second workgroup of every row kernel holds one body."""
    b0, v0 = ic.plummer(257, seed=9)
    lev, ls, d = against_restatement(prec, b0, v0, 1.0, R.DT, 3, dict(radius=0.15, substeps=8, cap=12), 3, min_level=1)
    assert 0 < d["count"].max() <= 12 and ls["body_steps"] < 3 * 257 * 8


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("prec", PRECS)
def test_one_substep_has_one_level(prec, frozen):
    """substeps = 1: L = 0, the only level -- a handle without levels, byte for byte."""
    b0, v0, kw = plummer_case(257, prec, False)
    scheme = dict(substeps=1, cap=24, **kw)
    with started(prec, b0, v0, R.DT, 1.0, scheme, None, dict(min_level=0, frozen=frozen)) as sim, started(prec, b0, v0, R.DT, 1.0, scheme) as twin:
        sim.simulate(3)
        twin.simulate(3)
        assert state(sim, 24) == state(twin, 24)
        ls = sim.neighbor_level_stats()
        assert (ls["ticks"], ls["block_steps"], ls["body_steps"], ls["finest_level"]) == (3, 3, 3 * 257, 0)


def nearest(b):
    x = np.asarray(b, np.float64)[:, :3]
    d = np.sqrt(((x[None] - x[:, None]) ** 2).sum(2))
    np.fill_diagonal(d, np.inf)
    return np.sort(d, axis=1)


@pytest.mark.parametrize("prec", PRECS)
def test_full_rows_next_to_rows_of_radius_zero(prec):
    """cap = 5: the even bodies below 20 hold exactly cap members, the odd ones have radius 0 and an empty row: tau = inf, so
    they coarsen to min_level and stay there."""
    cap = 5
    b0, v0 = ic.plummer(77, seed=6)
    dd = nearest(b0)
    full = 0.5 * (dd[:, cap - 1] + dd[:, cap])
    radii = (0.75 * full).astype(np.float32)
    radii[:20:2] = full[:20:2]
    radii[1:20:2] = 0.0
    dt = R.DT / 4                                                        # (no row outgrows cap in four steps of it: membership margin 1.3e-3)
    lev, ls, d = against_restatement(prec, b0, v0, 1.0, dt, 4, dict(radii=radii.astype(np.float32 if prec == "f32" else np.float64), substeps=8, cap=cap), 3, min_level=1)
    first = LR.ac_levels_ref(b0, v0, 1.0, EPS2, dt, 0, L=3, cap=cap, radii=radii)[7]
    assert (first[:20:2] == cap).all() and (d["count"][1:20:2] == 0).all() and ls["body_steps"] > 4 * 77 * 2
    assert (lev[1:20:2] == 1).all() and (lev[d["count"] == 0] == 1).all()


@pytest.mark.parametrize("prec", PRECS)
def test_every_body_in_every_row(prec):
    A = R.ALL_MEMBERS
    b0, v0 = R.fixture("plummer1024")
    b0, v0 = b0[:A["n"]].copy(), v0[:A["n"]].copy()
    lev, ls, d = against_restatement(prec, b0, v0, A["G"], A["dt"], 3, dict(radius=A["radius"], substeps=A["substeps"], cap=A["cap"]), 2)
    assert (d["count"] == A["n"] - 1).all()


def two_clusters():
    """Two cold, light clumps of 32 bodies, 1 apart, closing at 8 (test_ac_scheme_gpu.two_clusters)."""
    rng = np.random.default_rng(12)
    b = np.zeros((64, 4), np.float32)
    v = np.zeros((64, 4), np.float32)
    b[:, :3] = rng.uniform(-0.05, 0.05, (64, 3))
    b[:32, 0] -= 0.5
    b[32:, 0] += 0.5
    b[:, 3] = 1e-3 / 64
    v[:32, 0], v[32:, 0] = 4.0, -4.0
    return b, v


@pytest.mark.parametrize("prec", PRECS)
def test_an_overflow_at_a_regular_time_keeps_its_policy_with_levels_on(prec):
    b0, v0 = two_clusters()
    n, cap, big = len(b0), 40, 128
    lv = dict(min_level=1)
    with started(prec, b0, v0, R.DT, 1.0, dict(radius=0.5, substeps=4, cap=cap), None, lv) as sim, \
            started(prec, b0, v0, R.DT, 1.0, dict(radius=0.5, substeps=4, cap=big), None, lv) as twin:
        done = None
        for k in range(1, 13):
            try:
                sim.simulate(1)
            except capi.NBodyError as e:
                done, err = k, e
                break
        assert done is not None and done > 1 and err.code == 4, done
        twin.simulate(done)
        tc = twin.download_neighbor_scheme(big)["count"]
        for number in ("%d rows" % (tc > cap).sum(), "largest count %d" % tc.max(), "cap %d" % cap):
            assert number in str(err)
        assert state(sim) == state(twin)                                 # that step's state is complete
        assert sim.neighbor_level_stats() == twin.neighbor_level_stats()
        with pytest.raises(capi.NBodyError) as again:
            sim.simulate(1)
        assert again.value.code == 4 and str(again.value) == str(err)
        assert state(sim) == state(twin)
        sim.set_neighbor_scheme(radius=0.5, substeps=4, cap=big)         # clears it, and switches the levels off
        assert sim.neighbor_level_stats()["enabled"] == 0
        sim.simulate(2)


# ---- 5. the checkpoint ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adapt", [False, True])
@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("prec", PRECS)
def test_a_restored_handle_continues_bit_for_bit(prec, frozen, adapt):
    """Two steps, the checkpoint into a fresh handle, two more on both.  Without the levels the restored handle would start them by
    rule and part ways: asserted on a third handle."""
    e = R.record()["fixtures"]["plummer256"]
    b0, v0 = R.fixture("plummer256")
    cap = e["cap"]
    scheme, ad, lv = dict(substeps=8, cap=cap, radius=e["radius"]), dict(target=4) if adapt else None, dict(min_level=0, frozen=frozen)
    with started(prec, b0, v0, e["dt"], 1.0, scheme, ad, lv) as a, hermite(e["n"], prec) as b, hermite(e["n"], prec) as c:
        if frozen:
            a.download_neighbor_scheme(cap)
            a.upload_neighbor_levels((np.arange(e["n"]) % 4).astype(np.uint8))
        a.simulate(2)
        ck = a.neighbor_scheme_checkpoint(cap)
        assert ck["levels"].tobytes() == a.download_neighbor_levels().tobytes()
        b.restore_neighbor_scheme(ck, scheme=scheme, adapt=ad, levels=lv)
        assert b.neighbor_scheme_stats()["builds"] == 0 and b.neighbor_level_stats()["body_steps"] == 0
        assert state(b, cap, adapt, True) == state(a, cap, adapt, True)
        a.simulate(2)
        b.simulate(2)
        assert state(b, cap, adapt, True) == state(a, cap, adapt, True)
        if frozen:                                                       # an upload without levels starts them by rule: min_level everywhere
            c.restore_neighbor_scheme(dict(ck, levels=None), scheme=scheme, adapt=ad, levels=lv)
            assert (c.download_neighbor_levels() == 0).all()
            c.simulate(2)
            assert state(c, cap) != state(a, cap)


# ---- 6. what stales the levels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_what_stales_the_levels_runs_the_start_rule(prec):
    """An upload of the scheme without levels, a changed dt, a changed G and nb_set_neighbor_adapt: the levels are the host rule on
    the downloaded components (f64: equal; f32: the components are binary32, the rule's arithmetic is fp64 on both sides: equal)."""
    e = R.record()["fixtures"]["plummer256"]
    b0, v0 = R.fixture("plummer256")
    cap, L, m, eta = e["cap"], 6, 1, 0.02
    scheme = dict(substeps=2 ** L, cap=cap, radius=e["radius"])

    def rule(sim, dt):
        d = sim.download_neighbor_scheme(cap)
        return LR.start_rule(d["accel_irr"], d["jerk_irr"], d["accel_reg"], d["jerk_reg"], dt, eta, m, L)

    with started(prec, b0, v0, e["dt"], 1.0, scheme, None, dict(min_level=m, eta=eta)) as sim:
        first = sim.download_neighbor_levels()
        assert first.tobytes() == rule(sim, e["dt"]).tobytes() and len(set(first.tolist())) > 1
        sim.simulate(2)
        moved = sim.download_neighbor_levels()
        # a changed dt
        sim.set_params(e["dt"] / 2, 1.0)
        lev = sim.download_neighbor_levels()
        assert lev.tobytes() == rule(sim, e["dt"] / 2).tobytes()
        # a changed G
        sim.set_params(e["dt"] / 2, 2.0)
        lev = sim.download_neighbor_levels()
        assert lev.tobytes() == rule(sim, e["dt"] / 2).tobytes()
        # nb_set_neighbor_adapt
        sim.simulate(1)
        sim.set_neighbor_adapt(target=4)
        lev = sim.download_neighbor_levels()
        assert lev.tobytes() == rule(sim, e["dt"] / 2).tobytes() and sim.neighbor_level_stats()["enabled"] == 1
        sim.set_neighbor_adapt(None)
        # an upload of the scheme without levels
        sim.simulate(1)
        ck = sim.neighbor_scheme_checkpoint(cap)
        sim.upload_neighbor_scheme(**ck["scheme"])
        lev = sim.download_neighbor_levels()
        assert lev.tobytes() == rule(sim, e["dt"] / 2).tobytes()
        # nb_set_neighbor_levels itself, and its counters
        sim.simulate(1)
        sim.set_neighbor_levels(min_level=m, eta=eta)
        assert sim.neighbor_level_stats() == dict(enabled=1, regular_steps=0, ticks=0, block_steps=0, body_steps=0, entries=0, clamped=0, finest_level=0)
        assert sim.download_neighbor_levels().tobytes() == rule(sim, e["dt"] / 2).tobytes()
        assert moved.shape == first.shape


# ---- 7. queries behind stepped handles -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_queries_behind_level_steps_equal_a_fresh_twin(prec):
    sim, e, _ = recorded_handle(prec, "plummer256", 1)
    n = e["n"]
    with sim, hermite(n, prec) as twin:
        sim.simulate(3)

        def ask(s):
            out = list(s.neighbors(bodies=(0, n), radius=0.3)) + list(s.knn(bodies=(0, n), k=6)) + list(s.field(bodies=(0, n)))
            sp = s.split_force(bodies=(0, n), radius=0.3, jerk=True)
            return [np.asarray(x).tobytes() for x in out if x is not None] + [sp[k].tobytes() for k in sorted(sp)]
        got = ask(sim)
        x, v, _ = sim.read()
        twin.init(x, v)
        twin.set_params(e["dt"], e["G"])
        assert got == ask(twin)
        assert x.tobytes() != R.fixture("plummer256")[0].astype(sim.dtype).tobytes()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------
def test_errors_name_the_function_and_the_field():
    b0, v0 = R.fixture("plummer256")
    n = len(b0)

    def fails(code, words, call):
        with pytest.raises(capi.NBodyError) as e:
            call()
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)

    lev = np.zeros(n, np.uint8)
    with Simulation(n) as leap:                                           # a leapfrog handle
        leap.init(b0, v0)
        fails(4, ("nb_set_neighbor_levels", "Hermite"), lambda: leap.set_neighbor_levels(min_level=0))
        fails(4, ("nb_download_neighbor_levels", "Hermite"), lambda: leap.download_neighbor_levels())
        fails(4, ("nb_upload_neighbor_levels", "Hermite"), lambda: leap.upload_neighbor_levels(lev))
        fails(4, ("nb_neighbor_level_stats", "Hermite"), lambda: leap.neighbor_level_stats())
    with hermite(n, "f32") as sim:
        sim.init(b0, v0)
        sim.set_params(R.DT, 1.0)
        assert sim.neighbor_level_stats()["enabled"] == 0
        fails(4, ("nb_set_neighbor_levels", "nb_set_neighbor_scheme"), lambda: sim.set_neighbor_levels(min_level=0))       # no scheme set
        fails(4, ("nb_download_neighbor_levels", "nb_set_neighbor_scheme"), lambda: sim.download_neighbor_levels())
        fails(4, ("nb_upload_neighbor_levels", "nb_set_neighbor_scheme"), lambda: sim.upload_neighbor_levels(lev))
        sim.set_neighbor_scheme(radius=0.1, substeps=8, cap=24)
        fails(4, ("nb_download_neighbor_levels", "nb_set_neighbor_levels"), lambda: sim.download_neighbor_levels())     # levels not set
        fails(4, ("nb_upload_neighbor_levels", "nb_set_neighbor_levels"), lambda: sim.upload_neighbor_levels(lev))
        fails(1, ("nb_set_neighbor_levels", "min_level"), lambda: sim.set_neighbor_levels(min_level=4))                   # > log2(8)
        fails(1, ("nb_set_neighbor_levels", "flags"), lambda: sim.set_neighbor_levels(flags=2))
        fails(1, ("nb_set_neighbor_levels", "reserved"), lambda: sim.set_neighbor_levels(reserved=7))
        fails(1, ("nb_set_neighbor_levels", "eta"), lambda: sim.set_neighbor_levels(eta=-0.5))
        fails(1, ("nb_set_neighbor_levels", "eta"), lambda: sim.set_neighbor_levels(eta=float("nan")))
        assert sim.neighbor_level_stats()["enabled"] == 0                # a refused call changes nothing
        sim.set_neighbor_levels(min_level=1)
        fails(4, ("nb_upload_neighbor_levels", "not current"), lambda: sim.upload_neighbor_levels(np.ones(n, np.uint8)))  # before the scheme is current
        sim.download_neighbor_scheme(24)
        for bad, i in ((0, 5), (4, n - 1), (255, 0)):                     # outside [min_level, L] = [1, 3]
            z = np.ones(n, np.uint8)
            z[i] = bad
            fails(1, ("nb_upload_neighbor_levels", "levels[%d] = %d" % (i, bad)), lambda: sim.upload_neighbor_levels(z))
        sim.upload_neighbor_levels(np.full(n, 3, np.uint8))
        assert (sim.download_neighbor_levels() == 3).all()
        fails(4, ("nb_set_block_steps", "neighbour scheme"), lambda: sim.set_block_steps(max_level=4))      # block steps stay excluded
        sim.simulate(1)


# ---- 9. off again --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["null", "scheme"])
@pytest.mark.parametrize("prec", PRECS)
def test_switching_levels_off_leaves_a_handle_that_never_had_them(prec, how):
    """Levels set and switched off again before a step (NULL, or the scheme set again): every later bit is the twin's."""
    e = R.record()["fixtures"]["plummer256"]
    b0, v0 = R.fixture("plummer256")
    cap = e["cap"]
    scheme = dict(substeps=8, cap=cap, radius=e["radius"])
    with started(prec, b0, v0, e["dt"], 1.0, scheme, None, dict(min_level=1)) as sim, started(prec, b0, v0, e["dt"], 1.0, scheme) as twin:
        assert sim.neighbor_level_stats()["enabled"] == 1
        if how == "null":
            sim.set_neighbor_levels(None)
        else:
            sim.set_neighbor_scheme(**scheme)
        assert sim.neighbor_level_stats()["enabled"] == 0
        sim.simulate(3)
        twin.simulate(3)
        assert state(sim, cap) == state(twin, cap)
        assert sim.neighbor_scheme_stats() == twin.neighbor_scheme_stats()
        # ... and on a handle that has stepped with levels: the scheme's components are left alone, the shared substeps take over
        sim.set_neighbor_levels(min_level=1)
        sim.simulate(1)
        sim.set_neighbor_levels(None)
        x, v, _ = sim.read()
        ck = sim.neighbor_scheme_checkpoint(cap)
        assert "levels" not in ck
        twin.restore_neighbor_scheme(ck, scheme=scheme)
        sim.simulate(2)
        twin.simulate(2)
        assert state(sim, cap) == state(twin, cap)
