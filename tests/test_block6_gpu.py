"""Block individual time steps on order-6 handles (Simulation.set_block_steps6) on the GPU, against the restatement in
tests/block6_ref.py: frozen levels with an exact schedule (active sets below, across and above the 512- and 1,024-row workgroups
and the 256-row tile, several j-chunks), a census of the gathered pass, pinned levels against a shared order-6 handle, dynamic
levels exactly on tiny systems and within counts on 300 bodies with a tight pair, an eccentric Kepler orbit, the bitwise
invariants with the seven-array checkpoint, switching off, the state changes that re-initialise the levels, and the errors.
f64 bounds are the project's; f32 bounds are 8 x the binary32-storing restatement's distance (tests/golden/block6.json)."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_pos_err

from nbody3d_amd import Simulation, capi, ic

import block_ref as B
import block6_ref as R
from block_ref import EPS2, norm_err

pytestmark = pytest.mark.gpu


def hermite6(n, prec, **kw):
    sim = Simulation(n, precision=prec, integrator="hermite4", **kw)
    sim.set_hermite_order(6)
    return sim


def read_state(sim):
    """The handle's state as a hermite6_ref dict."""
    b, v, a = sim.read()
    j = sim.read_jerk()
    s, c = sim.read_snap()
    return {"b": b, "v": v, "a": a[:, :3], "j": j[:, :3], "s": s[:, :3], "c": c[:, :3], "w": (a[:, 3], j[:, 3], s[:, 3], c[:, 3])}


def arrays(sim):
    """The seven arrays of a checkpoint: (b, v, a, j, s, c, levels)."""
    b, v, a = sim.read()
    return (b, v, a, sim.read_jerk()) + tuple(sim.read_snap()) + (sim.read_levels(),)


def bits(sim):
    return tuple(x.tobytes() for x in arrays(sim))


def rel(got, want):
    return abs(got - want) / want


F64_BOUND = {"x": 1e-10, "v": 1e-10, "a": 1e-12, "j": 1e-12, "s": 1e-12, "c": 1e-10}


def check(d, prec, rec, what):
    """d: hermite6_ref.distances by quantity; f64: the project's bounds, f32: 8 x the recorded binary32-storing distance."""
    bound = {q: F64_BOUND[q] if prec == "f64" else R.FACTOR * rec[q] for q in R.QUANTITIES}
    print("%s %s: %s" % (what, prec, "  ".join("%s %.3g (bound %.3g)" % (q, d[q], bound[q]) for q in R.QUANTITIES)))
    bad = {q: (d[q], bound[q]) for q in R.QUANTITIES if not d[q] <= bound[q]}
    assert not bad, bad


def check_carried(sim, st, b0, v0):
    assert st["b"][:, 3].tobytes() == b0[:, 3].astype(sim.dtype).tobytes() and st["v"][:, 3].tobytes() == v0[:, 3].astype(sim.dtype).tobytes()
    assert not any(w.any() for w in st["w"])


# ---- 1. frozen levels: an exact schedule ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.FROZEN_SIZES)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_frozen_levels_follow_the_exact_schedule(prec, n):
    b0, v0, lev, (ref, rl, rs) = R.frozen_ref(n)
    with hermite6(n, prec) as sim:
        sim.init(b0, v0)
        sim.set_params(R.DT_FROZEN, 1.0)
        sim.set_block_steps6(max_level=R.L_FROZEN, frozen=True)
        sim.upload_levels(lev)
        sim.simulate(1)
        st, stats, got_lev = read_state(sim), sim.block_stats(), sim.read_levels()
        assert sim.variant.startswith("hermite6_")
        check_carried(sim, st, b0, v0)
    print("frozen %s N=%d: %s" % (prec, n, stats))
    assert stats["block_steps"] == 8 == rs["block_steps"] and stats["body_steps"] == rs["body_steps"] and stats["outer_steps"] == 1, (stats, rs)
    assert stats["enabled"] == 1 and stats["clamped"] == 0 and stats["finest_level"] == 3, stats
    assert np.array_equal(got_lev, lev) and np.array_equal(rl, lev)
    check(R.distances(st, ref, R.DT_FROZEN, R.L_FROZEN), prec, R.record()["frozen"][str(n)], "frozen N=%d" % n)


# ---- 2. census for the gathered pass -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CENSUS))
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_census_of_the_gathered_pass(prec, name):
    """A body of mass 1e3 at row 256 (the first row of the second tile) and at row n - 1, inside or outside the level-1 set: a tile
    row that is missed or doubled for the gathered rows moves (a1, j1, s1) by orders of magnitude above the bounds."""
    b0, v0, lev, (ref, rl, rs) = R.census_ref(name)
    n = len(b0)
    with hermite6(n, prec) as sim:
        sim.init(b0, v0)
        sim.set_params(R.DT_CENSUS, 1.0)
        sim.set_block_steps6(max_level=1, frozen=True)
        sim.upload_levels(lev)
        sim.simulate(1)
        st, stats = read_state(sim), sim.block_stats()
        check_carried(sim, st, b0, v0)
    assert stats["block_steps"] == 2 == rs["block_steps"] and stats["body_steps"] == rs["body_steps"] == n + int(lev.sum()), (stats, rs)
    check(R.distances(st, ref, R.DT_CENSUS, 1), prec, R.record()["census"][name], "census %s" % name)


# ---- 3. pinned levels equal shared steps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_pinned_levels_equal_shared_steps(prec):
    n = 300
    b0, v0 = ic.plummer(n, seed=21)
    with hermite6(n, prec) as blk, hermite6(n, prec) as plain:
        blk.init(b0, v0)
        blk.set_block_steps6(max_level=2, min_level=2, frozen=prec == "f32")      # (f32: frozen at min_level = pinned)
        blk.simulate(3, 4e-3, 1.0)
        plain.init(b0, v0)
        plain.simulate(12, 1e-3, 1.0)
        b, v, _ = blk.read()
        pb, pv, _ = plain.read()
        st = blk.block_stats()
    ex, ev, er = norm_err(b[:, :3], pb[:, :3]), norm_err(v[:, :3], pv[:, :3]), rel_pos_err(b, pb, 1.0)
    print("pinned level 2 %s N=%d against 12 shared order-6 steps: positions %.3g (rel_pos_err %.3g), velocities %.3g" % (prec, n, ex, er, ev))
    assert st["block_steps"] == 12 and st["body_steps"] == 12 * n and st["finest_level"] == 2, st
    if prec == "f64":
        assert ex <= 1e-10 and ev <= 1e-10, (ex, ev)
    else:
        assert er <= 1e-4, er


# ---- 4. dynamic levels, exactly ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", R.TINY)
def test_dynamic_levels_on_tiny_systems_match_the_restatement_exactly(n, seed):
    b0, v0, (ref, rl, rs), margin = R.tiny_ref(n, seed)
    p = R.TINY_RUN
    print("restatement N=%d: smallest decision margin %.3g, %s, levels %s" % (n, margin, rs, rl.tolist()))
    assert margin >= 5e-4, margin            # no decision near a level boundary: the engine must take the same ones
    with hermite6(n, "f64") as sim:
        sim.init(b0, v0)
        sim.set_block_steps6(eta=p["eta"], max_level=p["max_level"])
        sim.simulate(p["outer"], p["dt"], 1.0)
        st, stats, lev = read_state(sim), sim.block_stats(), sim.read_levels()
    d = R.distances(st, ref, p["dt"], p["max_level"])
    print("engine N=%d: %s, %s" % (n, stats, d))
    assert np.array_equal(lev, rl), (lev, rl)
    for k in ("block_steps", "body_steps", "finest_level", "outer_steps"):
        assert stats[k] == rs[k], (k, stats, rs)
    assert stats["clamped"] == 0
    assert all(d[q] <= 1e-10 for q in R.QUANTITIES), d


# ---- 5. dynamic levels, N = 300 with the tight pair ----------------------------------------------------------------------------
def test_dynamic_levels_on_300_bodies_with_a_tight_pair():
    """The restatement's smallest decision margin is 6.6e-5, so a decision may flip: counts within 2 %, the energy within 10 x the
    restatement's drift, positions within 8 x what noise of 1e-12 on every (a1, j1, s1) moves the restatement by (block6.json)."""
    b0, v0, (ref, rl, rs), rde = R.pair300_ref()
    p, rec = R.PAIR300, R.record()["pair300"]
    with hermite6(p["n"], "f64") as sim:
        sim.init(b0, v0)
        sim.set_params(p["dt"], 1.0)
        sim.set_block_steps6(eta=p["eta"], max_level=p["max_level"])
        k0, p0, _ = sim.diagnostics()
        sim.simulate(p["outer"])
        k1, p1, _ = sim.diagnostics()
        b = sim.read()[0]
        st, lev = sim.block_stats(), sim.read_levels()
    de = abs((k1 + p1 - k0 - p0) / (k0 + p0))
    ex, bound = norm_err(b[:, :3], ref["b"][:, :3]), R.FACTOR * rec["noise_position_dev"]
    print("N=300 tight pair: positions %.3g (bound %.3g), |dE/E| %.3g (restatement %.3g), %s (restatement %s), levels %s"
          % (ex, bound, de, rde, st, rs, np.bincount(lev).tolist()))
    assert rs["block_steps"] == rec["stats"]["block_steps"] and rs["body_steps"] == rec["stats"]["body_steps"]
    assert rel(st["body_steps"], rs["body_steps"]) <= 0.02 and rel(st["block_steps"], rs["block_steps"]) <= 0.02, (st, rs)
    assert st["clamped"] == 0
    assert de <= 10 * rde, (de, rde)
    assert ex <= bound, (ex, bound)


# ---- 6. Kepler e = 0.9 ---------------------------------------------------------------------------------------------------------
def test_kepler_orbit_on_the_engine():
    b0, v0, (ref, rl, rs), rde = R.kepler6_ref()
    k = B.KEPLER
    e0 = B.energy(b0, v0, 1.0, k["eps2"])
    with hermite6(2, "f64", eps2=k["eps2"]) as sim:
        sim.init(b0, v0)
        sim.set_block_steps6(eta=k["eta"], max_level=k["max_level"])
        sim.simulate(k["outer"], k["dt"], k["G"])
        b, v, _ = sim.read()
        st = sim.block_stats()
        de = abs((B.energy(b, v, 1.0, k["eps2"]) - e0) / e0)
        print("Kepler e=0.9 order 6: |dE/E| %.3g (restatement %.3g), %s (restatement %s)" % (de, rde, st, rs))
        assert de <= 2 * rde, (de, rde)
        assert rel(st["body_steps"], rs["body_steps"]) <= 0.05, (st, rs)
        assert st["clamped"] == 0
        # the same orbit with too few levels: decisions are clamped and reported
        sim.init(b0, v0)
        sim.set_block_steps6(eta=k["eta"], max_level=6)
        sim.block_stats(reset=True)
        sim.simulate(k["outer"])
        st = sim.block_stats()
        print("  max_level 6: %s" % st)
        assert st["clamped"] > 0 and st["finest_level"] == 6, st


# ---- 7. bitwise invariants -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bitwise_invariants(prec):
    n, dt = 1025, 2.0 ** -5
    b0, v0 = B.tight_pair(*ic.plummer(n, seed=21))
    blk = dict(eta=0.02, max_level=10) if prec == "f64" else dict(max_level=R.L_FROZEN, frozen=True)
    lev0 = None if prec == "f64" else R.frozen_levels(n)

    def begin(s, b, v):
        s.init(b, v)
        s.set_params(dt, 1.0)
        s.set_block_steps6(**blk)
        if lev0 is not None:
            s.upload_levels(lev0)

    with hermite6(n, prec) as one, hermite6(n, prec) as two:
        begin(one, b0, v0)
        begin(two, b0, v0)
        one.simulate(3)
        for k in range(3):
            two.step()
            if k < 2:       # read-only calls between steps change no bit
                two.field(np.zeros((5, 4), two.dtype))
                two.neighbors(np.zeros((5, 4), two.dtype), radius=0.5)
                two.diagnostics()
                two.block_stats()
                two.read_levels()
        assert bits(one) == bits(two)                          # nb_step(3) == 3 x nb_step(1); two handles, same bits
        s1, s2 = one.block_stats(), two.block_stats()
        assert s1 == s2 and s1["outer_steps"] == 3 and s1["body_steps"] > 3 * n and s1["finest_level"] > 0, (s1, s2)
        before = bits(one)
        assert one.force_pass(2) > 0.0                         # the full N x N order-6 pass into scratch
        assert bits(one) == before
        one.simulate(3, 0.0)                                   # dt = 0: a no-op on the state
        assert bits(one)[:6] == before[:6]
        assert one.block_stats() == s1
        # checkpoint: the seven arrays after 2 outer steps (c != 0); a fresh handle continues with the same bits
        begin(one, b0, v0)
        one.simulate(2)
        cb, cv, ca, cj, cs, cc, cl = arrays(one)
        assert cc[:, :3].any()
        one.simulate(2)
        with hermite6(n, prec) as fresh:
            fresh.init(cb, cv)
            fresh.set_params(dt, 1.0)
            fresh.upload_derivs6(ca, cj, cs, cc)
            fresh.set_block_steps6(**blk)
            assert tuple(x.tobytes() for x in arrays(fresh)[:6]) == tuple(x.tobytes() for x in (cb, cv, ca, cj, cs, cc))      # the setter left all six
            fresh.upload_levels(cl)
            fresh.simulate(2)
            assert bits(fresh) == bits(one)


# ---- 8. switching off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", ["set_block_steps6", "set_block_steps"])
def test_switching_off_steps_as_a_plain_order6_handle(off):
    n, dt = 300, 2.0 ** -7
    b0, v0 = B.tight_pair(*ic.plummer(n, seed=21))
    with hermite6(n, "f64") as sim, hermite6(n, "f64") as plain:
        sim.init(b0, v0)
        sim.set_block_steps6(eta=0.02, max_level=8)
        sim.simulate(2, dt, 1.0)
        cb, cv, ca, cj, cs, cc, _ = arrays(sim)
        getattr(sim, off)(None)
        assert sim.block_stats()["enabled"] == 0 and sim.hermite_order() == 6
        sim.simulate(3)
        plain.init(cb, cv)
        plain.upload_derivs6(ca, cj, cs, cc)
        plain.simulate(3, dt, 1.0)
        assert tuple(x.tobytes() for x in sim.read()) == tuple(x.tobytes() for x in plain.read())
        assert sim.read_jerk().tobytes() == plain.read_jerk().tobytes()
        assert tuple(x.tobytes() for x in sim.read_snap()) == tuple(x.tobytes() for x in plain.read_snap())
        with pytest.raises(capi.NBodyError) as e:          # no levels without block steps
            sim.read_levels()
        assert e.value.code == 4


# ---- 9. re-initialisation ------------------------------------------------------------------------------------------------------
def start_rule(a, j, dt, eta, L):
    margins, stats = [], {"clamped": 0}
    lev = B.start_levels(a[:, :3], j[:, :3], dt, eta, 0, L, stats, margins)
    assert min(margins) >= 1e-3, min(margins)              # the system was chosen so: no start decision near a level boundary
    return lev.astype(np.uint8)


def test_a_change_of_dt_or_G_and_a_new_upload_reinitialise_the_levels():
    n = 12
    b0, v0 = B.tight_pair(*ic.plummer(n, seed=3))
    with hermite6(n, "f64") as sim:
        sim.init(b0, v0)
        sim.set_block_steps6(eta=0.02, max_level=12)
        sim.simulate(1, 2.0 ** -3, 1.0)
        before = sim.read_levels()
        a, j = sim.read()[2], sim.read_jerk()
        s, c = sim.read_snap()
        sim.set_params(2.0 ** -5, 1.0)                     # a change of dt: the start rule on the derivatives as they stand
        lev = sim.read_levels()
        want = start_rule(a, j, 2.0 ** -5, 0.02, 12)
        print("levels before %s, after the change of dt %s, start rule %s" % (before.tolist(), lev.tolist(), want.tolist()))
        assert np.array_equal(lev, want)
        assert sim.read()[2].tobytes() == a.tobytes() and sim.read_snap()[1].tobytes() == c.tobytes()      # the derivatives were kept
        sim.set_params(2.0 ** -5, 1.0)                     # the same dt again: nothing goes stale
        sim.simulate(1)
        sim.set_params(2.0 ** -5, 2.0)                     # a change of G: derivatives and levels start again (c = 0)
        lev = sim.read_levels()
        a2, j2 = sim.read()[2], sim.read_jerk()
        assert not sim.read_snap()[1].any()
        assert np.array_equal(lev, start_rule(a2, j2, 2.0 ** -5, 0.02, 12))
        sim.init(b0, v0)                                   # a new upload without upload_levels
        sim.set_params(2.0 ** -5, 1.0)
        a0, j0 = B.fj_ref(b0, v0, 1.0, EPS2)
        assert np.array_equal(sim.read_levels(), start_rule(a0, j0, 2.0 ** -5, 0.02, 12))
        # frozen with stale levels: every body at min_level
        sim.set_block_steps6(max_level=5, min_level=2, frozen=True)
        assert (sim.read_levels() == 2).all()


# ---- 10. errors ----------------------------------------------------------------------------------------------------------------
def test_errors():
    n = 64
    b0, v0 = ic.plummer(n, seed=2)
    L = capi.load_library()
    assert L.nb_set_block_steps6(None, None) == 1
    with Simulation(n) as lf:                              # a leapfrog handle
        lf.init(b0, v0)
        lf.set_params(1e-3, 1.0)
        for call in (lambda: lf.set_block_steps6(), lambda: lf.set_block_steps6(None)):
            with pytest.raises(capi.NBodyError) as e:
                call()
            assert e.value.code == 4 and "nb_set_block_steps6" in str(e.value) and "nb_set_hermite_order" in str(e.value), str(e.value)
    with Simulation(n, precision="f64", integrator="hermite4") as h4:      # an order-4 handle
        h4.init(b0, v0)
        h4.set_params(1e-3, 1.0)
        with pytest.raises(capi.NBodyError) as e:
            h4.set_block_steps6()
        assert e.value.code == 4 and "nb_set_block_steps6" in str(e.value) and "nb_set_hermite_order" in str(e.value), str(e.value)
        h4.set_block_steps()                               # pinned: order 6 while block steps are on
        with pytest.raises(capi.NBodyError) as e:
            h4.set_hermite_order(6)
        assert e.value.code == 4 and "nb_set_hermite_order" in str(e.value)
    with hermite6(n, "f32") as sim:
        sim.init(b0, v0)
        sim.set_params(1e-3, 1.0)
        with pytest.raises(capi.NBodyError) as e:          # binary32 storage cannot carry the criterion
            sim.set_block_steps6()
        assert e.value.code == 4 and "nb_set_block_steps6" in str(e.value) and "NB_F32" in str(e.value) and "a4" in str(e.value), str(e.value)
        assert sim.block_stats()["enabled"] == 0
        sim.set_block_steps6(max_level=4, frozen=True)     # frozen levels work
        sim.simulate(1)
        assert sim.block_stats()["block_steps"] == 1
        sim.set_block_steps6(None)
    with hermite6(n, "f64") as sim:
        sim.init(b0, v0)
        sim.set_params(1e-3, 1.0)
        with pytest.raises(capi.NBodyError) as e:          # pinned: the order-4 entry point on an order-6 handle
            sim.set_block_steps()
        assert e.value.code == 4 and "nb_set_block_steps" in str(e.value) and "nb_set_hermite_order" in str(e.value), str(e.value)
        for kw, field in ((dict(max_level=31), "max_level"), (dict(max_level=3, min_level=4), "min_level"), (dict(eta=-1.0), "eta"),
                          (dict(eta=float("nan")), "eta")):
            with pytest.raises(capi.NBodyError) as e:
                sim.set_block_steps6(**kw)
            assert e.value.code == 1 and "nb_set_block_steps6" in str(e.value) and field in str(e.value), str(e.value)
        cfg = capi.nb_block_steps()
        cfg.struct_size = C.sizeof(cfg)
        cfg.flags = 2
        assert L.nb_set_block_steps6(sim._h, C.byref(cfg)) == 1 and b"flags" in L.nb_last_error(sim._h)
        cfg.flags = 0
        cfg.struct_size = C.sizeof(cfg) - 8
        assert L.nb_set_block_steps6(sim._h, C.byref(cfg)) == 1 and b"struct_size" in L.nb_last_error(sim._h)
        assert sim.block_stats()["enabled"] == 0           # none of the rejected calls switched anything on
        sim.set_block_steps6(max_level=4, min_level=1)
        with pytest.raises(capi.NBodyError) as e:
            sim.set_hermite_order(4)
        assert e.value.code == 4 and "nb_set_hermite_order" in str(e.value) and "nb_set_block_steps6" in str(e.value), str(e.value)
        with pytest.raises(capi.NBodyError) as e:
            sim.set_neighbor_scheme(radius=0.1)
        assert e.value.code == 4 and "nb_set_neighbor_scheme" in str(e.value), str(e.value)
        lev = np.full(n, 2, np.uint8)
        lev[n - 1] = 5
        with pytest.raises(capi.NBodyError) as e:
            sim.upload_levels(lev)
        assert e.value.code == 1 and "nb_upload_levels" in str(e.value)
        sim.upload_levels(np.full(n, 2, np.uint8))
        sim.simulate(2)
        st = sim.block_stats(reset=True)
        assert st["outer_steps"] == 2 and st["block_steps"] >= 2 and st["body_steps"] >= 2 * n, st


def test_timing_reports_one_outer_step_per_launch():
    n = 1025
    b0, v0 = B.tight_pair(*ic.plummer(n, seed=21))
    with hermite6(n, "f64") as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -6, 1.0)
        sim.set_block_steps6(max_level=8)
        sim.enable_timing(True)
        sim.simulate(3)
        t = sim.step_breakdown()
    assert t["launches"] == 3 and t["force_ms"] > 0 and t["integrate_ms"] == 0 and t["span_ms"] == t["force_ms"], t
