"""Block individual time steps (Simulation.set_block_steps) on the GPU, against the fp64 restatement in tests/block_ref.py: frozen
levels with an exact schedule (every kernel path: active sets below, across and above the 512- and 1,024-row workgroups and the
256-row tile, several j-chunks), pinned levels against a shared-step handle, dynamic levels EXACTLY only on tiny systems (N = 6
and 12: one wave of the scheduler, one workgroup of everything else), a 300-body sphere with a tight pair held to step counts
within 2 % / 5 % and an energy bound, an eccentric Kepler orbit, the bitwise invariants (two handles against each other: a fault
both share passes), the state changes that re-initialise the levels, and the errors.  Dynamic levels at sizes where the scheduler
runs several waves and the active sets span many workgroups -- every level, every count, every decision in both precisions -- are
held in test_block_decisions_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_pos_err

from nbody3d_amd import Simulation, capi, ic

import block_ref as R
from block_ref import EPS2, norm_err

pytestmark = pytest.mark.gpu


def hermite(n, prec, **kw):
    return Simulation(n, precision=prec, integrator="hermite4", **kw)


def state(sim):
    return tuple(x.tobytes() for x in sim.read()) + (sim.read_jerk().tobytes(), sim.read_levels().tobytes())


def rel(got, want):
    return abs(got - want) / want


# ---- 1. frozen levels: an exact schedule ---------------------------------------------------------------------------------------
_frozen = {}


def frozen_levels(n):
    """Bodies 1 + 2k, k < 513, at level 2; 40 % of the rest at level 1; the others at level 0; then body min(5, n - 1) at level 3
    (body 5 where there is one), so that every size runs the 8 block steps of max_level 3."""
    lev = np.zeros(n, np.uint8)
    two = np.array([1 + 2 * k for k in range(513) if 1 + 2 * k < n], np.int64)
    lev[two] = 2
    rest = np.setdiff1d(np.arange(n), two)
    rng = np.random.default_rng(7)
    lev[rest[rng.random(len(rest)) < 0.4]] = 1
    lev[min(5, n - 1)] = 3
    return lev


def frozen_ref(n):
    """(b0, v0, levels, restatement result): computed once per size, shared by both precisions, never written."""
    if n not in _frozen:
        b0, v0 = ic.plummer(n, seed=21)
        lev = frozen_levels(n)
        _frozen[n] = (b0, v0, lev, R.block_ref(b0, v0, 1.0, EPS2, 2.0 ** -4, 1, max_level=3, levels=lev, frozen=True))
    return _frozen[n]


@pytest.mark.parametrize("n", [2, 77, 1025, 4099])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_frozen_levels_follow_the_exact_schedule(prec, n):
    b0, v0, lev, (rb, rv, ra, rj, rl, rs) = frozen_ref(n)
    with hermite(n, prec) as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -4, 1.0)
        sim.set_block_steps(max_level=3, frozen=True)
        sim.upload_levels(lev)
        sim.simulate(1)
        b, v, a = sim.read()
        j = sim.read_jerk()
        st = sim.block_stats()
        got_lev = sim.read_levels()
    ea, ej = norm_err(a[:, :3], ra), norm_err(j[:, :3], rj)
    ex, ev, er = norm_err(b[:, :3], rb[:, :3]), norm_err(v[:, :3], rv[:, :3]), rel_pos_err(b, rb, 1.0)
    print("frozen %s N=%d: positions %.3g (rel_pos_err %.3g), velocities %.3g, a %.3g, j %.3g; %s" % (prec, n, ex, er, ev, ea, ej, st))
    assert st["block_steps"] == 8 == rs["block_steps"] and st["body_steps"] == rs["body_steps"] and st["outer_steps"] == 1, (st, rs)
    assert st["enabled"] == 1 and st["clamped"] == 0 and st["finest_level"] == 3, st
    assert np.array_equal(got_lev, lev) and np.array_equal(rl, lev)
    if prec == "f64":
        assert ex <= 1e-10 and ev <= 1e-10 and ea <= 1e-12 and ej <= 1e-12, (ex, ev, ea, ej)
    else:
        assert er <= 1e-4 and ea <= 2e-5 and ej <= 2e-5, (er, ea, ej)
    assert b[:, 3].tobytes() == b0[:, 3].astype(sim.dtype).tobytes() and v[:, 3].tobytes() == v0[:, 3].astype(sim.dtype).tobytes()
    assert not a[:, 3].any() and not j[:, 3].any()


# ---- 2. pinned levels equal shared steps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_pinned_levels_equal_shared_steps(prec):
    n = 300
    b0, v0 = ic.plummer(n, seed=21)
    with hermite(n, prec) as blk, hermite(n, prec) as plain:
        blk.init(b0, v0)
        blk.set_block_steps(max_level=2, min_level=2)
        blk.simulate(3, 4e-3, 1.0)
        plain.init(b0, v0)
        plain.simulate(12, 1e-3, 1.0)
        b, v, _ = blk.read()
        pb, pv, _ = plain.read()
        st = blk.block_stats()
    ex, ev, er = norm_err(b[:, :3], pb[:, :3]), norm_err(v[:, :3], pv[:, :3]), rel_pos_err(b, pb, 1.0)
    print("pinned level 2 %s N=%d against 12 shared steps: positions %.3g (rel_pos_err %.3g), velocities %.3g" % (prec, n, ex, er, ev))
    assert st["block_steps"] == 12 and st["body_steps"] == 12 * n and st["finest_level"] == 2, st
    if prec == "f64":
        assert ex <= 1e-10 and ev <= 1e-10, (ex, ev)
    else:
        assert er <= 1e-4, er


# ---- 3. dynamic levels, tiny systems -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(6, 9), (12, 3)])
def test_dynamic_levels_on_tiny_systems_match_the_restatement_exactly(n, seed):
    b0, v0 = R.tight_pair(*ic.plummer(n, seed=seed))
    margins = []
    rb, rv, ra, rj, rl, rs = R.block_ref(b0, v0, 1.0, EPS2, 2.0 ** -3, 2, eta=0.02, max_level=12, margins=margins)
    print("restatement N=%d: smallest decision margin %.3g, %s, levels %s" % (n, min(margins), rs, rl.tolist()))
    assert min(margins) >= 1e-3, min(margins)            # no decision near a level boundary: the engine must take the same ones
    with hermite(n, "f64") as sim:
        sim.init(b0, v0)
        sim.set_block_steps(eta=0.02, max_level=12)
        sim.simulate(2, 2.0 ** -3, 1.0)
        b, v, a = sim.read()
        j = sim.read_jerk()
        st, lev = sim.block_stats(), sim.read_levels()
    ex, ev = norm_err(b[:, :3], rb[:, :3]), norm_err(v[:, :3], rv[:, :3])
    print("engine N=%d: %s, positions %.3g, velocities %.3g, a %.3g, j %.3g" % (n, st, ex, ev, norm_err(a[:, :3], ra), norm_err(j[:, :3], rj)))
    assert np.array_equal(lev, rl), (lev, rl)
    for k in ("block_steps", "body_steps", "finest_level", "outer_steps"):
        assert st[k] == rs[k], (k, st, rs)
    assert st["clamped"] == 0
    assert ex <= 1e-10 and ev <= 1e-10 and norm_err(a[:, :3], ra) <= 1e-10 and norm_err(j[:, :3], rj) <= 1e-10


# ---- 4. dynamic levels, N = 300 with the tight pair ----------------------------------------------------------------------------
_pair300 = {}


def pair300_ref():
    if not _pair300:
        b0, v0 = R.tight_pair(*ic.plummer(300, seed=21))
        out = R.block_ref(b0, v0, 1.0, EPS2, 2.0 ** -4, 2, eta=0.02, max_level=12)
        e0, e1 = R.energy(b0, v0, 1.0, EPS2), R.energy(out[0], out[1], 1.0, EPS2)
        _pair300["x"] = (b0, v0, out, abs((e1 - e0) / e0))
    return _pair300["x"]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_dynamic_levels_on_300_bodies_with_a_tight_pair(prec):
    """The restatement's smallest decision margin is 7e-5, so a decision may flip: positions to 1e-8 (f64; the restatement differs
    from a pinned level-8 run by 7.3e-9, which bounds what a flipped level moves a body; a wrong h, a stale prediction or a wrong
    corrector shows at >= 1e-6), the counts to 2 % (f64) / 5 % (f32)."""
    b0, v0, (rb, rv, ra, rj, rl, rs), rde = pair300_ref()
    with hermite(300, prec) as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -4, 1.0)
        sim.set_block_steps(eta=0.02, max_level=12)
        k0, p0, _ = sim.diagnostics()
        sim.simulate(2)
        k1, p1, _ = sim.diagnostics()
        b = sim.read()[0]
        st, lev = sim.block_stats(), sim.read_levels()
    de = abs((k1 + p1 - k0 - p0) / (k0 + p0))
    ex, er = norm_err(b[:, :3], rb[:, :3]), rel_pos_err(b, rb, 1.0)
    print("N=300 tight pair %s: positions %.3g (rel_pos_err %.3g), |dE/E| %.3g (restatement %.3g), %s (restatement %s), levels %s"
          % (prec, ex, er, de, rde, st, rs, np.bincount(lev).tolist()))
    assert rs["block_steps"] == 189 and rs["body_steps"] == 5104
    if prec == "f64":
        assert ex <= 1e-8, ex
        assert rel(st["body_steps"], rs["body_steps"]) <= 0.02 and rel(st["block_steps"], rs["block_steps"]) <= 0.02, (st, rs)
    else:
        assert er <= 1e-4, er
        assert rel(st["body_steps"], rs["body_steps"]) <= 0.05, (st, rs)
    assert de <= 10 * rde, (de, rde)
    assert st["clamped"] == 0


# ---- 5. Kepler e = 0.9 ---------------------------------------------------------------------------------------------------------
def test_kepler_orbit_on_the_engine():
    b0, v0, (rb, rv, ra, rj, rl, rs), rde = R.kepler_ref()
    k = R.KEPLER
    e0 = R.energy(b0, v0, 1.0, k["eps2"])
    with hermite(2, "f64", eps2=k["eps2"]) as sim:
        sim.init(b0, v0)
        sim.set_block_steps(eta=k["eta"], max_level=k["max_level"])
        sim.simulate(k["outer"], k["dt"], k["G"])
        b, v, _ = sim.read()
        st = sim.block_stats()
        de = abs((R.energy(b, v, 1.0, k["eps2"]) - e0) / e0)
        print("Kepler e=0.9 engine: |dE/E| %.3g (restatement %.3g), %s (restatement %s)" % (de, rde, st, rs))
        assert de <= 2 * rde, (de, rde)
        assert rel(st["body_steps"], rs["body_steps"]) <= 0.05, (st, rs)
        assert st["clamped"] == 0
        # the same orbit with too few levels: decisions are clamped and reported
        sim.init(b0, v0)
        sim.set_block_steps(eta=k["eta"], max_level=6)
        sim.block_stats(reset=True)
        sim.simulate(k["outer"])
        st = sim.block_stats()
        print("  max_level 6: %s" % st)
        assert st["clamped"] > 0 and st["finest_level"] == 6, st


# ---- 6. bitwise invariants -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bitwise_invariants(prec):
    n, dt = 1025, 2.0 ** -5
    b0, v0 = R.tight_pair(*ic.plummer(n, seed=21))
    blk = dict(eta=0.02, max_level=10)
    with hermite(n, prec) as one, hermite(n, prec) as two:
        for s in (one, two):
            s.init(b0, v0)
            s.set_params(dt, 1.0)
            s.set_block_steps(**blk)
        one.simulate(3)
        for k in range(3):
            two.step()
            if k < 2:       # read-only calls between steps change no bit
                two.field(np.zeros((5, 4), two.dtype))
                two.diagnostics()
                two.request_frame()
                two.block_stats()
                two.read_levels()
        assert state(one) == state(two)                        # nb_step(3) == 3 x nb_step(1); two handles, same bits
        s1, s2 = one.block_stats(), two.block_stats()
        assert s1 == s2 and s1["outer_steps"] == 3 and s1["body_steps"] > 3 * n and s1["finest_level"] > 0, (s1, s2)
        before = state(one)
        assert one.force_pass(2) > 0.0                         # the full N x N pass into scratch
        assert state(one) == before
        one.simulate(3, 0.0)                                   # dt = 0: a no-op on the state
        assert state(one)[:4] == before[:4]
        assert one.block_stats() == s1
        # checkpoint: (b, v, a, j, levels) after 2 outer steps; a fresh handle continues with the same bits
        one.init(b0, v0)
        one.simulate(2, dt, 1.0)
        cb, cv, ca = one.read()
        cj, cl = one.read_jerk(), one.read_levels()
        one.simulate(2)
        with hermite(n, prec) as fresh:
            fresh.init(cb, cv)
            fresh.upload_derivs(ca, cj)
            fresh.set_block_steps(**blk)
            fresh.upload_levels(cl)
            fresh.simulate(2, dt, 1.0)
            assert state(fresh) == state(one)


# ---- 7. state changes ----------------------------------------------------------------------------------------------------------
def test_switching_off_steps_as_a_plain_hermite_handle():
    n, dt = 300, 2.0 ** -7
    b0, v0 = R.tight_pair(*ic.plummer(n, seed=21))
    with hermite(n, "f64") as sim, hermite(n, "f64") as plain:
        sim.init(b0, v0)
        sim.set_block_steps(eta=0.02, max_level=8)
        sim.simulate(2, dt, 1.0)
        cb, cv, ca = sim.read()
        cj = sim.read_jerk()
        sim.set_block_steps(None)
        assert sim.block_stats()["enabled"] == 0
        sim.simulate(3)
        plain.init(cb, cv)
        plain.upload_derivs(ca, cj)
        plain.simulate(3, dt, 1.0)
        assert tuple(x.tobytes() for x in sim.read()) == tuple(x.tobytes() for x in plain.read())
        assert sim.read_jerk().tobytes() == plain.read_jerk().tobytes()
        with pytest.raises(capi.NBodyError) as e:          # no levels without block steps
            sim.read_levels()
        assert e.value.code == 4


def start_rule(a, j, dt, eta, L):
    margins, stats = [], {"clamped": 0}
    lev = R.start_levels(a[:, :3], j[:, :3], dt, eta, 0, L, stats, margins)
    assert min(margins) >= 1e-3, min(margins)              # the system was chosen so: no start decision near a level boundary
    return lev.astype(np.uint8)


def test_a_change_of_dt_and_a_new_upload_reinitialise_the_levels():
    n = 12
    b0, v0 = R.tight_pair(*ic.plummer(n, seed=3))
    with hermite(n, "f64") as sim:
        sim.init(b0, v0)
        sim.set_block_steps(eta=0.02, max_level=12)
        sim.simulate(1, 2.0 ** -3, 1.0)
        before = sim.read_levels()
        a, j = sim.read()[2], sim.read_jerk()
        sim.set_params(2.0 ** -5, 1.0)                     # a change of dt: the start rule on the derivatives as they stand
        lev = sim.read_levels()
        want = start_rule(a, j, 2.0 ** -5, 0.02, 12)
        print("levels before %s, after the change of dt %s, start rule %s" % (before.tolist(), lev.tolist(), want.tolist()))
        assert np.array_equal(lev, want)
        assert sim.read()[2].tobytes() == a.tobytes()      # the derivatives were kept
        sim.set_params(2.0 ** -5, 1.0)                     # the same dt again: nothing goes stale
        sim.simulate(1)
        sim.init(b0, v0)                                   # a new upload without upload_levels
        a0, j0 = R.fj_ref(b0, v0, 1.0, EPS2)
        assert np.array_equal(sim.read_levels(), start_rule(a0, j0, 2.0 ** -5, 0.02, 12))
        # frozen with stale levels: every body at min_level
        sim.set_block_steps(max_level=5, min_level=2, frozen=True)
        assert (sim.read_levels() == 2).all()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------
def test_errors():
    n = 64
    b0, v0 = ic.plummer(n, seed=2)
    L = capi.load_library()
    with Simulation(n) as lf:
        lf.init(b0, v0)
        lf.set_params(1e-3, 1.0)
        for call in (lambda: lf.set_block_steps(), lambda: lf.set_block_steps(None), lambda: lf.block_stats(), lambda: lf.read_levels(),
                     lambda: lf.upload_levels(np.zeros(n, np.uint8))):
            with pytest.raises(capi.NBodyError) as e:
                call()
            assert e.value.code == 4, str(e.value)
    with hermite(n, "f32") as sim:
        sim.set_block_steps()
        with pytest.raises(capi.NBodyError) as e:          # before init
            sim.upload_levels(np.zeros(n, np.uint8))
        assert e.value.code == 4 and "nb_upload_levels" in str(e.value)
        sim.set_block_steps(None)
        sim.init(b0, v0)
        sim.set_params(1e-3, 1.0)
        for kw, field in ((dict(max_level=31), "max_level"), (dict(max_level=3, min_level=4), "min_level"), (dict(eta=-1.0), "eta"),
                          (dict(eta=float("nan")), "eta")):
            with pytest.raises(capi.NBodyError) as e:
                sim.set_block_steps(**kw)
            assert e.value.code == 1 and "nb_set_block_steps" in str(e.value) and field in str(e.value), str(e.value)
        cfg = capi.nb_block_steps()
        cfg.struct_size = C.sizeof(cfg)
        cfg.flags = 2
        assert L.nb_set_block_steps(sim._h, C.byref(cfg)) == 1 and b"flags" in L.nb_last_error(sim._h)
        cfg.flags = 0
        cfg.struct_size = C.sizeof(cfg) - 8
        assert L.nb_set_block_steps(sim._h, C.byref(cfg)) == 1 and b"struct_size" in L.nb_last_error(sim._h)
        st = capi.nb_block_stats()
        st.struct_size = 8
        assert L.nb_block_stats(sim._h, C.byref(st), 0) == 1 and b"struct_size" in L.nb_last_error(sim._h)
        assert sim.block_stats()["enabled"] == 0           # none of the rejected calls switched anything on
        sim.set_block_steps(max_level=4, min_level=1)
        for bad in (5, 0):
            lev = np.full(n, 2, np.uint8)
            lev[n - 1] = bad
            with pytest.raises(capi.NBodyError) as e:
                sim.upload_levels(lev)
            assert e.value.code == 1 and "nb_upload_levels" in str(e.value) and "levels" in str(e.value)
        sim.upload_levels(np.full(n, 2, np.uint8))
        sim.simulate(2)
        st = sim.block_stats(reset=True)
        assert st["outer_steps"] == 2 and st["block_steps"] >= 2 and st["body_steps"] >= 2 * n, st
        st = sim.block_stats()
        assert st["enabled"] == 1 and all(st[k] == 0 for k in ("outer_steps", "block_steps", "body_steps", "clamped", "finest_level")), st


def test_timing_reports_one_outer_step_per_launch():
    n = 1025
    b0, v0 = R.tight_pair(*ic.plummer(n, seed=21))
    with hermite(n, "f32") as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -6, 1.0)
        sim.set_block_steps(max_level=8)
        sim.enable_timing(True)
        sim.simulate(3)
        t = sim.step_breakdown()
    assert t["launches"] == 3 and t["force_ms"] > 0 and t["integrate_ms"] == 0 and t["span_ms"] == t["force_ms"], t
