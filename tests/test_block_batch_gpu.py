"""Batched block steps (Simulation.set_block_batch) on the GPU: block steps with a small active set run from the device's own
header, many per host wait.  Frozen levels with an exact schedule and the exact split into small and host steps, dynamic levels
against the fp64 restatement (every level and every count equal: tests/block_ref.py, tests/golden/block_decisions.*), the bitwise
invariants (depth, where batches end, two handles, a checkpoint), small_max = 0 against a handle with the mode off, a row's bits
against |A| and its place in the active list, the counters with a bound on the host's policy, and the errors."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_pos_err

from nbody3d_amd import Simulation, capi, ic

import block_ref as R
from block_ref import EPS2, norm_err

pytestmark = pytest.mark.gpu

X_TOL = V_TOL = 1e-10                # the project's fp64 bounds on norm_err after block steps (test_block_decisions_gpu.py)
A_TOL = J_TOL = 1e-12
COUNTS = ("block_steps", "body_steps", "finest_level", "outer_steps", "clamped")


def hermite(n, prec, **kw):
    return Simulation(n, precision=prec, integrator="hermite4", **kw)


def state(sim):
    return tuple(x.tobytes() for x in sim.read()) + (sim.read_jerk().tobytes(), sim.read_levels().tobytes())


def identities(sim):
    """The identities of the batch counters against each other and against nb_block_stats (both since the same reset)."""
    bs, st = sim.block_batch_stats(), sim.block_stats()
    assert bs["small_steps"] + bs["host_steps"] == st["block_steps"], (bs, st)
    assert bs["slots"] == bs["small_steps"] + bs["host_steps"] + bs["idle_slots"], bs
    assert bs["host_steps"] <= bs["host_waits"] <= bs["slots"], bs
    return bs, st


# ---- 1. frozen levels: an exact schedule, and which path every block step took -------------------------------------------------
_frozen = {}


def frozen_levels(n):
    """test_block_gpu.frozen_levels, restated: bodies 1 + 2k, k < 513, at level 2; 40 % of the rest at level 1; the others at level
    0; then body min(5, n - 1) at level 3."""
    lev = np.zeros(n, np.uint8)
    two = np.array([1 + 2 * k for k in range(513) if 1 + 2 * k < n], np.int64)
    lev[two] = 2
    rest = np.setdiff1d(np.arange(n), two)
    rng = np.random.default_rng(7)
    lev[rest[rng.random(len(rest)) < 0.4]] = 1
    lev[min(5, n - 1)] = 3
    return lev


def frozen_ref(n):
    """(b0, v0, levels, restatement result): computed once per size, shared by every case, never written."""
    if n not in _frozen:
        b0, v0 = ic.plummer(n, seed=21)
        lev = frozen_levels(n)
        _frozen[n] = (b0, v0, lev, R.block_ref(b0, v0, 1.0, EPS2, 2.0 ** -4, 1, max_level=3, levels=lev, frozen=True))
    return _frozen[n]


def active_at(lev, L, t):
    """|A(t)| of frozen levels: the bodies whose step 2^(L - l) divides t."""
    return int(((t % (1 << (L - lev.astype(np.int64)))) == 0).sum())


@pytest.mark.parametrize("small_max", [64, 1024])
@pytest.mark.parametrize("n", [2, 77, 1025, 4099])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_frozen_levels_follow_the_exact_schedule(prec, n, small_max):
    b0, v0, lev, (rb, rv, ra, rj, rl, rs) = frozen_ref(n)
    sizes = {t: active_at(lev, 3, t) for t in range(1, 9)}
    assert all(sizes[t] == 1 for t in (1, 3, 5, 7)) and sizes[8] == n
    assert sizes[2] == sizes[6] and (sizes[2] == 1 if n == 2 else sizes[2] == 38 if n == 77 else 64 < sizes[2] <= 1024), sizes
    small = [t for t in range(1, 8) if sizes[t] <= small_max]      # tick 8 is a host step even where small_max > n
    assert set(small) >= {1, 3, 5, 7} and ((2 in small and 6 in small) == (n < 1025 or small_max == 1024))
    with hermite(n, prec) as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -4, 1.0)
        sim.set_block_steps(max_level=3, frozen=True)
        sim.set_block_batch(depth=8, small_max=small_max)
        sim.upload_levels(lev)
        sim.simulate(1)
        b, v, a = sim.read()
        j = sim.read_jerk()
        bs, st = identities(sim)
        got_lev = sim.read_levels()
    ea, ej = norm_err(a[:, :3], ra), norm_err(j[:, :3], rj)
    ex, ev, er = norm_err(b[:, :3], rb[:, :3]), norm_err(v[:, :3], rv[:, :3]), rel_pos_err(b, rb, 1.0)
    print("frozen %s N=%d small_max %d: positions %.3g (rel_pos_err %.3g), velocities %.3g, a %.3g, j %.3g; %s %s"
          % (prec, n, small_max, ex, er, ev, ea, ej, st, bs))
    assert st["block_steps"] == 8 == rs["block_steps"] and st["body_steps"] == rs["body_steps"] and st["outer_steps"] == 1, (st, rs)
    assert st["enabled"] == 1 and st["clamped"] == 0 and st["finest_level"] == 3, st
    assert np.array_equal(got_lev, lev) and np.array_equal(rl, lev)
    if prec == "f64":
        assert ex <= 1e-10 and ev <= 1e-10 and ea <= 1e-12 and ej <= 1e-12, (ex, ev, ea, ej)
    else:
        assert er <= 1e-4 and ea <= 2e-5 and ej <= 2e-5, (er, ea, ej)
    assert b[:, 3].tobytes() == b0[:, 3].astype(sim.dtype).tobytes() and v[:, 3].tobytes() == v0[:, 3].astype(sim.dtype).tobytes()
    assert not a[:, 3].any() and not j[:, 3].any()
    assert bs["enabled"] == 1 and bs["small_steps"] == len(small) and bs["host_steps"] == 8 - len(small), (bs, small)
    assert bs["small_steps"] + bs["host_steps"] == 8


# ---- 2. dynamic decisions, fp64: every level and every count equal to the restatement's -----------------------------------------
def expected_schedule(n):
    """As test_block_decisions_gpu.expected_schedule: per outer step (rows, x, v, a, j, levels, cumulative stats)."""
    if n in R.STORED:
        rec = next(e for e in R.decisions_record()["schedules"] if e["n"] == n)
        lev, st = [np.load(p) for p in R.fixture_paths(n)]
        return [(st[:, 0].astype(np.int64),) + tuple(st[:, c:c + 3] for c in (1, 4, 7, 10)) + (lev, rec["stats"][0])]
    outs, _ = R.run_schedule(n)
    rows = np.arange(n)
    return [(rows,) + tuple(z[:, :3] for z in o[:4]) + o[4:] for o in outs]


@pytest.mark.parametrize("n,small_max", [(1025, 64), (4099, 1024)])
def test_dynamic_decisions_follow_the_restatement(n, small_max):
    p = R.SCHEDULES[n]
    rec = next(e for e in R.decisions_record()["schedules"] if e["n"] == n)
    outs = expected_schedule(n)
    b0, v0 = R.audit_system(n, p["seed"])
    later = max(X_TOL, R.FACTOR * rec["noise_position_dev"])
    assert len(outs) == p["outer"] and rec["stats"][-1]["clamped"] == 0
    with hermite(n, "f64") as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** p["dt_log2"], 1.0)
        sim.set_block_steps(eta=R.ETA, max_level=p["max_level"])
        sim.set_block_batch(depth=16, small_max=small_max)
        for k, (rows, rx, rv, ra, rj, rl, rs) in enumerate(outs):
            sim.simulate(1)
            b, v, a = sim.read()
            j = sim.read_jerk()
            lev = sim.read_levels()
            bs, st = identities(sim)
            errs = [norm_err(g[rows, :3], w) for g, w in ((b, rx), (v, rv), (a, ra), (j, rj))]
            print("N=%d small_max %d outer step %d: %s (restatement %s) %s; positions %.3g, velocities %.3g, a %.3g, j %.3g; levels %s"
                  % (n, small_max, k + 1, st, rs, bs, *errs, np.bincount(lev).tolist()))
            assert np.array_equal(lev, rl), "levels differ for bodies %s" % np.nonzero(lev != rl)[0][:32].tolist()
            for c in COUNTS:
                assert st[c] == rs[c], (c, st, rs)
            assert errs[0] <= (X_TOL if k == 0 else later) and errs[1] <= V_TOL and errs[2] <= A_TOL and errs[3] <= J_TOL, errs
            assert b[:, 3].tobytes() == b0[:, 3].astype(np.float64).tobytes() and v[:, 3].tobytes() == v0[:, 3].astype(np.float64).tobytes()
            assert not a[:, 3].any() and not j[:, 3].any()
        assert bs["small_steps"] > 0 and bs["host_steps"] >= p["outer"], bs      # both paths ran


# ---- 3. bitwise invariants -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bitwise_invariants(prec):
    n, dt = 1025, 2.0 ** -5
    b0, v0 = R.tight_pair(*ic.plummer(n, seed=21))
    blk = dict(eta=0.02, max_level=10)
    with hermite(n, prec) as one, hermite(n, prec) as two:
        for s, depth in ((one, 1), (two, 32)):
            s.init(b0, v0)
            s.set_params(dt, 1.0)
            s.set_block_steps(**blk)
            s.set_block_batch(depth=depth, small_max=256)
        one.simulate(3)
        for k in range(3):
            two.step()
            if k < 2:       # read-only calls between steps change no bit
                two.field(np.zeros((5, 4), two.dtype))
                two.diagnostics()
                two.request_frame()
                two.block_stats()
                two.block_batch_stats()
                two.read_levels()
        assert state(one) == state(two)        # depth 1 against depth 32; nb_step(3) == 3 x nb_step(1); two handles, same bits
        (b1, s1), (b2, s2) = identities(one), identities(two)
        print("%s depth 1: %s; depth 32: %s; %s" % (prec, b1, b2, s1))
        assert s1 == s2 and s1["outer_steps"] == 3 and s1["body_steps"] > 3 * n and s1["finest_level"] > 0, (s1, s2)
        assert b1["small_steps"] == b2["small_steps"] > 0 and b1["host_steps"] == b2["host_steps"] >= 3, (b1, b2)
        assert b1["idle_slots"] == 0 and b1["slots"] == b1["host_waits"] == s1["block_steps"], b1      # depth 1: a wait per block step
        assert b2["host_waits"] < b1["host_waits"], (b1, b2)                                          # depth 32 waits less often
        before = state(one)
        assert one.force_pass(2) > 0.0                         # the full N x N pass into scratch
        assert state(one) == before
        one.simulate(3, 0.0)                                   # dt = 0: a no-op on the state
        assert state(one)[:4] == before[:4]
        assert one.block_stats() == s1
        # checkpoint: (b, v, a, j, levels) after 2 outer steps; a fresh handle with the same small_max and another depth continues
        one.init(b0, v0)
        one.simulate(2, dt, 1.0)
        cb, cv, ca = one.read()
        cj, cl = one.read_jerk(), one.read_levels()
        one.simulate(2)
        with hermite(n, prec) as fresh:
            fresh.init(cb, cv)
            fresh.upload_derivs(ca, cj)
            fresh.set_block_steps(**blk)
            fresh.set_block_batch(depth=7, small_max=256)
            fresh.upload_levels(cl)
            fresh.simulate(2, dt, 1.0)
            assert state(fresh) == state(one)
            identities(fresh)
        # the counters' reset
        one.block_batch_stats(reset=True)
        z = one.block_batch_stats()
        assert z["enabled"] == 1 and all(z[k] == 0 for k in ("host_waits", "slots", "small_steps", "host_steps", "idle_slots")), z


# ---- 4. small_max = 0 is the path of a handle with the mode off ---------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_small_max_zero_is_the_mode_off(prec):
    n, dt = 1025, 2.0 ** -5
    b0, v0 = R.tight_pair(*ic.plummer(n, seed=21))
    with hermite(n, prec) as on, hermite(n, prec) as off:
        for s in (on, off):
            s.init(b0, v0)
            s.set_params(dt, 1.0)
            s.set_block_steps(eta=0.02, max_level=10)
        on.set_block_batch(depth=32, small_max=0)
        on.simulate(3)
        off.simulate(3)
        assert state(on) == state(off)
        assert on.block_stats() == off.block_stats()
        bs, st = identities(on)
        print("%s small_max 0: %s %s" % (prec, bs, st))
        assert bs["small_steps"] == 0 and bs["idle_slots"] == 0 and bs["slots"] == st["block_steps"] == bs["host_steps"], (bs, st)
        assert off.block_batch_stats()["enabled"] == 0


# ---- 5. a row's bits do not depend on |A| or on its place in the list ----------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_small_row_does_not_depend_on_the_active_set(prec):
    """Handle P has only body 700 at level 1, handle Q body 700 and 140 massless bodies: at tick 1 |A| = 1 against 141, and body 700
    sits at list position 0 against the number of massless bodies below it.  Massless rows add exactly +-0 to every sum, so every
    massive row must carry the same bits in both; the massless rows themselves step differently and must differ."""
    n = 1025
    b0, v0 = ic.plummer(n, seed=21)
    b0 = b0.copy()
    others = np.setdiff1d(np.arange(n), [700])
    ghost = np.sort(np.random.default_rng(5).choice(others, 140, replace=False))
    b0[ghost, 3] = 0.0
    massive = np.setdiff1d(np.arange(n), ghost)
    print("body 700 at list position %d of %d" % (int((ghost < 700).sum()), len(ghost) + 1))
    got = {}
    for name, deep in (("P", [700]), ("Q", [700] + ghost.tolist())):
        lev = np.zeros(n, np.uint8)
        lev[deep] = 1
        with hermite(n, prec) as sim:
            sim.init(b0, v0)
            sim.set_params(2.0 ** -4, 1.0)
            sim.set_block_steps(max_level=1, frozen=True)
            sim.set_block_batch(small_max=256)
            sim.upload_levels(lev)
            sim.simulate(2)
            bs, st = identities(sim)
            assert bs["small_steps"] == 2 and bs["host_steps"] == 2 and st["body_steps"] == 2 * (n + len(deep)), (bs, st)
            got[name] = sim.read() + (sim.read_jerk(),)
    for p, q in zip(got["P"], got["Q"]):
        assert p[massive].tobytes() == q[massive].tobytes()
    assert got["P"][0][ghost].tobytes() != got["Q"][0][ghost].tobytes() and got["P"][1][ghost].tobytes() != got["Q"][1][ghost].tobytes()


# ---- 6. counters: the policy on a true hierarchy -------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_policy_on_a_hierarchy(prec):
    """64 bodies at level 6, the rest at level 0: 63 small steps of 64 bodies and one host step per outer step.  With depth 16 the
    ideal is 4 waits and no idle slot (batches of 16, 16, 16, and 15 plus the park); the policy may use 5 and 1."""
    n = 4099
    b0, v0 = ic.plummer(n, seed=21)
    lev = np.zeros(n, np.uint8)
    lev[np.random.default_rng(3).choice(n, 64, replace=False)] = 6
    with hermite(n, prec) as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -4, 1.0)
        sim.set_block_steps(max_level=6, frozen=True)
        sim.set_block_batch(depth=16, small_max=256)
        sim.upload_levels(lev)
        for k in range(5):
            sim.simulate(1)
            bs, st = identities(sim)
            sim.block_batch_stats(reset=True)
            sim.block_stats(reset=True)
            print("%s outer step %d: %s" % (prec, k + 1, bs))
            assert st["block_steps"] == 64 and st["body_steps"] == 63 * 64 + n, st
            assert bs["small_steps"] == 63 and bs["host_steps"] == 1, bs
            if k == 0:
                assert bs["slots"] >= 64
            else:
                assert bs["host_waits"] <= 5 and bs["idle_slots"] <= 1, bs


# ---- 7. errors and switching ---------------------------------------------------------------------------------------------------
def test_errors_and_switching():
    n = 64
    b0, v0 = ic.plummer(n, seed=2)
    L = capi.load_library()

    def refused(call, code, *words):
        with pytest.raises(capi.NBodyError) as e:
            call()
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)

    with Simulation(n) as lf:                                 # a leapfrog handle
        lf.init(b0, v0)
        lf.set_params(1e-3, 1.0)
        refused(lambda: lf.set_block_batch(), 4, "nb_set_block_batch")
    with hermite(n, "f64") as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -6, 1.0)
        refused(lambda: sim.set_block_batch(), 4, "nb_set_block_batch", "nb_set_block_steps")      # no block steps
        assert sim.block_batch_stats()["enabled"] == 0
        sim.set_hermite_order(6)
        sim.set_block_steps6(max_level=4)
        refused(lambda: sim.set_block_batch(), 4, "nb_set_block_batch", "order")                   # an order-6 handle
        sim.set_block_steps6(None)
        sim.set_hermite_order(4)
        sim.set_pass_precision("mixed")
        sim.set_block_steps(max_level=4)
        refused(lambda: sim.set_block_batch(), 4, "nb_set_block_batch", "NB_PASS_MIXED")           # the mixed pass
        sim.set_pass_precision("native")
        cfg = capi.nb_block_batch()
        for field, value in (("struct_size", 12), ("depth", 1025), ("small_max", 1025), ("flags", 1)):
            cfg.struct_size, cfg.depth, cfg.small_max, cfg.flags = C.sizeof(cfg), 0, capi.BLOCK_BATCH_SMALL_DEFAULT, 0
            setattr(cfg, field, value)
            assert L.nb_set_block_batch(sim._h, C.byref(cfg)) == 1, field
            msg = L.nb_last_error(sim._h)
            assert b"nb_set_block_batch" in msg and field.encode() in msg, msg
        st = capi.nb_block_batch_stats()
        st.struct_size = 8
        assert L.nb_block_batch_stats(sim._h, C.byref(st), 0) == 1 and b"struct_size" in L.nb_last_error(sim._h)
        assert sim.block_batch_stats()["enabled"] == 0        # none of the rejected calls switched anything on
        sim.set_block_batch()                                 # the defaults: depth 32, small_max 256
        assert sim.block_batch_stats()["enabled"] == 1
        refused(lambda: sim.set_hermite_order(6), 4, "nb_set_hermite_order", "nb_set_block_batch")
        refused(lambda: sim.set_pass_precision("mixed"), 4, "nb_set_pass_precision", "nb_set_block_batch")
        sim.set_block_steps(max_level=5)                      # a reconfiguration keeps the mode
        assert sim.block_batch_stats()["enabled"] == 1
        sim.simulate(2)
        bs, st = identities(sim)
        assert st["outer_steps"] == 2 and bs["small_steps"] + bs["host_steps"] >= 2, (bs, st)
        sim.set_block_batch(None)
        assert sim.block_batch_stats()["enabled"] == 0 and sim.block_stats()["enabled"] == 1
        sim.set_block_batch(depth=4)
        sim.set_block_steps(None)                             # off with the block steps
        assert sim.block_batch_stats()["enabled"] == 0 and sim.block_stats()["enabled"] == 0
        sim.simulate(1)                                       # a plain Hermite handle again


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
        sim.set_block_batch(depth=16, small_max=8)
        sim.simulate(1, 2.0 ** -3, 1.0)
        a, j = sim.read()[2], sim.read_jerk()
        sim.set_params(2.0 ** -5, 1.0)                     # a change of dt: the start rule on the derivatives as they stand
        assert np.array_equal(sim.read_levels(), start_rule(a, j, 2.0 ** -5, 0.02, 12))
        assert sim.read()[2].tobytes() == a.tobytes()      # the derivatives were kept
        sim.simulate(1)                                    # ... and the run goes on
        sim.init(b0, v0)                                   # a new upload without upload_levels
        a0, j0 = R.fj_ref(b0, v0, 1.0, EPS2)
        assert np.array_equal(sim.read_levels(), start_rule(a0, j0, 2.0 ** -5, 0.02, 12))
        sim.simulate(1)
        bs, st = identities(sim)
        assert st["outer_steps"] == 3 and bs["small_steps"] > 0 and bs["host_steps"] >= 3, (bs, st)


def test_timing_reports_one_outer_step_per_launch():
    n = 1025
    b0, v0 = R.tight_pair(*ic.plummer(n, seed=21))
    with hermite(n, "f32") as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -6, 1.0)
        sim.set_block_steps(max_level=8)
        sim.set_block_batch()
        sim.enable_timing(True)
        sim.simulate(3)
        t = sim.step_breakdown()
        identities(sim)
    assert t["launches"] == 3 and t["force_ms"] > 0 and t["integrate_ms"] == 0 and t["span_ms"] == t["force_ms"], t
