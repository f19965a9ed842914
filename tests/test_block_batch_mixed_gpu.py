"""Batched block steps on mixed-precision handles (Simulation.set_block_batch_mixed) on the GPU: tests/test_block_batch_gpu.py's cases
on f64 handles with set_pass_precision("mixed").  Frozen levels with an exact schedule and the exact split into small and host
steps against the restatement of the double-single pass (tests/mixed_ref.py in tests/block_ref.py's loop), dynamic levels on hard
pairs against the recorded fp64 figures, the bitwise invariants (depth, where batches end, two handles, a checkpoint), small_max = 0
against a mixed handle with the mode off, a row's bits against |A| and its place in the active list, two tiles per chunk with a
ragged last chunk as a census of the rows, the host's policy, and the errors."""
import ctypes as C

import numpy as np
import pytest

from nbody3d_amd import Simulation, capi, ic

import block_ref as R
import mixed_ref as M
import block_batch_mixed_ref as Q
from block_ref import EPS2, norm_err
from block6_ref import frozen_levels

pytestmark = pytest.mark.gpu


def handle(n, mixed=True, prec="f64", **kw):
    sim = Simulation(n, precision=prec, integrator="hermite4", **kw)
    if mixed:
        sim.set_pass_precision("mixed")
    return sim


def state(sim):
    return tuple(x.tobytes() for x in sim.read()) + (sim.read_jerk().tobytes(), sim.read_levels().tobytes())


def identities(sim):
    """The identities of the batch counters against each other and against nb_block_stats (both since the same reset)."""
    bs, st = sim.block_batch_stats(), sim.block_stats()
    assert bs["small_steps"] + bs["host_steps"] == st["block_steps"], (bs, st)
    assert bs["slots"] == bs["small_steps"] + bs["host_steps"] + bs["idle_slots"], bs
    assert bs["host_steps"] <= bs["host_waits"] <= bs["slots"], bs
    return bs, st


def refused(call, code, *words):
    with pytest.raises(capi.NBodyError) as e:
        call()
    assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)


# ---- 1. frozen levels: an exact schedule, and which path every block step took -------------------------------------------------
_frozen = {}
DT_FROZEN, L_FROZEN = 2.0 ** -4, 3


def frozen_system(n):
    """A Plummer sphere in float64 whose rows binary32 does not hold (every lo word is in play from the start), and the levels."""
    b0, v0 = [np.array(z, np.float64) for z in ic.plummer(n, seed=21)]
    b0[:, :3] += 1e-9
    return b0, v0, frozen_levels(n)


def frozen_ref(n):
    """(b0, v0, levels, the restatement with the kernel's binary32 sums, the bounds on positions and velocities): FACTOR x the
    distance between the restatements with binary32 and with fp64 sums, at least 1e-9 -- test_mixed_gpu's rule.  Once per size."""
    if n not in _frozen:
        b0, v0, lev = frozen_system(n)
        run = lambda acc: R.block_ref(b0, v0, 1.0, EPS2, DT_FROZEN, 1, max_level=L_FROZEN, levels=lev, frozen=True, fj=M.with_acc(acc))
        f32, f64 = run("f32"), run("fp64")
        tol = tuple(max(1e-9, M.FACTOR * norm_err(f32[k][:, :3], f64[k][:, :3])) for k in (0, 1))
        _frozen[n] = (b0, v0, lev, f32, tol)
    return _frozen[n]


def active_at(lev, L, t):
    """|A(t)| of frozen levels: the bodies whose step 2^(L - l) divides t."""
    return int(((t % (1 << (L - lev.astype(np.int64)))) == 0).sum())


def expected_small(n, lev, small_max):
    sizes = {t: active_at(lev, L_FROZEN, t) for t in range(1, 9)}
    assert all(sizes[t] == 1 for t in (1, 3, 5, 7)) and sizes[8] == n
    assert sizes[2] == sizes[6] and (sizes[2] == 1 if n == 2 else sizes[2] == 38 if n == 77 else 64 < sizes[2] <= 1024), sizes
    small = [t for t in range(1, 8) if sizes[t] <= small_max]      # tick 8 is a host step even where small_max > n
    assert set(small) >= {1, 3, 5, 7} and ((2 in small and 6 in small) == (n < 1025 or small_max == 1024))
    return small


def frozen_run(n, b0, v0, lev, small_max, mixed=True):
    """One outer step; small_max None: the mode off.  (bodies, vel, block_stats, batch stats or None, levels)"""
    with handle(n, mixed=mixed) as sim:
        sim.init(b0, v0)
        sim.set_params(DT_FROZEN, 1.0)
        sim.set_block_steps(max_level=L_FROZEN, frozen=True)
        if small_max is not None:
            sim.set_block_batch_mixed(depth=8, small_max=small_max)
        sim.upload_levels(lev)
        sim.simulate(1)
        b, v, a = sim.read()
        j = sim.read_jerk()
        bs, st = identities(sim) if small_max is not None else (None, sim.block_stats())
        assert b[:, 3].tobytes() == b0[:, 3].tobytes() and v[:, 3].tobytes() == v0[:, 3].tobytes()
        assert b.dtype == np.float64 and not a[:, 3].any() and not j[:, 3].any()
        return b, v, st, bs, sim.read_levels()


@pytest.mark.parametrize("small_max", [64, 1024])
@pytest.mark.parametrize("n", [2, 77, 1025])
def test_frozen_levels_follow_the_exact_schedule(n, small_max):
    b0, v0, lev, (rb, rv, ra, rj, rl, rs), (tx, tv) = frozen_ref(n)
    small = expected_small(n, lev, small_max)
    b, v, st, bs, got_lev = frozen_run(n, b0, v0, lev, small_max)
    ex, ev = norm_err(b[:, :3], rb[:, :3]), norm_err(v[:, :3], rv[:, :3])
    print("mixed frozen N=%d small_max %d: positions %.3g (bound %.3g), velocities %.3g (bound %.3g); %s %s" % (n, small_max, ex, tx, ev, tv, st, bs))
    assert st["block_steps"] == 8 == rs["block_steps"] and st["body_steps"] == rs["body_steps"] and st["outer_steps"] == 1, (st, rs)
    assert st["enabled"] == 1 and st["clamped"] == 0 and st["finest_level"] == 3, st
    assert np.array_equal(got_lev, lev) and np.array_equal(rl, lev)
    assert bs["enabled"] == 1 and bs["small_steps"] == len(small) and bs["host_steps"] == 8 - len(small), (bs, small)
    assert ex <= tx and ev <= tv, (ex, tx, ev, tv)


@pytest.mark.parametrize("small_max", [64, 1024])
def test_frozen_levels_at_4099_against_the_mode_off(small_max):
    """N = 4,099 (two j-chunks of the gathered pass, 17 of the small one): the same counts, and positions and velocities against a
    mixed handle with the mode OFF within max(1e-9, FACTOR x the distance between that handle and a native f64 handle)."""
    n = 4099
    if n not in _frozen:
        b0, v0, lev = frozen_system(n)
        off, native = frozen_run(n, b0, v0, lev, None), frozen_run(n, b0, v0, lev, None, mixed=False)
        _frozen[n] = (b0, v0, lev, off, tuple(max(1e-9, M.FACTOR * norm_err(off[k][:, :3], native[k][:, :3])) for k in (0, 1)))
    b0, v0, lev, (rb, rv, rst, _, _), (tx, tv) = _frozen[n]
    small = expected_small(n, lev, small_max)
    b, v, st, bs, got_lev = frozen_run(n, b0, v0, lev, small_max)
    ex, ev = norm_err(b[:, :3], rb[:, :3]), norm_err(v[:, :3], rv[:, :3])
    print("mixed frozen N=%d small_max %d against the mode off: positions %.3g (bound %.3g), velocities %.3g (bound %.3g); %s %s"
          % (n, small_max, ex, tx, ev, tv, st, bs))
    assert st == rst and st["block_steps"] == 8 and st["body_steps"] == sum(active_at(lev, L_FROZEN, t) for t in range(1, 9)), (st, rst)
    assert np.array_equal(got_lev, lev)
    assert bs["enabled"] == 1 and bs["small_steps"] == len(small) and bs["host_steps"] == 8 - len(small), (bs, small)
    assert ex <= tx and ev <= tv, (ex, tx, ev, tv)


# ---- 2. dynamic levels on hard pairs -------------------------------------------------------------------------------------------
def test_dynamic_levels_follow_the_fp64_schedule():
    """mixed_ref.BLOCK (512 bodies, four pairs 2e-3 apart, eps2 1e-8, dt 2^-4, max_level 16, eta 0.02, four outer steps) with
    small_max 256 and depth 16 against the fp64 restatement recorded in mixed.json, under test_mixed_gpu's conditions: block steps
    within 2 %, body steps within 0.5 %, nothing clamped; both paths ran.  The energy condition is |dE/E0| <= FACTOR x the recorded
    fp64 figure (1.61e-7), not test_mixed_gpu's 2 x: the gathered pass meets that one with 5 - 8 % room in ITS summation order, and
    the small pass adds the same terms in another (four quarters of a chunk in wave order, one chunk per CU).  The failures the
    condition is there for are far away: a binary32-storing handle sits at 56 x the fp64 figure, and a lost lo word fails the
    counts (+1,466 % block steps).  The mixed handle without the mode and the native f64 handle run beside it and are printed.
    On an MI355X (profiles/r27/block_batch_mixed.md), block steps / body steps / |dE/E0|: batched 2,070 / 37,250 / 2.22e-7 (2,052
    small steps, 18 host steps, 132 waits); mode off 2,070 / 37,246 / 2.98e-7; native 2,070 / 37,242 / 1.61e-7, the fp64
    restatement's figures exactly."""
    k, ref = M.BLOCK, M.record()["block"]["fp64"]
    b0, v0 = M.block_system()
    e0, got = R.energy(b0, v0, 1.0, k["eps2"]), {}
    for name, mixed, batch in (("on", True, True), ("off", True, False), ("native", False, False)):
        with handle(k["n"], mixed=mixed, eps2=k["eps2"]) as sim:
            sim.init(b0, v0)
            sim.set_params(k["dt"], 1.0)
            sim.set_block_steps(eta=k["eta"], max_level=k["max_level"])
            if batch:
                sim.set_block_batch_mixed(depth=16, small_max=256)
            sim.simulate(k["outer"])
            b, v, _ = sim.read()
            bs = identities(sim)[0] if batch else None
            got[name] = (sim.block_stats(), abs((R.energy(b, v, 1.0, k["eps2"]) - e0) / e0), bs)
    st, de, bs = got["on"]
    print("mixed dynamic levels, batched: %s %s, |dE/E0| %.3g; mode off: %s, |dE/E0| %.3g; native f64 handle: %s, |dE/E0| %.3g; fp64 restatement %s"
          % (st, bs, de, got["off"][0], got["off"][1], got["native"][0], got["native"][1], ref))
    assert abs(st["block_steps"] - ref["block_steps"]) <= 0.02 * ref["block_steps"], (st, ref)
    assert abs(st["body_steps"] - ref["body_steps"]) <= 0.005 * ref["body_steps"], (st, ref)
    assert st["clamped"] == 0 and st["outer_steps"] == k["outer"], st
    assert bs["small_steps"] > 0 and bs["host_steps"] >= k["outer"], bs      # both paths ran
    assert de <= M.FACTOR * ref["dE"], (de, ref["dE"])


# ---- 3. bitwise invariants -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setter_first", [True, False])
def test_bitwise_invariants(setter_first):
    n, dt = 1025, 2.0 ** -5
    b0, v0 = R.tight_pair(*ic.plummer(n, seed=21))
    blk = dict(eta=0.02, max_level=10)
    with handle(n) as one, handle(n) as two:
        for s, depth in ((one, 1), (two, 32)):
            s.init(b0, v0)
            s.set_params(dt, 1.0)
            s.set_block_steps(**blk)
            s.set_block_batch_mixed(depth=depth, small_max=256)
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
        print("mixed depth 1: %s; depth 32: %s; %s" % (b1, b2, s1))
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
        # checkpoint: the five fp64 arrays after 2 outer steps; a fresh handle with the same small_max and another depth continues
        one.init(b0, v0)
        one.simulate(2, dt, 1.0)
        cb, cv, ca = one.read()
        cj, cl = one.read_jerk(), one.read_levels()
        assert all(z.dtype == np.float64 for z in (cb, cv, ca, cj))
        one.simulate(2)
        with handle(n, mixed=False) as fresh:
            fresh.init(cb, cv)
            if setter_first:
                fresh.set_pass_precision("mixed")
            fresh.upload_derivs(ca, cj)
            if not setter_first:
                fresh.set_pass_precision("mixed")
            fresh.set_block_steps(**blk)
            fresh.set_block_batch_mixed(depth=7, small_max=256)
            fresh.upload_levels(cl)
            fresh.simulate(2, dt, 1.0)
            assert state(fresh) == state(one)
            identities(fresh)
        # the counters' reset
        one.block_batch_stats(reset=True)
        z = one.block_batch_stats()
        assert z["enabled"] == 1 and all(z[k] == 0 for k in ("host_waits", "slots", "small_steps", "host_steps", "idle_slots")), z


# ---- 4. small_max = 0 is the path of a mixed handle with the mode off ----------------------------------------------------------
def test_small_max_zero_is_the_mode_off():
    n, dt = 1025, 2.0 ** -5
    b0, v0 = R.tight_pair(*ic.plummer(n, seed=21))
    with handle(n) as on, handle(n) as off:
        for s in (on, off):
            s.init(b0, v0)
            s.set_params(dt, 1.0)
            s.set_block_steps(eta=0.02, max_level=10)
        on.set_block_batch_mixed(depth=32, small_max=0)
        on.simulate(3)
        off.simulate(3)
        assert state(on) == state(off)
        assert on.block_stats() == off.block_stats()
        bs, st = identities(on)
        print("mixed small_max 0: %s %s" % (bs, st))
        assert bs["small_steps"] == 0 and bs["idle_slots"] == 0 and bs["slots"] == st["block_steps"] == bs["host_steps"], (bs, st)
        assert off.block_batch_stats()["enabled"] == 0


# ---- 5. a row's bits do not depend on |A| or on its place in the list ----------------------------------------------------------
def test_a_small_row_does_not_depend_on_the_active_set():
    """Handle P has only body 700 at level 1, handle Q body 700 and 140 massless bodies: at tick 1 |A| = 1 against 141, and body 700
    sits at list position 0 against the number of massless bodies below it.  Massless rows add exactly +-0 to every sum, so every
    massive row must carry the same bits in both; the massless rows themselves step differently and must differ."""
    n = 1025
    b0, v0 = [np.array(z, np.float64) for z in ic.plummer(n, seed=21)]
    b0[:, :3] += 1e-9
    others = np.setdiff1d(np.arange(n), [700])
    ghost = np.sort(np.random.default_rng(5).choice(others, 140, replace=False))
    b0[ghost, 3] = 0.0
    massive = np.setdiff1d(np.arange(n), ghost)
    print("body 700 at list position %d of %d" % (int((ghost < 700).sum()), len(ghost) + 1))
    got = {}
    for name, deep in (("P", [700]), ("Q", [700] + ghost.tolist())):
        lev = np.zeros(n, np.uint8)
        lev[deep] = 1
        with handle(n) as sim:
            sim.init(b0, v0)
            sim.set_params(2.0 ** -4, 1.0)
            sim.set_block_steps(max_level=1, frozen=True)
            sim.set_block_batch_mixed(small_max=256)
            sim.upload_levels(lev)
            sim.simulate(2)
            bs, st = identities(sim)
            assert bs["small_steps"] == 2 and bs["host_steps"] == 2 and st["body_steps"] == 2 * (n + len(deep)), (bs, st)
            got[name] = sim.read() + (sim.read_jerk(),)
    for p, q in zip(got["P"], got["Q"]):
        assert p[massive].tobytes() == q[massive].tobytes()
    assert got["P"][0][ghost].tobytes() != got["Q"][0][ghost].tobytes() and got["P"][1][ghost].tobytes() != got["Q"][1][ghost].tobytes()


# ---- 6. two tiles per chunk, a ragged last chunk, and a census of the rows -----------------------------------------------------
def two_tile_run(system, mixed, on):
    n, b0, v0, lev, _ = system
    with handle(n, mixed=mixed, eps2=Q.EPS2) as sim:
        sim.init(b0, v0)
        sim.set_params(Q.DT, 1.0)
        sim.set_block_steps(max_level=1, frozen=True)
        if on:
            sim.set_block_batch_mixed(small_max=256)
        sim.upload_levels(lev)
        sim.simulate(1)
        st = sim.block_stats()
        assert st["block_steps"] == 2 and st["body_steps"] == n + Q.ACTIVE, st
        if on:
            bs = sim.block_batch_stats()
            assert bs["small_steps"] == 1 and bs["host_steps"] == 1, bs
        return sim.read()[1][:Q.ACTIVE, :3]


def test_two_tiles_per_chunk_and_a_ragged_last_chunk():
    """n = 256 x CUs + 257 (block_batch_mixed_ref.two_tile_system): every chunk of the small pass sweeps two tiles through the
    double-buffered loop, the last chunk has 257 rows.  The velocities of the 64 small-step bodies against the mixed handle with the
    mode off, within max(1e-9, FACTOR x the distance between that handle and a native f64 handle).  It is a census: rows at both
    ends of a wave's quarter, of a tile and of a chunk, and every row of the ragged chunk, carry 64 x the common mass, and leaving
    out or doubling any ONE of them moves a velocity by at least 4 x the bound (asserted here with the measured bound, and in
    test_block_batch_mixed_cpu.py with an estimated one)."""
    import torch
    system = Q.two_tile_system(torch.cuda.get_device_properties(0).multi_processor_count)
    off, native, on = two_tile_run(system, True, False), two_tile_run(system, False, False), two_tile_run(system, True, True)
    bound = max(1e-9, M.FACTOR * norm_err(off, native))
    d, moves = norm_err(on, off), Q.census_moves(system)
    print("two tiles per chunk, N=%d: velocities on against off %.3g (bound %.3g); one heavy row moves a velocity by %.3g at least (x %.1f the bound)"
          % (system[0], d, bound, moves.min(), moves.min() / bound))
    assert moves.min() >= 4 * bound, (moves.min(), bound)
    assert d <= bound, (d, bound)


# ---- 7. counters: the policy on a true hierarchy -------------------------------------------------------------------------------
def test_policy_on_a_hierarchy():
    """64 bodies at level 6, the rest at level 0: 63 small steps of 64 bodies and one host step per outer step.  With depth 16 the
    ideal is 4 waits and no idle slot (batches of 16, 16, 16, and 15 plus the park); the policy may use 5 and 1."""
    n = 4099
    b0, v0 = ic.plummer(n, seed=21)
    lev = np.zeros(n, np.uint8)
    lev[np.random.default_rng(3).choice(n, 64, replace=False)] = 6
    with handle(n) as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -4, 1.0)
        sim.set_block_steps(max_level=6, frozen=True)
        sim.set_block_batch_mixed(depth=16, small_max=256)
        sim.upload_levels(lev)
        for k in range(5):
            sim.simulate(1)
            bs, st = identities(sim)
            sim.block_batch_stats(reset=True)
            sim.block_stats(reset=True)
            print("mixed outer step %d: %s" % (k + 1, bs))
            assert st["block_steps"] == 64 and st["body_steps"] == 63 * 64 + n, st
            assert bs["small_steps"] == 63 and bs["host_steps"] == 1, bs
            if k == 0:
                assert bs["slots"] >= 64
            else:
                assert bs["host_waits"] <= 5 and bs["idle_slots"] <= 1, bs


# ---- 8. errors and switching ---------------------------------------------------------------------------------------------------
def test_errors_and_switching():
    n = 64
    b0, v0 = ic.plummer(n, seed=2)
    L = capi.load_library()
    NAME = "nb_set_block_batch_mixed"
    enabled = lambda sim: sim.block_batch_stats()["enabled"]

    with Simulation(n, precision="f64") as lf:                # a leapfrog handle
        lf.init(b0, v0)
        lf.set_params(1e-3, 1.0)
        refused(lambda: lf.set_block_batch_mixed(), 4, NAME, "Hermite handle")
    with handle(n, mixed=False, prec="f32") as f32:           # an NB_F32 handle
        f32.init(b0, v0)
        f32.set_params(2.0 ** -6, 1.0)
        f32.set_block_steps(max_level=4)
        refused(lambda: f32.set_block_batch_mixed(), 4, NAME, "NB_F32", "nb_set_block_batch")
        assert enabled(f32) == 0
    with handle(n, mixed=False) as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -6, 1.0)
        sim.set_hermite_order(6)
        sim.set_block_steps6(max_level=4)
        refused(lambda: sim.set_block_batch_mixed(), 4, NAME, "order", "nb_set_hermite_order")       # an order-6 handle
        sim.set_block_steps6(None)
        sim.set_hermite_order(4)
        sim.set_pass_precision("mixed")
        refused(lambda: sim.set_block_batch_mixed(), 4, NAME, "nb_set_block_steps")                  # no block steps
        sim.set_pass_precision("native")
        sim.set_block_steps(max_level=4)
        refused(lambda: sim.set_block_batch_mixed(), 4, NAME, "nb_set_pass_precision", "nb_set_block_batch")      # a native-precision handle
        sim.set_pass_precision("mixed")
        sim.set_pass_guard(1e-3)
        refused(lambda: sim.set_block_batch_mixed(), 4, NAME, "nb_set_pass_guard")                   # a guarded handle
        sim.set_pass_guard(0.0)
        refused(lambda: sim.set_block_batch(), 4, "nb_set_block_batch", "NB_PASS_MIXED")             # the native setter stays refused
        cfg = capi.nb_block_batch()
        for field, value in (("struct_size", 12), ("depth", 1025), ("small_max", 1025), ("flags", 1)):
            cfg.struct_size, cfg.depth, cfg.small_max, cfg.flags = C.sizeof(cfg), 0, capi.BLOCK_BATCH_SMALL_DEFAULT, 0
            setattr(cfg, field, value)
            assert L.nb_set_block_batch_mixed(sim._h, C.byref(cfg)) == 1, field
            msg = L.nb_last_error(sim._h)
            assert NAME.encode() in msg and field.encode() in msg, msg
        assert enabled(sim) == 0                              # none of the refused calls switched anything on
        sim.set_block_batch_mixed()                           # the defaults: depth 32, small_max 256
        assert enabled(sim) == 1
        # while the mode is on
        refused(lambda: sim.set_pass_precision("native"), 4, "nb_set_pass_precision", NAME)
        sim.set_pass_precision("mixed")                       # changes nothing: NB_OK
        refused(lambda: sim.set_pass_guard(1e-3), 4, "nb_set_pass_guard", NAME)
        sim.set_pass_guard(0.0)                               # changes nothing: NB_OK
        refused(lambda: sim.set_hermite_order(6), 4, "nb_set_hermite_order")
        refused(lambda: sim.set_neighbor_scheme(radius=0.2), 4, "nb_set_neighbor_scheme")
        refused(lambda: sim.set_block_batch(), 4, "nb_set_block_batch", "NB_PASS_MIXED")
        assert enabled(sim) == 1 and sim.pass_precision() == "mixed" and sim.pass_guard() == 0.0 and sim.hermite_order() == 4
        sim.set_block_steps(max_level=5)                      # a reconfiguration keeps the mode
        assert enabled(sim) == 1
        sim.simulate(2)
        bs, st = identities(sim)
        assert st["outer_steps"] == 2 and bs["small_steps"] + bs["host_steps"] >= 2 and bs["small_steps"] > 0, (bs, st)
        # each of the four switches it off
        for off in (lambda: sim.set_block_batch_mixed(None), lambda: sim.set_block_batch(None), lambda: sim.set_block_batch6(None)):
            off()
            assert enabled(sim) == 0 and sim.block_stats()["enabled"] == 1 and sim.pass_precision() == "mixed"
            sim.set_block_batch_mixed(depth=4)
            assert enabled(sim) == 1
        sim.set_block_steps(None)                             # off with the block steps
        assert enabled(sim) == 0 and sim.block_stats()["enabled"] == 0
        sim.simulate(1)                                       # a plain mixed Hermite handle again
        # after set_block_batch_mixed(None) the precision is free again, and set_block_batch() then runs the native mode
        sim.set_block_steps(max_level=5)
        sim.set_block_batch_mixed()
        sim.set_block_batch_mixed(None)
        sim.set_pass_precision("native")
        assert sim.pass_precision() == "native" and sim.variant.startswith("hermite4_f64_")
        sim.set_block_batch()
        assert enabled(sim) == 1
        refused(lambda: sim.set_pass_precision("mixed"), 4, "nb_set_pass_precision", "nb_set_block_batch")      # the present words
        sim.block_batch_stats(reset=True)
        sim.block_stats(reset=True)
        sim.simulate(2)
        bs, st = identities(sim)
        assert st["outer_steps"] == 2 and bs["small_steps"] > 0, (bs, st)
