"""Batched block steps on order-6 handles (Simulation.set_block_batch6) on the GPU: block steps with a small active set run from
the device's own header, many per host wait, with the order-6 scheme of set_block_steps6 inside a slot.  Every expected value is
the restatement's (tests/block6_ref.py, tests/golden/block6.json): frozen levels with the exact schedule and the exact split into
small and host steps, a census of the small pass, dynamic levels exactly and within counts, the bitwise invariants (depth, where
batches end, two handles, the seven-array checkpoint), small_max = 0 against a handle with the mode off, a row's bits against |A|,
the small pass's tile loop with two tiles per chunk (orders 6 and 4), the host's policy, the errors and the switches.  f64 runs
dynamic levels and f32 frozen ones (the only f32 order-6 block handles there are)."""
import ctypes as C

import numpy as np
import pytest

from nbody3d_amd import Simulation, capi, ic

import block_ref as B
import block6_ref as R
from block_ref import EPS2, norm_err
from test_block6_gpu import F64_BOUND, arrays, bits, check, check_carried, hermite6, read_state, rel

pytestmark = pytest.mark.gpu

BATCH_COUNTERS = ("host_waits", "slots", "small_steps", "host_steps", "idle_slots")


def identities(sim):
    """The identities of the batch counters against each other and against nb_block_stats (both since the same reset)."""
    bs, st = sim.block_batch_stats(), sim.block_stats()
    assert bs["small_steps"] + bs["host_steps"] == st["block_steps"], (bs, st)
    assert bs["slots"] == bs["small_steps"] + bs["host_steps"] + bs["idle_slots"], bs
    assert bs["host_steps"] <= bs["host_waits"] <= bs["slots"], bs
    return bs, st


def active_at(lev, L, t):
    """|A(t)| of frozen levels: the bodies whose step 2^(L - l) divides t."""
    return int(((t % (1 << (L - lev.astype(np.int64)))) == 0).sum())


# ---- 1. frozen levels: an exact schedule, and which path every block step took -------------------------------------------------
@pytest.mark.parametrize("small_max", [64, 1024])
@pytest.mark.parametrize("n", R.FROZEN_SIZES)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_frozen_levels_follow_the_exact_schedule(prec, n, small_max):
    b0, v0, lev, (ref, rl, rs) = R.frozen_ref(n)
    L = R.L_FROZEN
    sizes = {t: active_at(lev, L, t) for t in range(1, 9)}
    assert all(sizes[t] == 1 for t in (1, 3, 5, 7)) and sizes[8] == n and sizes[2] == sizes[6], sizes
    small = [t for t in range(1, 8) if sizes[t] <= small_max]      # tick 8 is a host step even where small_max >= n
    assert set(small) >= {1, 3, 5, 7} and ((2 in small) == (6 in small) == (sizes[2] <= small_max))
    with hermite6(n, prec) as sim:
        sim.init(b0, v0)
        sim.set_params(R.DT_FROZEN, 1.0)
        sim.set_block_steps6(max_level=L, frozen=True)
        sim.set_block_batch6(depth=8, small_max=small_max)
        sim.upload_levels(lev)
        sim.simulate(1)
        st, got_lev = read_state(sim), sim.read_levels()
        bs, stats = identities(sim)
        check_carried(sim, st, b0, v0)             # mass lanes carried, the .w of a, j, s, c zero
    print("frozen %s N=%d small_max %d: |A(t)| %s, %s %s" % (prec, n, small_max, sizes, stats, bs))
    assert stats["block_steps"] == 8 == rs["block_steps"] and stats["body_steps"] == rs["body_steps"] and stats["outer_steps"] == 1, (stats, rs)
    assert stats["enabled"] == 1 and stats["clamped"] == 0 and stats["finest_level"] == 3, stats
    assert np.array_equal(got_lev, lev) and np.array_equal(rl, lev)
    assert bs["enabled"] == 1 and bs["small_steps"] == len(small) and bs["host_steps"] == 8 - len(small), (bs, small)
    check(R.distances(st, ref, R.DT_FROZEN, L), prec, R.record()["frozen"][str(n)], "frozen N=%d small_max %d" % (n, small_max))


# ---- 2. census of the small pass -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CENSUS))
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_census_of_the_small_pass(prec, name):
    """test_block6_gpu.test_census_of_the_gathered_pass with tick 1 as a small step -- 64 active bodies, with the heavy rows among
    them 66, or 65 at N = 257 where row 256 is the last row too: a tile row that the small pass misses or doubles moves
    (a1, j1, s1) by orders of magnitude above the bounds."""
    b0, v0, lev, (ref, rl, rs) = R.census_ref(name)
    n = len(b0)
    assert active_at(lev, 1, 1) == R.CENSUS_ACTIVE + (len(R.census_heavy(n)) if R.CENSUS[name][1] else 0) <= 66
    with hermite6(n, prec) as sim:
        sim.init(b0, v0)
        sim.set_params(R.DT_CENSUS, 1.0)
        sim.set_block_steps6(max_level=1, frozen=True)
        sim.set_block_batch6(small_max=256)
        sim.upload_levels(lev)
        sim.simulate(1)
        st = read_state(sim)
        bs, stats = identities(sim)
        check_carried(sim, st, b0, v0)
    assert stats["block_steps"] == 2 == rs["block_steps"] and stats["body_steps"] == rs["body_steps"] == n + int(lev.sum()), (stats, rs)
    assert bs["small_steps"] == 1 and bs["host_steps"] == 1, bs
    check(R.distances(st, ref, R.DT_CENSUS, 1), prec, R.record()["census"][name], "census %s" % name)


# ---- 3. dynamic levels, exactly ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", R.TINY)
def test_dynamic_levels_on_tiny_systems_match_the_restatement_exactly(n, seed):
    b0, v0, (ref, rl, rs), margin = R.tiny_ref(n, seed)
    p = R.TINY_RUN
    assert margin >= 5e-4, margin            # no decision near a level boundary: the engine must take the same ones
    with hermite6(n, "f64") as sim:
        sim.init(b0, v0)
        sim.set_block_steps6(eta=p["eta"], max_level=p["max_level"])
        sim.set_block_batch6()
        sim.simulate(p["outer"], p["dt"], 1.0)
        st, lev = read_state(sim), sim.read_levels()
        bs, stats = identities(sim)
    d = R.distances(st, ref, p["dt"], p["max_level"])
    print("engine N=%d: %s %s, %s" % (n, stats, bs, d))
    assert np.array_equal(lev, rl), (lev, rl)
    for k in ("block_steps", "body_steps", "finest_level", "outer_steps"):
        assert stats[k] == rs[k], (k, stats, rs)
    assert stats["clamped"] == 0
    assert all(d[q] <= 1e-10 for q in R.QUANTITIES), d
    assert bs["small_steps"] > 0, bs


# ---- 4. dynamic levels, N = 300 with the tight pair ----------------------------------------------------------------------------
def test_dynamic_levels_on_300_bodies_with_a_tight_pair():
    """The acceptance of test_block6_gpu's case, with small_max 64 so that both paths run."""
    b0, v0, (ref, rl, rs), rde = R.pair300_ref()
    p, rec = R.PAIR300, R.record()["pair300"]
    with hermite6(p["n"], "f64") as sim:
        sim.init(b0, v0)
        sim.set_params(p["dt"], 1.0)
        sim.set_block_steps6(eta=p["eta"], max_level=p["max_level"])
        sim.set_block_batch6(small_max=64)
        k0, p0, _ = sim.diagnostics()
        sim.simulate(p["outer"])
        k1, p1, _ = sim.diagnostics()
        b = sim.read()[0]
        lev = sim.read_levels()
        bs, st = identities(sim)
    de = abs((k1 + p1 - k0 - p0) / (k0 + p0))
    ex, bound = norm_err(b[:, :3], ref["b"][:, :3]), R.FACTOR * rec["noise_position_dev"]
    print("N=300 tight pair: positions %.3g (bound %.3g), |dE/E| %.3g (restatement %.3g), %s (restatement %s) %s, levels %s"
          % (ex, bound, de, rde, st, rs, bs, np.bincount(lev).tolist()))
    assert rel(st["body_steps"], rs["body_steps"]) <= 0.02 and rel(st["block_steps"], rs["block_steps"]) <= 0.02, (st, rs)
    assert st["clamped"] == 0
    assert de <= 10 * rde, (de, rde)
    assert ex <= bound, (ex, bound)
    assert bs["small_steps"] > 0 and bs["host_steps"] > p["outer"], bs      # both paths ran (a host step that is not an outer step's last)


# ---- 5. bitwise invariants -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bitwise_invariants(prec):
    n, dt = 1025, 2.0 ** -5
    b0, v0 = B.tight_pair(*ic.plummer(n, seed=21))
    blk = dict(eta=0.02, max_level=10) if prec == "f64" else dict(max_level=R.L_FROZEN, frozen=True)
    lev0 = None if prec == "f64" else R.frozen_levels(n)

    def begin(s, b, v, depth):
        s.init(b, v)
        s.set_params(dt, 1.0)
        s.set_block_steps6(**blk)
        s.set_block_batch6(depth=depth, small_max=256)
        if lev0 is not None:
            s.upload_levels(lev0)

    with hermite6(n, prec) as one, hermite6(n, prec) as two:
        begin(one, b0, v0, 1)
        begin(two, b0, v0, 32)
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
                two.read_snap()
        assert bits(one) == bits(two)          # depth 1 against depth 32; nb_step(3) == 3 x nb_step(1); two handles, same bits
        (b1, s1), (b2, s2) = identities(one), identities(two)
        print("%s depth 1: %s; depth 32: %s; %s" % (prec, b1, b2, s1))
        assert s1 == s2 and s1["outer_steps"] == 3 and s1["body_steps"] > 3 * n and s1["finest_level"] > 0, (s1, s2)
        assert b1["small_steps"] == b2["small_steps"] > 0 and b1["host_steps"] == b2["host_steps"] >= 3, (b1, b2)
        assert b1["idle_slots"] == 0 and b1["slots"] == b1["host_waits"] == s1["block_steps"], b1      # depth 1: a wait per block step
        assert b2["host_waits"] < b1["host_waits"], (b1, b2)                                          # depth 32 waits less often
        before = bits(one)
        assert one.force_pass(2) > 0.0                         # the full N x N order-6 pass into scratch
        assert bits(one) == before
        one.simulate(3, 0.0)                                   # dt = 0: a no-op on the state
        assert bits(one)[:6] == before[:6]
        assert one.block_stats() == s1
        # checkpoint: the seven arrays after 2 outer steps (c != 0); a fresh handle with the same small_max and another depth continues
        begin(one, b0, v0, 1)
        one.simulate(2)
        cb, cv, ca, cj, cs, cc, cl = arrays(one)
        assert cc[:, :3].any()
        one.simulate(2)
        for start6 in (False, True):
            with hermite6(n, prec) as fresh:
                if start6:
                    fresh.set_start6(1)            # the engine's own starts would differ; an uploaded start is kept
                fresh.init(cb, cv)
                fresh.set_params(dt, 1.0)
                fresh.upload_derivs6(ca, cj, cs, cc)
                fresh.set_block_steps6(**blk)
                fresh.set_block_batch6(depth=7, small_max=256)
                assert tuple(x.tobytes() for x in arrays(fresh)[:6]) == tuple(x.tobytes() for x in (cb, cv, ca, cj, cs, cc))      # the setters left all six
                fresh.upload_levels(cl)
                fresh.simulate(2)
                assert bits(fresh) == bits(one), start6
                identities(fresh)
        # the counters' reset
        one.block_batch_stats(reset=True)
        z = one.block_batch_stats()
        assert z["enabled"] == 1 and all(z[k] == 0 for k in BATCH_COUNTERS), z


# ---- 6. small_max = 0 is the path of a handle with the mode off ---------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_small_max_zero_is_the_mode_off(prec):
    n, dt = 1025, 2.0 ** -5
    b0, v0 = B.tight_pair(*ic.plummer(n, seed=21))
    blk = dict(eta=0.02, max_level=10) if prec == "f64" else dict(max_level=R.L_FROZEN, frozen=True)
    with hermite6(n, prec) as on, hermite6(n, prec) as off:
        for s in (on, off):
            s.init(b0, v0)
            s.set_params(dt, 1.0)
            s.set_block_steps6(**blk)
        on.set_block_batch6(depth=32, small_max=0)
        if prec == "f32":
            for s in (on, off):
                s.upload_levels(R.frozen_levels(n))
        on.simulate(3)
        off.simulate(3)
        assert bits(on) == bits(off)
        assert on.block_stats() == off.block_stats()
        bs, st = identities(on)
        print("%s small_max 0: %s %s" % (prec, bs, st))
        assert bs["small_steps"] == 0 and bs["idle_slots"] == 0 and bs["slots"] == st["block_steps"] == bs["host_steps"], (bs, st)
        assert st["block_steps"] > 3 and off.block_batch_stats()["enabled"] == 0


# ---- 7. a row's bits do not depend on |A| or on its place in the list ----------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_small_row_does_not_depend_on_the_active_set(prec):
    """test_block_batch_gpu's case at order 6.  Handle P has only body 700 at level 1, handle Q body 700 and 140 massless bodies: at
    tick 1 |A| = 1 against 141, and body 700 sits at list position 0 against the number of massless bodies below it.  Massless rows
    add exactly +-0 to every one of the nine sums, so every massive row must carry the same bits in both; the massless rows
    themselves step differently and must differ."""
    n = 1025
    b0, v0 = ic.plummer(n, seed=21)
    b0 = b0.copy()
    others = np.setdiff1d(np.arange(n), [700])
    ghost = np.sort(np.random.default_rng(5).choice(others, 140, replace=False))
    b0[ghost, 3] = 0.0
    massive = np.setdiff1d(np.arange(n), ghost)
    got = {}
    for name, deep in (("P", [700]), ("Q", [700] + ghost.tolist())):
        lev = np.zeros(n, np.uint8)
        lev[deep] = 1
        with hermite6(n, prec) as sim:
            sim.init(b0, v0)
            sim.set_params(2.0 ** -4, 1.0)
            sim.set_block_steps6(max_level=1, frozen=True)
            sim.set_block_batch6(small_max=256)
            sim.upload_levels(lev)
            sim.simulate(2)
            bs, st = identities(sim)
            assert bs["small_steps"] == 2 and bs["host_steps"] == 2 and st["body_steps"] == 2 * (n + len(deep)), (bs, st)
            got[name] = arrays(sim)[:6]
    for p, q in zip(got["P"], got["Q"]):
        assert p[massive].tobytes() == q[massive].tobytes()
    assert got["P"][0][ghost].tobytes() != got["Q"][0][ghost].tobytes() and got["P"][1][ghost].tobytes() != got["Q"][1][ghost].tobytes()


# ---- 8. more than one tile per chunk -------------------------------------------------------------------------------------------
def two_tile_system():
    """n = 256 x CUs + 257: the small pass's chunk rule (one chunk of whole 256-row tiles per CU) then gives 512 rows per chunk, so
    every chunk sweeps two tiles through the double-buffered loop and the last chunk is ragged (257 rows on 256 CUs).  Mass 1e3 at
    the last row of the first tile, at both sides of the border between the first two chunks and at the last row; bodies 0 .. 63 at
    level 1."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 256 * cus + 257
    b0, v0 = ic.plummer(n, seed=21)
    b0 = b0.copy()
    b0[[256, 511, 512, n - 1], 3] = 1e3
    lev = np.zeros(n, np.uint8)
    lev[:R.CENSUS_ACTIVE] = 1
    return n, b0, v0, lev


def two_tile_run(order, prec, on, system):
    n, b0, v0, lev = system
    with Simulation(n, precision=prec, integrator="hermite4") as sim:
        if order == 6:
            sim.set_hermite_order(6)
        sim.init(b0, v0)
        sim.set_params(R.DT_CENSUS, 1.0)
        (sim.set_block_steps6 if order == 6 else sim.set_block_steps)(max_level=1, frozen=True)
        if on:
            (sim.set_block_batch6 if order == 6 else sim.set_block_batch)(small_max=256)
        sim.upload_levels(lev)
        sim.simulate(1)
        st = sim.block_stats()
        assert st["block_steps"] == 2 and st["body_steps"] == n + R.CENSUS_ACTIVE, st
        if on:
            bs = sim.block_batch_stats()
            assert bs["small_steps"] == 1 and bs["host_steps"] == 1, bs
        if order == 6:
            return read_state(sim)
        b, v, a = sim.read()
        return {"x": b[:, :3], "v": v[:, :3], "a": a[:, :3], "j": sim.read_jerk()[:, :3]}


def test_two_tiles_per_chunk():
    """f64: the handle with the mode on against the one without, within the project's bounds.  f32: per quantity, the distance of
    the f32 handle with the mode on from the f64 handle without it is at most FACTOR x the distance of the f32 handle without it:
    the yardstick is the gathered path, no number is fixed here.  A missed or doubled tile moves a, j and s of the 64 rows by
    orders of magnitude."""
    system = two_tile_system()
    ref = two_tile_run(6, "f64", False, system)
    d = R.distances(two_tile_run(6, "f64", True, system), ref, R.DT_CENSUS, 1)
    print("two tiles per chunk, N=%d, f64 on against off: %s" % (system[0], d))
    bad = {q: (d[q], F64_BOUND[q]) for q in R.QUANTITIES if not d[q] <= F64_BOUND[q]}
    assert not bad, bad
    off = R.distances(two_tile_run(6, "f32", False, system), ref, R.DT_CENSUS, 1)
    on = R.distances(two_tile_run(6, "f32", True, system), ref, R.DT_CENSUS, 1)
    print("  f32 against the f64 handle: on %s, off %s" % (on, off))
    bad = {q: (on[q], off[q]) for q in R.QUANTITIES if not on[q] <= R.FACTOR * off[q]}
    assert not bad, bad


def test_two_tiles_per_chunk_at_order_4():
    """The same case through set_block_batch on order-4 handles: (x, v, a, j), f64 within 1e-10 / 1e-12 (norm_err)."""
    system = two_tile_system()
    ref = two_tile_run(4, "f64", False, system)
    got = two_tile_run(4, "f64", True, system)
    d = {q: norm_err(got[q], ref[q]) for q in "xvaj"}
    print("two tiles per chunk at order 4, N=%d, f64 on against off: %s" % (system[0], d))
    assert d["x"] <= 1e-10 and d["v"] <= 1e-10 and d["a"] <= 1e-12 and d["j"] <= 1e-12, d
    g32, o32 = two_tile_run(4, "f32", True, system), two_tile_run(4, "f32", False, system)
    on, off = {q: norm_err(g32[q], ref[q]) for q in "xvaj"}, {q: norm_err(o32[q], ref[q]) for q in "xvaj"}
    print("  f32 against the f64 handle: on %s, off %s" % (on, off))
    bad = {q: (on[q], off[q]) for q in "xvaj" if not on[q] <= R.FACTOR * off[q]}
    assert not bad, bad


# ---- 9. counters: the policy on a true hierarchy -------------------------------------------------------------------------------
def hierarchy(n=4099):
    b0, v0 = ic.plummer(n, seed=21)
    lev = np.zeros(n, np.uint8)
    lev[np.random.default_rng(3).choice(n, 64, replace=False)] = 6
    return n, b0, v0, lev


def test_policy_on_a_hierarchy():
    """64 bodies at level 6, the rest at level 0: 63 small steps of 64 bodies and one host step per outer step.  With depth 16 the
    ideal is 4 waits and no idle slot (batches of 16, 16, 16, and 15 plus the park); the policy may use 5 and 1."""
    n, b0, v0, lev = hierarchy()
    with hermite6(n, "f64") as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -4, 1.0)
        sim.set_block_steps6(max_level=6, frozen=True)
        sim.set_block_batch6(depth=16, small_max=256)
        sim.upload_levels(lev)
        for k in range(5):
            sim.simulate(1)
            bs, st = identities(sim)
            sim.block_batch_stats(reset=True)
            sim.block_stats(reset=True)
            print("outer step %d: %s" % (k + 1, bs))
            assert st["block_steps"] == 64 and st["body_steps"] == 63 * 64 + n, st
            assert bs["small_steps"] == 63 and bs["host_steps"] == 1, bs
            if k == 0:
                assert bs["slots"] >= 64
            else:
                assert bs["host_waits"] <= 5 and bs["idle_slots"] <= 1, bs


# ---- 10. errors and switching --------------------------------------------------------------------------------------------------
def test_errors_and_switching():
    n = 64
    b0, v0 = ic.plummer(n, seed=2)
    L = capi.load_library()

    def refused(call, code, *words):
        with pytest.raises(capi.NBodyError) as e:
            call()
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)

    assert L.nb_set_block_batch6(None, None) == 1 and b"nb_set_block_batch6" in L.nb_last_error(None)      # a NULL handle
    with Simulation(n) as lf:                                 # a leapfrog handle
        lf.init(b0, v0)
        lf.set_params(1e-3, 1.0)
        refused(lambda: lf.set_block_batch6(), 4, "nb_set_block_batch6")
    with Simulation(n, precision="f64", integrator="hermite4") as h4:      # an order-4 handle, with and without block steps
        h4.init(b0, v0)
        h4.set_params(2.0 ** -6, 1.0)
        refused(lambda: h4.set_block_batch6(), 4, "nb_set_block_batch6", "nb_set_hermite_order")
        h4.set_block_steps(max_level=4)
        refused(lambda: h4.set_block_batch6(), 4, "nb_set_block_batch6", "nb_set_hermite_order")
        assert h4.block_batch_stats()["enabled"] == 0
    with hermite6(n, "f64") as sim, hermite6(n, "f64") as plain:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -6, 1.0)
        refused(lambda: sim.set_block_batch6(), 4, "nb_set_block_batch6", "nb_set_block_steps6")      # no block steps
        sim.set_block_steps6(max_level=4)
        refused(lambda: sim.set_block_batch(), 4, "nb_set_block_batch", "order")                       # the order-4 entry point stays refused
        cfg = capi.nb_block_batch()
        for field, value in (("struct_size", 12), ("depth", 1025), ("small_max", 1025), ("flags", 1)):
            cfg.struct_size, cfg.depth, cfg.small_max, cfg.flags = C.sizeof(cfg), 0, capi.BLOCK_BATCH_SMALL_DEFAULT, 0
            setattr(cfg, field, value)
            assert L.nb_set_block_batch6(sim._h, C.byref(cfg)) == 1, field
            msg = L.nb_last_error(sim._h)
            assert b"nb_set_block_batch6" in msg and field.encode() in msg, msg
        assert sim.block_batch_stats()["enabled"] == 0        # none of the rejected calls switched anything on
        sim.set_block_batch6()                                # the defaults: depth 32, small_max 256
        assert sim.block_batch_stats()["enabled"] == 1
        refused(lambda: sim.set_hermite_order(4), 4, "nb_set_hermite_order", "nb_set_block_steps6")
        refused(lambda: sim.set_neighbor_scheme(radius=0.1), 4, "nb_set_neighbor_scheme")
        sim.set_start6(1)                                     # keeps working
        sim.set_start6(0)
        sim.set_block_steps6(max_level=5)                     # a reconfiguration keeps the mode
        assert sim.block_batch_stats()["enabled"] == 1
        sim.simulate(2)
        bs, st = identities(sim)
        assert st["outer_steps"] == 2 and bs["small_steps"] + bs["host_steps"] >= 2, (bs, st)
        for off in ("set_block_batch6", "set_block_batch"):  # off through the two batch setters: the block steps stay
            getattr(sim, off)(None)
            assert sim.block_batch_stats()["enabled"] == 0 and sim.block_stats()["enabled"] == 1
            sim.set_block_batch6(depth=4)
            assert sim.block_batch_stats()["enabled"] == 1
        sim.set_block_steps(None)                             # off with the block steps, through either setter
        assert sim.block_batch_stats()["enabled"] == 0 and sim.block_stats()["enabled"] == 0
        sim.set_block_steps6(max_level=5)
        assert sim.block_batch_stats()["enabled"] == 0        # switching the block steps on again does not bring the mode back
        sim.set_block_batch6(depth=4)
        sim.simulate(1)
        cb, cv, ca, cj, cs, cc, _ = arrays(sim)
        sim.set_block_steps6(None)
        assert sim.block_batch_stats()["enabled"] == 0 and sim.block_stats()["enabled"] == 0 and sim.hermite_order() == 6
        sim.simulate(3)                                       # a plain order-6 handle again
        plain.init(cb, cv)
        plain.upload_derivs6(ca, cj, cs, cc)
        plain.simulate(3, 2.0 ** -6, 1.0)
        assert tuple(x.tobytes() for x in arrays_plain(sim)) == tuple(x.tobytes() for x in arrays_plain(plain))


def arrays_plain(sim):
    b, v, a = sim.read()
    return (b, v, a, sim.read_jerk()) + tuple(sim.read_snap())


def start_rule(a, j, dt, eta, L):
    margins, stats = [], {"clamped": 0}
    lev = B.start_levels(a[:, :3], j[:, :3], dt, eta, 0, L, stats, margins)
    assert min(margins) >= 1e-3, min(margins)              # the system was chosen so: no start decision near a level boundary
    return lev.astype(np.uint8)


def test_a_change_of_dt_and_a_new_upload_reinitialise_the_levels():
    n = 12
    b0, v0 = B.tight_pair(*ic.plummer(n, seed=3))
    with hermite6(n, "f64") as sim:
        sim.init(b0, v0)
        sim.set_block_steps6(eta=0.02, max_level=12)
        sim.set_block_batch6(depth=16, small_max=8)
        sim.simulate(1, 2.0 ** -3, 1.0)
        a, j = sim.read()[2], sim.read_jerk()
        c = sim.read_snap()[1]
        sim.set_params(2.0 ** -5, 1.0)                     # a change of dt: the start rule on the derivatives as they stand
        assert np.array_equal(sim.read_levels(), start_rule(a, j, 2.0 ** -5, 0.02, 12))
        assert sim.read()[2].tobytes() == a.tobytes() and sim.read_snap()[1].tobytes() == c.tobytes()      # the derivatives were kept
        sim.simulate(1)                                    # ... and the run goes on
        sim.init(b0, v0)                                   # a new upload without upload_levels
        a0, j0 = B.fj_ref(b0, v0, 1.0, EPS2)
        assert np.array_equal(sim.read_levels(), start_rule(a0, j0, 2.0 ** -5, 0.02, 12))
        sim.simulate(1)
        bs, st = identities(sim)
        assert st["outer_steps"] == 3 and bs["small_steps"] > 0 and bs["host_steps"] >= 3, (bs, st)


def test_stale_levels_restart_the_policy_at_one_slot():
    """The hierarchy of the policy test with a depth that holds a whole outer step: once the host has read the schedule an outer step
    is ONE batch of 64 slots.  After a change of dt (the levels uploaded again) and after the setter itself the policy knows nothing:
    the first batch is one slot, the rest of the outer step the second."""
    n, b0, v0, lev = hierarchy()
    with hermite6(n, "f64") as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -4, 1.0)
        sim.set_block_steps6(max_level=6, frozen=True)
        sim.set_block_batch6(depth=1024, small_max=256)
        sim.upload_levels(lev)

        def outer_step():
            sim.block_batch_stats(reset=True)
            sim.simulate(1)
            bs = sim.block_batch_stats()
            assert bs["small_steps"] == 63 and bs["host_steps"] == 1 and bs["idle_slots"] == 0, bs
            return bs["host_waits"], bs["slots"]

        assert outer_step() == (2, 64)
        assert outer_step() == (1, 64)
        sim.set_params(2.0 ** -5, 1.0)
        sim.upload_levels(lev)
        assert outer_step() == (2, 64)
        assert outer_step() == (1, 64)
        sim.set_block_batch6(depth=1024, small_max=256)    # touches no levels (they stay current), restarts the policy
        assert np.array_equal(sim.read_levels(), lev)
        assert outer_step() == (2, 64)


# ---- 11. timing ----------------------------------------------------------------------------------------------------------------
def test_timing_reports_one_outer_step_per_launch():
    n = 1025
    b0, v0 = B.tight_pair(*ic.plummer(n, seed=21))
    with hermite6(n, "f64") as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -6, 1.0)
        sim.set_block_steps6(max_level=8)
        sim.set_block_batch6()
        sim.enable_timing(True)
        sim.simulate(3)
        t = sim.step_breakdown()
        identities(sim)
    assert t["launches"] == 3 and t["force_ms"] > 0 and t["integrate_ms"] == 0 and t["span_ms"] == t["force_ms"], t
