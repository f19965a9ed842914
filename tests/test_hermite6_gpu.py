"""The 6th-order Hermite scheme (nb_set_hermite_order(6)) on the GPU: the force+jerk+snap pass against an fp64 direct sum, steps
against the numpy restatement (tests/hermite6_ref.py), the bitwise invariants (step batching, two handles, checkpoint restore with
a crackle that is not zero), changed dt and G, the Kepler runs of the CPU convergence test, order switching, queries behind a
stepped handle and the errors.  Sizes 2, 3, 257, 1,025, 4,099: the smallest with a partial tile, a second i-block, a last lane
group of one body and a second j-chunk.  f64 handles: 1e-12 on the row metric, 1e-10 on states; f32 handles: 8 x what the binary32
restatement of the same case is off by (tests/golden/hermite6.json, recorded on the CPU)."""
import numpy as np
import pytest

from nbody3d_amd import Simulation, capi

import hermite6_ref as R

pytestmark = pytest.mark.gpu

PRECS = ["f32", "f64"]


def h6(n, prec, **kw):
    return Simulation(n, precision=prec, integrator="hermite6", **kw)


def state(sim):
    b, v, a = sim.read()
    j = sim.read_jerk()
    s, c = sim.read_snap()
    for z in (a, j, s, c):
        assert not z[:, 3].any()                       # the .w of a, j, s and c is 0
    return {"b": b, "v": v, "a": a[:, :3], "j": j[:, :3], "s": s[:, :3], "c": c[:, :3]}


def bits(sim):
    st = state(sim)
    return tuple(st[k].tobytes() for k in ("b", "v", "a", "j", "s", "c"))


def check(d, prec, rec, what):
    """d: distances by quantity; f64: 1e-10 each, f32: 8 x the recorded binary32-storing distance."""
    bound = {q: 1e-10 if prec == "f64" else 8.0 * rec[q] for q in R.QUANTITIES}
    print("%s %s: %s" % (what, prec, "  ".join("%s %.3g (bound %.3g)" % (q, d[q], bound[q]) for q in R.QUANTITIES)))
    bad = {q: (d[q], bound[q]) for q in R.QUANTITIES if not d[q] <= bound[q]}
    assert not bad, bad


# ---- 1. the pass alone, and the pair census -------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(R.SIZES) + list(R.CENSUS))
@pytest.mark.parametrize("prec", PRECS)
def test_start_matches_the_fp64_direct_sum(prec, key):
    """accel, jerk and snap after the start against fp64 direct sums of A, J, S on the stored rows, on |got - ref|_2 / sum |term|_2.
    The census cases carry one body of mass 1e3 -- the last row of the last tile (N = 257), the first row of the second j-chunk
    (N = 4,099): its term is nearly all of every other row's sums, so one missed or doubled pair is an error of order 1."""
    b, v, a, j, s, sc = R.pass_ref(key)
    n = len(b)
    with h6(n, prec) as sim:
        assert sim.variant.startswith("hermite6_") and sim.hermite_order() == 6
        sh = sim.shape_info()
        assert sh["jsplit"] * sh["j_per_split"] >= n and sh["j_per_split"] % 256 == 0, sh
        if n == 4099:
            assert sh["jsplit"] == 2 and sh["j_per_split"] == R.CENSUS["chunk"][1], sh      # a second j-chunk, starting at the census row
        sim.init(b, v)
        sim.set_params(R.H, R.G_PASS)
        st = state(sim)
    assert not st["c"].any()                                                                # crackle == 0 after a start
    assert st["b"].tobytes() == b.astype(sim.dtype).tobytes() and st["v"].tobytes() == v.astype(sim.dtype).tobytes()
    err = {"a": R.row_err(st["a"], a, sc[0]), "j": R.row_err(st["j"], j, sc[1]), "s": R.row_err(st["s"], s, sc[2])}
    rec = R.record()["pass"][str(key)]
    bound = {q: 1e-12 if prec == "f64" else 8.0 * rec[q] for q in err}
    print("start %s %s: %s" % (prec, key, "  ".join("%s %.3g (bound %.3g)" % (q, err[q], bound[q]) for q in err)))
    assert all(err[q] <= bound[q] for q in err), (err, bound)
    if key in R.CENSUS:       # the heavy body's term alone is far above the bound in every other row: a missed pair cannot hide
        row = R.CENSUS[key][1]
        x = np.asarray(b, np.float64)
        d = x[row, :3] - np.delete(x[:, :3], row, 0)
        d2 = (d * d).sum(1)
        share = (R.G_PASS * 1e3 * np.sqrt(d2) / (d2 + R.EPS2) ** 1.5) / np.delete(sc[0], row)
        assert share.min() > 1e3 * max(bound.values()), share.min()


# ---- 2. steps against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.STEPS)
@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("prec", PRECS)
def test_steps_match_the_restatement(prec, n, k):
    ref = R.steps_ref(n)[k]
    b, v = R.system(n)
    with h6(n, prec) as sim:
        sim.init(b, v)
        sim.simulate(k, R.H, 1.0)
        st = state(sim)
    assert np.array_equal(st["b"][:, 3], b[:, 3].astype(sim.dtype)) and not st["v"][:, 3].any()      # the mass lane and vel.w are carried
    check(R.distances(st, ref, R.H), prec, R.record()["steps"][str(n)][str(k)], "N=%d, %d steps" % (n, k))


# ---- 3. determinism and checkpoint ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_bitwise_invariants_and_checkpoint(prec):
    n = 1025
    b0, v0 = R.system(n)
    with h6(n, prec) as one, h6(n, prec) as two:
        for s in (one, two):
            s.init(b0, v0)
            s.set_params(R.H, 1.0)
        one.simulate(5)
        for _ in range(5):
            two.step()
        assert bits(one) == bits(two)                        # nb_step(5) == 5 x nb_step(1); two handles, same bits
        before = bits(one)
        one.simulate(3, 0.0)                                 # dt <= 0: a no-op
        assert bits(one) == before
        one.set_params(R.H, 1.0)
        assert one.force_pass(2) > 0.0                       # the force+jerk+snap pass into scratch
        assert bits(one) == before
        # checkpoint: read + read_jerk + read_snap -> a fresh handle: init, set_params, set_hermite_order(6), upload_derivs6
        st = state(one)
        assert st["c"].any()                                 # c != 0 crosses the restore
        cb, cv, ca = one.read()
        cj = one.read_jerk()
        cs, cc = one.read_snap()
        one.simulate(3)
        with Simulation(n, precision=prec, integrator="hermite4") as fresh:
            fresh.init(cb, cv)
            fresh.set_params(R.H, 1.0)
            fresh.set_hermite_order(6)
            fresh.upload_derivs6(ca, cj, cs, cc)
            fresh.simulate(3)
            assert bits(fresh) == bits(one)


# ---- 4. dt and G changes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_dt_may_change_between_steps(prec):
    n = 257
    b, v = R.system(n)
    ref = R.run(b, v, 1.0, R.DT_SEQUENCE, len(R.DT_SEQUENCE))
    with h6(n, prec) as sim:
        sim.init(b, v)
        for h in R.DT_SEQUENCE:
            sim.step(h, 1.0)
        st = state(sim)
    check(R.distances(st, ref, min(R.DT_SEQUENCE)), prec, R.record()["dt_sequence"], "N=%d, steps %s" % (n, R.DT_SEQUENCE))


@pytest.mark.parametrize("prec", PRECS)
def test_a_changed_G_runs_the_start_again(prec):
    n = 257
    b, v = R.system(n)
    with h6(n, prec) as sim, h6(n, prec) as other:
        sim.init(b, v)
        sim.simulate(2, R.H, 1.0)
        assert sim.read_snap()[1].any()
        sim.set_params(R.H, 0.5)
        assert not sim.read_snap()[1].any()                  # crackle reads 0 before the next step
        gb, gv, _ = sim.read()
        other.init(gb, gv)
        other.set_params(R.H, 0.5)
        assert bits(sim) == bits(other)
        sim.step()
        other.step()
        assert bits(sim) == bits(other)


@pytest.mark.parametrize("via", ["read", "read_jerk", "device_ptr"])
@pytest.mark.parametrize("prec", PRECS)
def test_a_changed_G_read_through_accel_or_jerk_still_runs_the_start(prec, via):
    """The calls that refresh (a, j) alone -- read() with accel, read_jerk(), device_ptr("accel") -- must not leave the snap and the
    crackle of the old G behind as current."""
    n = 257
    b, v = R.system(n)
    with h6(n, prec) as sim, h6(n, prec) as other:
        sim.init(b, v)
        sim.simulate(2, R.H, 1.0)
        assert sim.read_snap()[1].any()
        sim.set_params(R.H, 0.5)
        if via == "read":
            sim.read()
        elif via == "read_jerk":
            sim.read_jerk()
        elif via == "device_ptr":
            assert sim.device_ptr("accel") and sim.device_ptr("jerk")
        assert not sim.read_snap()[1].any()                  # crackle reads 0 before the next step
        gb, gv, _ = sim.read(accel=False)
        other.init(gb, gv)
        other.set_params(R.H, 0.5)
        assert bits(sim) == bits(other)
        sim.step()
        other.step()
        assert bits(sim) == bits(other)


@pytest.mark.parametrize("stale", ["upload", "device_ptr_bodies", "device_ptr_vel"])
@pytest.mark.parametrize("prec", PRECS)
def test_a_new_state_read_through_accel_or_jerk_still_runs_the_start(prec, stale):
    """A stepped handle (c != 0) is given a new state -- or hands out a pointer the caller may write through --, then read() and
    read_jerk() refresh (a, j): the next step must start from that state's own snap and crackle 0, as a fresh twin does."""
    n = 1025
    b0, v0 = R.system(n)
    b1, v1 = R.system(n, seed=77)
    with h6(n, prec) as sim, h6(n, prec) as twin:
        sim.init(b0, v0)
        sim.simulate(2, R.H, 1.0)
        assert sim.read_snap()[1].any()
        if stale == "upload":
            sim.init(b1, v1)
        else:
            b1, v1, _ = sim.read()
            assert sim.device_ptr("bodies" if stale == "device_ptr_bodies" else "vel")
        sim.read()                                           # accel: re-evaluates (a, j) only
        sim.read_jerk()
        twin.init(b1, v1)
        twin.set_params(R.H, 1.0)
        sim.step()
        twin.step()
        assert bits(sim) == bits(twin)
    with h6(n, prec) as sim, h6(n, prec) as twin:            # and read_snap straight after the refresh
        sim.init(b0, v0)
        sim.simulate(2, R.H, 1.0)
        sim.init(b1, v1)
        sim.read()
        twin.init(b1, v1)
        twin.set_params(R.H, 1.0)
        assert not sim.read_snap()[1].any() and bits(sim) == bits(twin)


# ---- 5. Kepler --------------------------------------------------------------------------------------------------------------------
def test_kepler_runs_are_the_restatements():
    """e = 0.5, one period, f64, at the three step sizes of tests/test_hermite6_cpu.py: the engine's final state is the restatement's
    to 1e-10, so it inherits the ratios (64.3, 64.9 per halving of dt)."""
    ends = R.kepler_ends(steps=R.KEPLER_STEPS)
    b0, v0 = R.kepler_pair()
    for k in R.KEPLER_STEPS:
        with h6(2, "f64", eps2=R.KEPLER_EPS2) as sim:
            sim.init(b0, v0)
            sim.simulate(k, 2 * np.pi / k, 1.0)
            st = state(sim)
        d = R.distances(st, ends[k], 2 * np.pi / k)
        check(d, "f64", None, "Kepler %d steps" % k)          # the whole state: x, v, a, j, s, c, the step test's f64 bounds


# ---- 6. order switching -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_order_6_to_4_continues_as_an_order_4_handle(prec):
    n = 1025
    b0, v0 = R.system(n)
    h4 = lambda: Simulation(n, precision=prec, integrator="hermite4")
    with h6(n, prec) as sim, h4() as four, h4() as plain, h4() as set4:
        sim.init(b0, v0)
        sim.simulate(2, R.H, 1.0)
        b, v, a = sim.read()
        j = sim.read_jerk()
        sim.set_hermite_order(4)                             # (a, j) stay current
        assert sim.hermite_order() == 4 and sim.variant.startswith("hermite4_")
        sim.simulate(2)
        four.init(b, v)
        four.upload_derivs(a, j)
        four.simulate(2, R.H, 1.0)
        assert four.variant == sim.variant and four.shape_info() == sim.shape_info()
        get = lambda s: tuple(x.tobytes() for x in s.read()) + (s.read_jerk().tobytes(),)
        assert get(sim) == get(four)
        # a handle that never called the setter next to one that called set_hermite_order(4)
        set4.set_hermite_order(4)
        for s in (plain, set4):
            s.init(b0, v0)
            s.simulate(3, R.H, 1.0)
        assert get(plain) == get(set4) and plain.variant == set4.variant and plain.hermite_order() == 4


# ---- 7. queries behind a stepped handle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_queries_behind_a_stepped_handle_equal_a_fresh_twin(prec):
    n = 1025
    b0, v0 = R.system(n)
    lists = np.random.default_rng(4).integers(0, n, (n, 24)).astype(np.uint32)
    with h6(n, prec) as sim, h6(n, prec) as twin:
        sim.init(b0, v0)
        sim.simulate(3, R.H, 1.0)
        b, v, _ = sim.read()
        twin.init(b, v)
        twin.set_params(R.H, 1.0)
        out = []
        for s in (sim, twin):
            idx, d2, cnt = s.neighbors(bodies=(0, n), radius=0.3)
            fa, fp = s.field(bodies=(0, n))
            la, lj, _ = s.list_force(lists, bodies=(0, n), jerk=True)
            out.append(tuple(z.tobytes() for z in (idx, d2, cnt, fa, fp, la, lj)))
        assert out[0] == out[1]
        assert cnt.any() and np.abs(lj).max() > 0


# ---- 8. other calls and the errors ------------------------------------------------------------------------------------------------
def raises(code, fn, *words):
    with pytest.raises(capi.NBodyError) as e:
        fn()
    assert e.value.code == code, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_other_calls_and_state_errors():
    n = 257
    b, v = R.system(n)
    z = np.zeros((n, 4), np.float32)
    with h6(n, "f32") as sim:
        sim.init(b, v)
        sim.set_params(R.H, 1.0)
        sim.enable_timing(True)
        sim.simulate(3)
        t = sim.step_breakdown()
        assert t["launches"] == 3 and t["force_ms"] > 0 and t["integrate_ms"] > 0 and t["span_ms"] >= t["force_ms"], t
        sim.enable_timing(False)
        assert sim.device_ptr("accel") and sim.device_ptr("jerk")
        raises(1, lambda: sim.set_hermite_order(5), "nb_set_hermite_order", "order")
        raises(4, lambda: sim.set_block_steps(eta=0.02), "nb_set_block_steps", "nb_set_hermite_order")
        raises(4, lambda: sim.set_neighbor_scheme(radius=0.2), "nb_set_neighbor_scheme", "nb_set_hermite_order")
        sim.set_block_steps(None)                            # NULL stays what it was: nothing to switch off
        sim.set_neighbor_scheme(None)
        raises(4, lambda: sim.upload_derivs(z, z), "nb_upload_derivs", "nb_upload_derivs6")
        before = bits(sim)
        sim.set_hermite_order(6)                             # already 6: nothing goes stale
        assert bits(sim) == before and before[5] != z[:, :3].tobytes()
    with Simulation(n, integrator="hermite4") as four:
        four.init(b, v)
        four.set_params(R.H, 1.0)
        raises(4, four.read_snap, "nb_download_snap", "order")
        raises(4, lambda: four.upload_derivs6(z, z, z, z), "nb_upload_derivs6", "order")
        four.set_block_steps(eta=0.02)
        raises(4, lambda: four.set_hermite_order(6), "nb_set_hermite_order", "nb_set_block_steps")
        four.set_block_steps(None)
        four.set_neighbor_scheme(radius=0.2)
        raises(4, lambda: four.set_hermite_order(6), "nb_set_hermite_order", "nb_set_neighbor_scheme")
        four.set_neighbor_scheme(None)
        four.set_hermite_order(6)
        assert four.hermite_order() == 6 and not four.read_snap()[1].any()
    with Simulation(n) as lf:
        lf.init(b, v)
        lf.set_params(R.H, 1.0)
        for fn, name in ((lambda: lf.set_hermite_order(6), "nb_set_hermite_order"), (lf.hermite_order, "nb_hermite_order"),
                         (lf.read_snap, "nb_download_snap"), (lambda: lf.upload_derivs6(z, z, z, z), "nb_upload_derivs6")):
            raises(4, fn, name, "Hermite handle")
