"""The start of its own of order-6 handles (Simulation.set_start6) on the GPU, against the restatement in tests/start6_ref.py: the
crackle pass against an fp64 direct sum (sizes 2, 3, 257, 1,025, 4,099 and the two census cases of hermite6_ref), the state bits
(a, j, s shared with the default start, steps against the restatement, step batching, two handles, the six-array checkpoint, a changed
G, the setter before and after steps), the two-rule start levels exactly on the small dynamic systems and on the 1,024-body
hard-pair fixture with its first outer step, frozen and uploaded levels, and the errors.  f64 bounds are the project's (1e-12 on the
row metric, 1e-10 on states); f32 bounds are 8 x the binary32-storing restatement's own figures (tests/golden/start6.json)."""
import numpy as np
import pytest

from nbody3d_amd import Simulation, capi

import block6_ref as B6
import block_ref as B
import hermite6_ref as H6
import start6_ref as R

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
    bound = {q: 1e-10 if prec == "f64" else R.FACTOR * rec[q] for q in R.QUANTITIES}
    print("%s %s: %s" % (what, prec, "  ".join("%s %.3g (bound %.3g)" % (q, d[q], bound[q]) for q in R.QUANTITIES)))
    bad = {q: (d[q], bound[q]) for q in R.QUANTITIES if not d[q] <= bound[q]}
    assert not bad, bad


# ---- 1. the crackle pass alone, and the pair census -----------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(R.SIZES) + list(R.CENSUS))
@pytest.mark.parametrize("prec", PRECS)
def test_crackle_matches_the_fp64_direct_sum(prec, key):
    """read_snap()[1] after set_start6(1) against the fp64 direct sum on the stored rows, on |got - ref|_2 / sum |term|_2; a, j and s
    keep the default start's bits.  The census cases carry one body of mass 1e3 (the last row of the last tile at N = 257, the first
    row of the second j-chunk at N = 4,099): its term is nearly all of every other row's sum, so one missed or doubled pair fails."""
    b, v, a, j, c, sc = R.pass_ref(key)
    n = len(b)
    with h6(n, prec) as sim:
        sim.init(b, v)
        sim.set_params(R.H, R.G_PASS)
        assert sim.start6 == capi.START6_ZERO
        before = state(sim)
        assert not before["c"].any()
        sim.set_start6(capi.START6_CRACKLE)              # drops the start no step has consumed
        assert sim.start6 == capi.START6_CRACKLE
        st = state(sim)
        if n == 4099:
            sh = sim.shape_info()
            assert sh["jsplit"] == 2 and sh["j_per_split"] == R.CENSUS["chunk"][1], sh
    for q in ("b", "v", "a", "j", "s"):
        assert st[q].tobytes() == before[q].tobytes(), q
    err = H6.row_err(st["c"], c, sc)
    bound = 1e-12 if prec == "f64" else R.FACTOR * R.record()["pass"][str(key)]["c"]
    print("crackle %s %s: %.3g (bound %.3g)" % (prec, key, err, bound))
    assert err <= bound, (err, bound)
    if key in R.CENSUS:       # the heavy body's term alone is above the bound in every other row: a missed pair cannot hide
        row = R.CENSUS[key][1]
        light = np.array(b, np.float64)
        light[row, 3] = 0.0
        d = np.delete(c - R.crk(light, v, a, j, R.G_PASS), row, 0)
        share = np.sqrt((d * d).sum(1)) / np.delete(sc, row)
        # a row that misses (or doubles) the heavy pair is off by its share, less what the row is off by anyway (<= bound): with
        # share > 10 x bound that is >= 9 x bound.  (The crackle's term changes sign along an orbit, so unlike the acceleration's
        # its share is small in a few rows: 4e-3 at the least here, nearly 1 in most.)
        print("census %s: smallest share of the heavy body's term %.3g, median %.3g" % (key, share.min(), np.median(share)))
        assert share.min() > 10 * bound, share.min()


# ---- 2. steps from the new start -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("prec", PRECS)
def test_steps_from_the_new_start_match_the_restatement(prec, n):
    """1, 2 and 5 shared steps against the restatement; nb_step(5) equals 5 x nb_step(1); two handles agree."""
    ref = R.steps_ref(n)
    b, v = H6.system(n)
    with h6(n, prec) as one, h6(n, prec) as two:
        for s in (one, two):
            s.init(b, v)
            s.set_start6(1)
            s.set_params(R.H, 1.0)
        done = 0
        for k in R.STEPS:
            for _ in range(k - done):
                one.step()
            done = k
            check(H6.distances(state(one), ref[k], R.H), prec, R.record()["steps"][str(n)][str(k)], "N=%d, %d steps" % (n, k))
        two.simulate(max(R.STEPS))
        assert bits(one) == bits(two)


# ---- 3. checkpoint, G, the setter ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_checkpoint_changed_G_and_the_setter(prec):
    n = 1025
    b0, v0 = H6.system(n)
    with h6(n, prec) as one, h6(n, prec) as twin, Simulation(n, precision=prec, integrator="hermite4") as fresh:
        for s in (one, twin):
            s.init(b0, v0)
            s.set_params(R.H, 1.0)
        one.set_start6(1)
        # a six-array checkpoint of the start itself (c != 0, no step yet) into a handle in the default mode: kept as uploaded
        cb, cv, ca = one.read()
        cj = one.read_jerk()
        cs, cc = one.read_snap()
        assert cc.any()
        fresh.init(cb, cv)
        fresh.set_params(R.H, 1.0)
        fresh.set_hermite_order(6)
        fresh.upload_derivs6(ca, cj, cs, cc)
        assert bits(fresh) == bits(one)
        fresh.set_start6(1)                                  # an uploaded start is not the engine's: the setter keeps it
        fresh.set_start6(0)
        assert bits(fresh) == bits(one)
        one.simulate(3)
        fresh.simulate(3)
        assert bits(fresh) == bits(one)
        # the setter on a stepped handle: the run continues as the twin's
        twin.simulate(2)
        one.set_start6(0)
        one.init(b0, v0)                                     # (a new upload: the next start is made in the mode in force, ZERO)
        one.simulate(2)
        assert bits(one) == bits(twin)
        one.set_start6(1)
        assert one.start6 == 1 and bits(one) == bits(twin)   # nothing of the running state changed
        one.simulate(2)
        twin.simulate(2)
        assert bits(one) == bits(twin)
        # a changed G remakes the exact c: as a fresh handle in the mode from the same (x, v)
        one.set_params(R.H, 0.5)
        gb, gv, _ = one.read(accel=False)
        c_new = one.read_snap()[1]
        assert c_new.any()
        twin.set_start6(1)
        twin.init(gb, gv)
        twin.set_params(R.H, 0.5)
        assert bits(one) == bits(twin)
        one.step()
        twin.step()
        assert bits(one) == bits(twin)
        # order 4 returns the mode to ZERO
        one.set_hermite_order(4)
        one.set_hermite_order(6)
        assert one.start6 == 0 and not one.read_snap()[1].any()


# ---- 4. block steps: the two-rule start ------------------------------------------------------------------------------------------
def start_levels_of(b0, v0, eps2, dt, eta, L):
    """(default-mode levels, levels after set_start6(1)) of one handle: the setter drops levels the engine chose itself."""
    with h6(len(b0), "f64", eps2=eps2) as sim:
        sim.init(b0, v0)
        sim.set_params(dt, 1.0)
        sim.set_block_steps6(eta=eta, max_level=L)
        zero = sim.read_levels()
        sim.set_start6(1)
        new = sim.read_levels()
        assert sim.block_stats()["clamped"] == 0
    return zero, new


def zero_levels(b0, v0, eps2, dt, eta, L):
    st = H6.start(b0, v0, 1.0, eps2)
    return B.start_levels(st["a"], st["j"], dt, eta, 0, L, {"clamped": 0}).astype(np.uint8)


@pytest.mark.parametrize("n,seed", B6.TINY)
def test_start_levels_on_tiny_systems_are_the_restatements(n, seed):
    b0, v0, lev, margin = R.tiny_start(n, seed)
    p = B6.TINY_RUN
    zero, new = start_levels_of(b0, v0, R.EPS2, p["dt"], p["eta"], p["max_level"])
    print("N=%d: margin %.3g, default %s, two-rule %s" % (n, margin, zero.tolist(), new.tolist()))
    assert np.array_equal(new, lev), (new, lev)
    assert np.array_equal(zero, zero_levels(b0, v0, R.EPS2, p["dt"], p["eta"], p["max_level"]))      # the default mode's levels are unchanged


def test_start_levels_on_300_bodies_with_a_tight_pair_are_the_restatements():
    b0, v0, lev, margin = R.pair300_start()
    p = B6.PAIR300
    zero, new = start_levels_of(b0, v0, R.EPS2, p["dt"], p["eta"], p["max_level"])
    print("N=300: margin %.3g, default %s, two-rule %s" % (margin, np.bincount(zero).tolist(), np.bincount(new).tolist()))
    assert np.array_equal(new, lev), np.nonzero(new != lev)[0]
    assert np.array_equal(zero, zero_levels(b0, v0, R.EPS2, p["dt"], p["eta"], p["max_level"]))


def test_first_outer_step_of_the_hard_pair_fixture():
    """Start levels exactly, one outer step with the restatement's block and body step counts, the state within 1e-10."""
    b0, v0, (ref, rl, rs, lev0), rde, margin = R.hard_ref()
    p = R.HARD
    with h6(p["n"], "f64", eps2=p["eps2"]) as sim:
        sim.init(b0, v0)
        sim.set_start6(1)
        sim.set_params(p["dt"], 1.0)
        sim.set_block_steps6(eta=p["eta"], max_level=p["max_level"])
        got0 = sim.read_levels()
        assert np.array_equal(got0, lev0), np.nonzero(got0 != lev0)[0]
        k0, p0, _ = sim.diagnostics()
        sim.block_stats(reset=True)
        sim.simulate(p["outer"])
        k1, p1, _ = sim.diagnostics()
        st, stats, lev = state(sim), sim.block_stats(), sim.read_levels()
    de = abs((k1 + p1 - k0 - p0) / (k0 + p0))
    d = B6.distances(st, ref, p["dt"], p["max_level"])
    print("hard pairs: margin %.3g, |dE/E0| %.3g (restatement %.3g), %s (restatement %s), %s" % (margin, de, rde, stats, rs, d))
    for k in ("block_steps", "body_steps", "outer_steps"):
        assert stats[k] == rs[k], (k, stats, rs)
    assert stats["clamped"] == 0
    assert all(d[q] <= 1e-10 for q in R.QUANTITIES), d


@pytest.mark.parametrize("prec", PRECS)
def test_frozen_and_uploaded_levels_are_untouched_by_the_mode(prec):
    n = 300
    b0, v0 = R.pair300_start()[:2]
    lev = B6.frozen_levels(n)
    got = []
    for mode in (0, 1):
        with h6(n, prec) as sim:
            sim.init(b0, v0)
            sim.set_start6(mode)
            sim.set_params(2.0 ** -4, 1.0)
            sim.set_block_steps6(max_level=3, min_level=1, frozen=True)
            assert (sim.read_levels() == 1).all()            # frozen: every body at min_level in either mode
            sim.upload_levels(lev.clip(1, 3))
            sim.set_start6(1 - mode)                         # the setter keeps uploaded levels
            sim.set_start6(mode)
            assert np.array_equal(sim.read_levels(), lev.clip(1, 3))
            c = sim.read_snap()[1]
            assert c.any() == (mode == 1)
            sim.upload_derivs6(sim.read()[2], sim.read_jerk(), sim.read_snap()[0], np.zeros_like(c))      # the same start in both modes
            sim.simulate(1)
            got.append(bits(sim) + (sim.read_levels().tobytes(), str(sim.block_stats())))
    assert got[0] == got[1]


# ---- 5. the errors ---------------------------------------------------------------------------------------------------------------
def raises(code, fn, *words):
    with pytest.raises(capi.NBodyError) as e:
        fn()
    assert e.value.code == code, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_errors():
    n = 257
    b, v = H6.system(n)
    with h6(n, "f32") as sim:
        sim.init(b, v)
        sim.set_params(R.H, 1.0)
        raises(1, lambda: sim.set_start6(2), "nb_set_start6", "mode")
        assert sim.start6 == 0
    with Simulation(n, integrator="hermite4") as four:
        four.init(b, v)
        four.set_params(R.H, 1.0)
        raises(4, lambda: four.set_start6(1), "nb_set_start6", "order")
        raises(4, lambda: four.start6, "nb_start6", "order")
    with Simulation(n) as lf:
        lf.init(b, v)
        lf.set_params(R.H, 1.0)
        raises(4, lambda: lf.set_start6(1), "nb_set_start6", "Hermite handle")
        raises(4, lambda: lf.start6, "nb_start6", "Hermite handle")
