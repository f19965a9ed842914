"""The guarded sums of the mixed-precision force+jerk pass (Simulation.set_pass_guard(r_near) on a handle with
set_pass_precision("mixed")) on the GPU, against the fp64 direct sum, with the bounds recorded in tests/golden/guard.json by the
numpy restatement (tests/guard_ref.py).  The sizes are test_mixed_gpu.py's: 300 (less than one tile), 1,025 (a second workgroup of
one row), 4,099 (two j-chunks with a ragged tile).  What the guard is for is the barycentre rows of the hard pairs: with today's
binary32 sums they miss every bound here by at least a factor of four (test_guard_cpu.py)."""
import numpy as np
import pytest

from nbody3d_amd import Simulation, capi, ic

import block_ref as R
import guard_ref as Gd
import mixed_ref as M
from block_ref import norm_err
from block6_ref import frozen_levels

pytestmark = pytest.mark.gpu

H = Gd.H
R0, R1, R2 = Gd.R_NEARS


def handle(n, r_near=None, mixed=True, prec="f64", **kw):
    sim = Simulation(n, precision=prec, integrator="hermite4", **kw)
    if mixed:
        sim.set_pass_precision("mixed")
    if r_near is not None:
        sim.set_pass_guard(r_near)
    return sim


def bits(sim):
    return tuple(x.tobytes() for x in sim.read()) + (sim.read_jerk().tobytes(),)


def raises(code, fn, *words):
    with pytest.raises(capi.NBodyError) as e:
        fn()
    assert e.value.code == code, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))


# ---- 1. a guard that holds no pair is plain NB_PASS_MIXED, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("n", M.SIZES)
def test_a_guard_of_the_softening_length_is_the_plain_mixed_pass(n):
    b, v = M.pass_system("hard", n)
    with handle(n, np.sqrt(1e-8), eps2=1e-8) as sim, handle(n, eps2=1e-8) as plain:
        for s in (sim, plain):
            s.init(b, v)
            s.set_params(H, 1.0)
        assert sim.variant.startswith("hermite4_f64mxg_") and plain.variant.startswith("hermite4_f64mx_")
        assert sim.shape_info()["jsplit"] == plain.shape_info()["jsplit"]
        assert bits(sim) == bits(plain)                    # the start
        before = bits(sim)
        assert sim.force_pass(1) > 0 and bits(sim) == before
        sim.simulate(5)
        plain.simulate(5)
        assert bits(sim) == bits(plain)


@pytest.mark.parametrize("n,frozen", [(4099, False), (70000, True)])
def test_block_steps_with_an_empty_guard_are_the_plain_mixed_ones(n, frozen):
    """The gathered passes and the fold of their fp64 chunk rows (nb_mxg_fold, from 17 j-chunks on): 4,099 bodies with dynamic levels
    are 17 chunks for a small active set, one ragged batch; 70,000 bodies with 64 of them at level 2 are 274 chunks, two batches."""
    if frozen:
        b, v = [np.array(z, np.float64) for z in ic.plummer(n, seed=1)]
        eps2, dt, blk = 1e-4, 2.0 ** -8, dict(max_level=2, frozen=True)
        lev = np.zeros(n, np.uint8)
        lev[np.random.default_rng(5).choice(n, 64, replace=False)] = 2
    else:
        b, v = M.pass_system("hard", n)
        eps2, dt, blk = 1e-8, 2.0 ** -6, dict(eta=0.02, max_level=12)
    with handle(n, np.sqrt(eps2), eps2=eps2) as sim, handle(n, eps2=eps2) as plain:
        for s in (sim, plain):
            s.init(b, v)
            s.set_params(dt, 1.0)
            s.set_block_steps(**blk)
            if frozen:
                s.upload_levels(lev)
            s.simulate(1)
        st = sim.block_stats()
        assert st == plain.block_stats() and st["block_steps"] > 1, st
        assert bits(sim) == bits(plain)
        assert np.array_equal(sim.read_levels(), plain.read_levels())


# ---- 2, 3. the four figures against the fp64 sum -------------------------------------------------------------------------------
def four_bounds(kind, n, r_near):
    b, v, ra, rj = M.pass_ref(kind, n)
    with handle(n, r_near, eps2=M.KINDS[kind]) as sim:
        sim.init(b, v)
        sim.set_params(H, 1.0)
        a, j = sim.read()[2], sim.read_jerk()
        assert sim.pass_guard() == r_near and sim.variant.startswith("hermite4_f64mxg_")
    got, rec = Gd.four(a, j, ra, rj, b), Gd.pass_record(kind, n)[Gd.key(r_near)]
    print("guarded pass %s N=%d r_near=%g: %s" % (kind, n, r_near, ", ".join("%s %.3g (restatement %.3g)" % (q, got[q], rec[q]) for q in Gd.QUANTITIES)))
    assert a.dtype == np.float64 and not a[:, 3].any() and not j[:, 3].any()
    for q in Gd.QUANTITIES:
        assert got[q] <= M.FACTOR * rec[q], (q, got, rec)


@pytest.mark.parametrize("n", M.SIZES)
@pytest.mark.parametrize("kind", M.HARD_KINDS)
def test_pair_and_barycentre_rows_against_the_fp64_sum(kind, n):
    four_bounds(kind, n, R0)


@pytest.mark.parametrize("kind", M.HARD_KINDS)
def test_a_third_body_in_the_near_set(kind):
    four_bounds(kind, 4099, R1)


@pytest.mark.parametrize("n", [300, 1025])
@pytest.mark.parametrize("kind", M.HARD_KINDS)
def test_every_term_compensated(kind, n):
    """r_near = 1e3: every stage of every wave takes the slow sums, every row has n near terms."""
    four_bounds(kind, n, R2)


# ---- 4. no pairs: the guard costs nothing in accuracy --------------------------------------------------------------------------
@pytest.mark.parametrize("n", M.SIZES)
def test_plummer_keeps_its_accuracy(n):
    b, v, ra, rj = M.pass_ref("plummer", n)
    rec = next(r for r in Gd.record()["plummer"] if r["n"] == n)
    with handle(n, R0, eps2=M.KINDS["plummer"]) as sim:
        sim.init(b, v)
        sim.set_params(H, 1.0)
        a, j = sim.read()[2], sim.read_jerk()
    ea, ej = norm_err(a[:, :3], ra), norm_err(j[:, :3], rj)
    print("guarded pass plummer N=%d: a %.3g (restatement %.3g), j %.3g (restatement %.3g)" % (n, ea, rec["a"], ej, rec["j"]))
    assert ea <= M.FACTOR * rec["a"] and ej <= M.FACTOR * rec["j"], (ea, ej, rec)


# ---- 5, 6. shared steps and state ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", Gd.STEPS_SIZES)
def test_shared_steps_and_state(n):
    """Five shared steps against the fp64 scheme's, within FACTOR x the distance the guarded restatement has from it (guard.json);
    step(5) is 5 x step(1), two handles agree bit for bit, the getter returns what was set."""
    b0, v0, (rb, rv, _, _) = Gd.steps_ref(n)
    rec = next(r for r in Gd.record()["steps"] if r["n"] == n)
    with handle(n, R0, eps2=1e-8) as sim, handle(n, R0, eps2=1e-8) as one, handle(n, R0, eps2=1e-8) as twin:
        for s in (sim, one, twin):
            s.init(b0, v0)
        sim.simulate(5, H, 1.0)
        twin.simulate(5, H, 1.0)
        one.set_params(H, 1.0)
        for _ in range(5):
            one.simulate(1)
        b, v, _ = sim.read()
        ex, ev = norm_err(b[:, :3], rb[:, :3]), norm_err(v[:, :3], rv[:, :3])
        print("guarded shared steps N=%d: positions %.3g (restatement %.3g), velocities %.3g (restatement %.3g)" % (n, ex, rec["x"], ev, rec["v"]))
        assert ex <= M.FACTOR * rec["x"] and ev <= M.FACTOR * rec["v"], (ex, ev, rec)
        assert bits(sim) == bits(one) == bits(twin)
        assert b[:, 3].tobytes() == b0[:, 3].tobytes()
        assert sim.pass_guard() == R0 and sim.pass_precision() == "mixed"
        sim.set_pass_guard(0.25)
        assert sim.pass_guard() == 0.25
        sim.set_pass_guard(0)
        assert sim.pass_guard() == 0.0 and sim.variant.startswith("hermite4_f64mx_")


def test_native_again_drops_the_guard():
    n = 1025
    b, v = M.pass_system("hard", n)
    with handle(n, mixed=False, eps2=1e-8) as plain, handle(n, R0, eps2=1e-8) as back:
        for sim in (plain, back):
            sim.init(b, v)
            sim.set_params(H, 1.0)
        guarded = bits(back)
        back.set_pass_precision("native")
        assert back.pass_guard() == 0.0 and plain.pass_guard() == 0.0 and back.variant == plain.variant
        assert bits(back) == guarded                       # the setters mark nothing stale
        back.init(b, v)
        assert bits(back) == bits(plain) != guarded        # the native pass in the grown buffer: the bits of a handle that never had a guard
        plain.simulate(3)
        back.simulate(3)
        assert bits(back) == bits(plain)
        back.set_pass_precision("mixed")
        assert back.pass_guard() == 0.0                    # ... and a new mixed mode starts without one


# ---- 7. checkpoints ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setter_first", [True, False])
@pytest.mark.parametrize("blocks", [False, True])
def test_a_checkpoint_continues_bit_for_bit(blocks, setter_first):
    n = 1025
    b0, v0 = M.pass_system("hard", n)
    lev = frozen_levels(n)
    blk = dict(max_level=3, frozen=True)
    with handle(n, R0, eps2=1e-8) as sim, handle(n, eps2=1e-8) as fresh:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -6, 1.0)
        if blocks:
            sim.set_block_steps(**blk)
            sim.upload_levels(lev)
        sim.simulate(3)
        b, v, a = sim.read()
        j = sim.read_jerk()
        fresh.init(b, v)
        if setter_first:
            fresh.set_pass_guard(R0)
        fresh.upload_derivs(a, j)
        if not setter_first:
            fresh.set_pass_guard(R0)
        fresh.set_params(2.0 ** -6, 1.0)
        if blocks:
            fresh.set_block_steps(**blk)
            fresh.upload_levels(sim.read_levels())
        assert bits(fresh) == bits(sim)
        sim.simulate(3)
        fresh.simulate(3)
        assert bits(fresh) == bits(sim)


# ---- 8. block steps, dynamic levels --------------------------------------------------------------------------------------------
def test_dynamic_levels_with_a_guard():
    """mixed_ref.BLOCK with the guard at 0.01, against the restatement with the guarded sum (guard.json): its block steps exactly;
    body steps within the spread mixed.json shows between the orders of its sums (a property of the schedule's sensitivity to the
    last bits of the pass, which the device's v_rsq_f32 moves as a sum order does); |dE/E0| at most twice the record."""
    k, ref = M.BLOCK, Gd.record()["block"][Gd.key(R0)]
    orders = [M.record()["block"]["mixed_" + a]["body_steps"] for a in M.ACCS]
    spread = max(orders) - min(orders)
    b0, v0 = M.block_system()
    e0 = R.energy(b0, v0, 1.0, k["eps2"])
    with handle(k["n"], R0, eps2=k["eps2"]) as sim:
        sim.init(b0, v0)
        sim.set_params(k["dt"], 1.0)
        sim.set_block_steps(eta=k["eta"], max_level=k["max_level"])
        sim.simulate(k["outer"])
        b, v, _ = sim.read()
        st, de = sim.block_stats(), abs((R.energy(b, v, 1.0, k["eps2"]) - e0) / e0)
    print("guarded dynamic levels: %s, |dE/E0| %.3g; restatement %s; spread of body steps %d" % (st, de, ref, spread))
    assert st["block_steps"] == ref["block_steps"], (st, ref)
    assert abs(st["body_steps"] - ref["body_steps"]) <= spread, (st, ref, spread)
    assert st["clamped"] == 0 and st["outer_steps"] == k["outer"], st
    assert de <= 2 * ref["dE"], (de, ref["dE"])


# ---- 9. the errors -------------------------------------------------------------------------------------------------------------
def test_errors_on_device_handles():
    n = 300
    b, v = ic.plummer(n, seed=21)

    def still_works(sim):
        sim.simulate(1)
        assert np.isfinite(sim.read()[0]).all()

    with handle(n, mixed=False) as native:
        native.init(b, v)
        native.set_params(H, 1.0)
        raises(4, lambda: native.set_pass_guard(0.01), "nb_set_pass_guard", "nb_set_pass_precision", "NB_PASS_NATIVE")
        assert native.pass_guard() == 0.0
        still_works(native)
    with handle(n, mixed=False, prec="f32") as f32:
        f32.init(b, v)
        f32.set_params(H, 1.0)
        raises(4, lambda: f32.set_pass_guard(0.01), "nb_set_pass_guard", "nb_set_pass_precision", "NB_F32")
        assert f32.pass_guard() == 0.0
        still_works(f32)
    with Simulation(n, precision="f64") as lf:
        lf.init(b, v)
        lf.set_params(H, 1.0)
        raises(4, lambda: lf.set_pass_guard(0.01), "nb_set_pass_guard", "nb_set_pass_precision", "Hermite handle")
        raises(4, lf.pass_guard, "nb_pass_guard", "Hermite handle")
        still_works(lf)
    with handle(n, mixed=False) as six:
        six.init(b, v)
        six.set_params(H, 1.0)
        six.set_hermite_order(6)
        raises(4, lambda: six.set_pass_guard(0.01), "nb_set_pass_guard", "nb_set_pass_precision", "order")
        assert six.pass_guard() == 0.0
        still_works(six)
    with handle(n, 0.01) as mx:
        mx.init(b, v)
        mx.set_params(H, 1.0)
        for bad in (-1.0, float("nan"), float("inf")):
            raises(1, lambda: mx.set_pass_guard(bad), "nb_set_pass_guard", "r_near")
        assert mx.pass_guard() == 0.01
        raises(1, lambda: mx.set_pass_precision(2), "nb_set_pass_precision", "mode")
        raises(4, lambda: mx.set_hermite_order(6), "nb_set_hermite_order", "NB_PASS_MIXED")
        still_works(mx)
