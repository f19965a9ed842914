"""The mixed-precision force+jerk pass of f64 Hermite handles (Simulation.set_pass_precision("mixed")) on the GPU, against the fp64
direct sum and the numpy restatement of its arithmetic (tests/mixed_ref.py), with the bounds recorded in tests/golden/mixed.json.
The sizes are the smallest at which the kernel can go wrong: 300 (less than one tile, one ragged workgroup), 1,025 (a second
workgroup of one row, the tile tail), 4,099 (two j-chunks, ragged last tile and last workgroup).  The hard inputs hold pairs
2e-3 and 2e-4 apart, built in float64 and not rounded to float32, unshifted and shifted by (3, -2, 1): on the shifted ones a
dropped or mis-staged lo stream fails the pair rows' bound by a factor of at least four (test_mixed_cpu.py).  One case at
N = 65,536 covers the partial sums the setter has to grow."""
import numpy as np
import pytest

from nbody3d_amd import Simulation, capi, ic

import block_ref as R
import mixed_ref as M
from block_ref import norm_err
from block6_ref import frozen_levels

pytestmark = pytest.mark.gpu

H = 2.0 ** -7


def handle(n, mixed=True, prec="f64", **kw):
    sim = Simulation(n, precision=prec, integrator="hermite4", **kw)
    if mixed:
        sim.set_pass_precision("mixed")
    return sim


def bits(sim):
    return tuple(x.tobytes() for x in sim.read()) + (sim.read_jerk().tobytes(),)


def raises(code, fn, *words):
    with pytest.raises(capi.NBodyError) as e:
        fn()
    assert e.value.code == code, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))


# ---- 1. the pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", M.SIZES)
@pytest.mark.parametrize("kind", list(M.KINDS))
def test_the_pass_against_the_fp64_sum(kind, n):
    b, v, ra, rj = M.pass_ref(kind, n)
    with handle(n, eps2=M.KINDS[kind]) as sim:
        sim.init(b, v)
        sim.set_params(H, 1.0)
        a = sim.read()[2]
        j = sim.read_jerk()
        name, shape, mode = sim.variant, sim.shape_info(), sim.pass_precision()
    ea, ej = norm_err(a[:, :3], ra), norm_err(j[:, :3], rj)
    print("mixed pass %s N=%d (%s): a %.3g, j %.3g" % (kind, n, name, ea, ej))
    assert name.startswith("hermite4_f64mx_") and mode == "mixed"
    assert shape["jsplit"] == (2 if n == 4099 else 1), shape           # kFjMinChunk: two j-chunks from 4,096 bodies on
    assert a.dtype == np.float64 and not a[:, 3].any() and not j[:, 3].any()
    assert ea <= 2e-5 and ej <= 2e-5, (ea, ej)                          # the f32 pass's bound
    if kind in M.HARD_KINDS:
        rec, rows = M.pass_record(kind, n)["lo"], M.pair_rows(kind)
        pa, pj = M.row_err(a, ra, rows), M.row_err(j, rj, rows)
        print("  pair rows: a %.3g (restatement %.3g), j %.3g (restatement %.3g)" % (pa, rec["pair_a"], pj, rec["pair_j"]))
        assert pa <= M.FACTOR * rec["pair_a"] and pj <= M.FACTOR * rec["pair_j"], (pa, pj, rec)


# ---- 2. native is untouched ----------------------------------------------------------------------------------------------------
def test_native_is_untouched():
    n = 1025
    b, v = M.pass_system("hard", n)
    with handle(n, mixed=False, eps2=1e-8) as plain, handle(n, eps2=1e-8) as back:
        for sim in (plain, back):
            sim.init(b, v)
            sim.set_params(H, 1.0)
        mixed_bits = bits(back)
        back.set_pass_precision("native")
        assert back.pass_precision() == "native" and back.variant == plain.variant and plain.variant.startswith("hermite4_f64_")
        assert bits(back) == mixed_bits                    # the setter marks nothing stale: the derivatives stay what they were
        back.init(b, v)                                    # ... and the next pass is the native one
        assert bits(back) == bits(plain) != mixed_bits
        plain.simulate(3)
        back.simulate(3)
        assert bits(back) == bits(plain)


# ---- 3. shared steps -----------------------------------------------------------------------------------------------------------
_steps = {}


def steps_ref(n):
    """(b0, v0, the restatement's 5 steps with the kernel's binary32 sums, its distance to the one with fp64 sums): once per size."""
    if n not in _steps:
        b0, v0 = M.pass_system("hard", n)
        f32, f64 = M.hermite_mixed(b0, v0, 1.0, 1e-8, H, 5), M.hermite_mixed(b0, v0, 1.0, 1e-8, H, 5, acc="fp64")
        _steps[n] = (b0, v0, f32, tuple(max(1e-9, M.FACTOR * norm_err(f32[k][:, :3], f64[k][:, :3])) for k in (0, 1)))
    return _steps[n]


@pytest.mark.parametrize("n", [300, 1025])
def test_shared_steps_follow_the_restatement(n):
    b0, v0, (rb, rv, _, _), (tx, tv) = steps_ref(n)
    with handle(n, eps2=1e-8) as sim, handle(n, eps2=1e-8) as one, handle(n, eps2=1e-8) as twin:
        for s in (sim, one, twin):
            s.init(b0, v0)
        sim.simulate(5, H, 1.0)
        twin.simulate(5, H, 1.0)
        one.set_params(H, 1.0)
        for _ in range(5):
            one.simulate(1)
        b, v, _ = sim.read()
        ex, ev = norm_err(b[:, :3], rb[:, :3]), norm_err(v[:, :3], rv[:, :3])
        print("mixed shared steps N=%d: positions %.3g (bound %.3g), velocities %.3g (bound %.3g)" % (n, ex, tx, ev, tv))
        assert ex <= tx and ev <= tv, (ex, tx, ev, tv)
        assert bits(sim) == bits(one) == bits(twin)
        assert b[:, 3].tobytes() == b0[:, 3].tobytes()


# ---- 4. checkpoints ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setter_first", [True, False])
@pytest.mark.parametrize("blocks", [False, True])
def test_a_checkpoint_continues_bit_for_bit(blocks, setter_first):
    n = 1025
    b0, v0 = M.pass_system("hard", n)
    lev = frozen_levels(n)
    blk = dict(max_level=3, frozen=True)
    with handle(n, eps2=1e-8) as sim, handle(n, mixed=False, eps2=1e-8) as fresh:
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
            fresh.set_pass_precision("mixed")
        fresh.upload_derivs(a, j)
        if not setter_first:
            fresh.set_pass_precision("mixed")
        fresh.set_params(2.0 ** -6, 1.0)
        if blocks:
            fresh.set_block_steps(**blk)
            fresh.upload_levels(sim.read_levels())
        assert bits(fresh) == bits(sim)
        sim.simulate(3)
        fresh.simulate(3)
        assert bits(fresh) == bits(sim)


# ---- 5. block steps, frozen levels ---------------------------------------------------------------------------------------------
def test_frozen_block_steps_follow_the_exact_schedule():
    n = 1025
    b0, v0 = M.pass_system("hard", n)
    lev = frozen_levels(n)
    run = lambda acc: R.block_ref(b0, v0, 1.0, 1e-8, 2.0 ** -6, 1, max_level=3, levels=lev, frozen=True, fj=M.with_acc(acc))
    (rb, rv, _, _, rl, rs), (db, dv, _, _, _, _) = run("f32"), run("fp64")
    tx, tv = [max(1e-9, M.FACTOR * norm_err(p[:, :3], q[:, :3])) for p, q in ((rb, db), (rv, dv))]
    with handle(n, eps2=1e-8) as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** -6, 1.0)
        sim.set_block_steps(max_level=3, frozen=True)
        sim.upload_levels(lev)
        sim.simulate(1)
        b, v, _ = sim.read()
        st, got = sim.block_stats(), sim.read_levels()
    ex, ev = norm_err(b[:, :3], rb[:, :3]), norm_err(v[:, :3], rv[:, :3])
    print("mixed frozen block steps N=%d: %s; positions %.3g (bound %.3g), velocities %.3g (bound %.3g)" % (n, st, ex, tx, ev, tv))
    assert st["block_steps"] == 8 == rs["block_steps"] and st["body_steps"] == rs["body_steps"] and st["outer_steps"] == 1, (st, rs)
    assert st["clamped"] == 0 and st["finest_level"] == 3 and np.array_equal(got, lev) and np.array_equal(rl, lev)
    assert ex <= tx and ev <= tv, (ex, tx, ev, tv)


# ---- 6. block steps, dynamic levels --------------------------------------------------------------------------------------------
def test_dynamic_levels_follow_the_fp64_schedule():
    """BLOCK (512 bodies, four pairs 2e-3 apart, eps2 1e-8, dt 2^-4, max_level 16, eta 0.02, four outer steps) against the fp64
    restatement recorded in mixed.json: block steps within 2 %, body steps within 0.5 %, nothing clamped, |dE/E0| at most twice the
    fp64 figure.  On the CPU (the same record): the double-single restatement with fp64 sums and with three orders of binary32 sums
    has the fp64 run's 2,070 block steps exactly, its 37,242 body steps to 0.035 % and 0.99 - 1.27 x its |dE/E0| of 1.61e-7; a
    binary32-storing handle takes 8,001 block steps (+287 %), +32 % body steps and 56 x the energy error; the hi word alone 32,421
    block steps (+1,466 %), +164 % body steps and 2.6 x the energy error.  The margins are conditions the restatements meet with
    room and both failure modes miss by a wide gap.  The native f64 handle runs the same system beside the mixed one and its figures
    are printed: the energy error of a run of 2,070 block steps through four hard pairs is a property of the trajectory taken, and
    what the engine's own fp64 pass gives on this device says how much of the mixed handle's figure is the pass.  On an MI355X:
    native 2,070 / 37,242 / 1.61e-7, the fp64 restatement's figures exactly; mixed 2,070 / 37,246 / 2.98e-7.  The restatements round
    the reciprocal root correctly; v_rsq_f32 is good to one ulp, and the restatement with its root moved by -1, 0 or +1 ulp at
    random gives 2.96 - 3.06e-7 on four seeds: the engine's figure is that of its arithmetic, 5 - 8 % inside the bound, and it does
    not depend on the device's CU count (512 bodies are one j-chunk, and two for every gathered pass)."""
    k, ref = M.BLOCK, M.record()["block"]["fp64"]
    b0, v0 = M.block_system()
    e0, got = R.energy(b0, v0, 1.0, k["eps2"]), {}
    for mixed in (True, False):
        with handle(k["n"], mixed=mixed, eps2=k["eps2"]) as sim:
            sim.init(b0, v0)
            sim.set_params(k["dt"], 1.0)
            sim.set_block_steps(eta=k["eta"], max_level=k["max_level"])
            sim.simulate(k["outer"])
            b, v, _ = sim.read()
            got[mixed] = (sim.block_stats(), abs((R.energy(b, v, 1.0, k["eps2"]) - e0) / e0))
    (st, de), (nst, nde) = got[True], got[False]
    print("mixed dynamic levels: %s, |dE/E0| %.3g; native f64 handle: %s, |dE/E0| %.3g; fp64 restatement %s" % (st, de, nst, nde, ref))
    assert abs(st["block_steps"] - ref["block_steps"]) <= 0.02 * ref["block_steps"], (st, ref)
    assert abs(st["body_steps"] - ref["body_steps"]) <= 0.005 * ref["body_steps"], (st, ref)
    assert st["clamped"] == 0 and st["outer_steps"] == k["outer"], st
    assert de <= 2 * ref["dE"], (de, ref["dE"])


# ---- 6b. the partial sums grow where the mixed shape needs more of them ------------------------------------------------------
def test_the_partial_sums_grow_for_the_mixed_shape():
    """N = 65,536: the smallest benchmark size at which the mixed pass's chunks x 16-byte rows exceed the native pass's chunks x
    32-byte rows (32 chunks against 8 on 256 CUs), so nb_set_pass_precision reallocates the partial sums.  The mixed pass against the
    native one on every row and against the fp64 direct sum on 64 rows; then back to native: the native pass in the grown buffer
    gives the bits of a handle that never called the setter."""
    n = 65536
    b, v = [np.array(z, np.float64) for z in ic.plummer(n, seed=1)]
    rows = np.linspace(0, n - 1, 64).astype(np.int64)
    ra, rj = R.fj_ref(b, v, 1.0, 1e-4, rows)
    with handle(n, mixed=False) as plain, handle(n) as sim:
        for s in (plain, sim):
            s.init(b, v)
            s.set_params(H, 1.0)
        mc, nc = sim.shape_info()["jsplit"], plain.shape_info()["jsplit"]
        assert 16 * mc > 32 * nc, (mc, nc)                 # the condition under which the setter grew the buffer
        na, nj = plain.read()[2], plain.read_jerk()
        a, j = sim.read()[2], sim.read_jerk()
        ea, ej = norm_err(a[:, :3], na[:, :3]), norm_err(j[:, :3], nj[:, :3])
        sa, sj = norm_err(a[rows, :3], ra), norm_err(j[rows, :3], rj)
        print("mixed pass N=%d, %d chunks (native %d): against the native pass a %.3g, j %.3g; 64 rows against fp64 a %.3g, j %.3g" % (n, mc, nc, ea, ej, sa, sj))
        assert ea <= 2e-5 and ej <= 2e-5 and sa <= 2e-5 and sj <= 2e-5, (ea, ej, sa, sj)
        sim.simulate(2)
        plain.simulate(2)
        # two steps from accelerations that may differ by 2e-5 of their scale: at most (2^-6)^2 / 2 x 2e-5 = 2.4e-9 of max |a| / max |x| < 1
        assert norm_err(sim.read()[0][:, :3], plain.read()[0][:, :3]) <= 2.4e-9
        sim.set_pass_precision("native")
        sim.init(b, v)
        plain.init(b, v)
        assert bits(sim) == bits(plain)


# ---- 7. the errors -------------------------------------------------------------------------------------------------------------
def test_errors_on_device_handles():
    n = 300
    b, v = ic.plummer(n, seed=21)

    def still_works(sim):
        sim.simulate(1)
        assert np.isfinite(sim.read()[0]).all()

    with handle(n, mixed=False, prec="f32") as f32:
        f32.init(b, v)
        f32.set_params(H, 1.0)
        raises(4, lambda: f32.set_pass_precision("mixed"), "nb_set_pass_precision", "NB_F32")
        assert f32.pass_precision() == "native"
        still_works(f32)
    with Simulation(n, precision="f64") as lf:
        lf.init(b, v)
        lf.set_params(H, 1.0)
        raises(4, lambda: lf.set_pass_precision("mixed"), "nb_set_pass_precision", "Hermite handle")
        raises(4, lf.pass_precision, "nb_pass_precision", "Hermite handle")
        still_works(lf)
    with handle(n, mixed=False) as six:
        six.init(b, v)
        six.set_params(H, 1.0)
        six.set_hermite_order(6)
        raises(4, lambda: six.set_pass_precision("mixed"), "nb_set_pass_precision", "order")
        still_works(six)
    with handle(n, mixed=False) as ac:
        ac.init(b, v)
        ac.set_params(H, 1.0)
        ac.set_neighbor_scheme(radius=0.2)
        raises(4, lambda: ac.set_pass_precision("mixed"), "nb_set_pass_precision", "neighbour scheme")
        still_works(ac)
    with handle(n) as mx:
        mx.init(b, v)
        mx.set_params(H, 1.0)
        raises(1, lambda: mx.set_pass_precision(2), "nb_set_pass_precision", "mode")
        raises(4, lambda: mx.set_hermite_order(6), "nb_set_hermite_order", "NB_PASS_MIXED")
        raises(4, lambda: mx.set_neighbor_scheme(radius=0.2), "nb_set_neighbor_scheme", "NB_PASS_MIXED")
        assert mx.pass_precision() == "mixed" and mx.hermite_order() == 4
        still_works(mx)
        mx.set_pass_precision(0)
        mx.set_hermite_order(6)                            # allowed again once the mode is native
        still_works(mx)


# ---- 8. nb_force_pass ----------------------------------------------------------------------------------------------------------
def test_force_pass_leaves_state_and_derivatives_alone():
    n = 1025
    b, v = M.pass_system("hard", n)
    with handle(n, eps2=1e-8) as sim, handle(n, eps2=1e-8) as twin:
        for s in (sim, twin):
            s.init(b, v)
            s.simulate(2, H, 1.0)
        before = bits(sim)
        assert sim.force_pass(1) > 0
        assert bits(sim) == before
        sim.simulate(2)
        twin.simulate(2)
        assert bits(sim) == bits(twin)
