"""The decision audit of block individual time steps (Simulation.set_block_steps with dynamic levels) above the sizes where one
wave schedules and one workgroup does everything else; the inputs, the measured margins and the reasons are in tests/block_ref.py
and tests/golden/block_decisions.json (measure_block_decisions.py), the conditions on the inputs in tests/test_block_cpu.py.

Part A -- a whole schedule in fp64 against the restatement: N = 1025, 1026, 3841 and 4099 (the scheduler's per-wave segments end in
one, two, one and three bodies; 256- and 512-body segments; five, nine and all sixteen waves), every level and every count EQUAL.
The restatement's smallest decision margin is 4e-6 and noise of 1e-12 -- the fp64 bound on a and j -- flips no decision, so a
difference is a fault of the engine.
Part B -- every decision and every corrector of one block step, and the start rule, binary32 and fp64, from the values the handle
itself stores: exact in both precisions, because no force error enters.  A binary32 schedule against a reference force is NOT
decidable (noise of 2e-7 flips 1 % of the bodies) and is not attempted.  A step from level 0 never coarsens, so the level rule
itself (one level, and only at a multiple of the doubled step) is held on free motion: G = 0 and zero derivatives make every
decision want min_level exactly, and the schedule from mixed uploaded levels is integer logic."""
import numpy as np
import pytest

from conftest import rel_pos_err

from nbody3d_amd import Simulation

import block_ref as R
from block_ref import norm_err

pytestmark = pytest.mark.gpu

X_TOL = V_TOL = 1e-10                # the project's fp64 bounds on norm_err after block steps (test_block_gpu.py, frozen levels)
A_TOL = J_TOL = 1e-12
COUNTS = ("block_steps", "body_steps", "finest_level", "outer_steps", "clamped")


def hermite(n, prec):
    return Simulation(n, precision=prec, integrator="hermite4")


# ---- part A ---------------------------------------------------------------------------------------------------------------------
def expected_schedule(n):
    """Per outer step (rows, x, v, a, j, levels, cumulative stats) -- the stored sizes from their fixtures and the record, the
    others from the restatement -- and a function that gives the log (run only to explain a failure at the stored sizes)."""
    if n in R.STORED:
        rec = next(e for e in R.decisions_record()["schedules"] if e["n"] == n)
        lev, state = [np.load(p) for p in R.fixture_paths(n)]
        outs = [(state[:, 0].astype(np.int64),) + tuple(state[:, c:c + 3] for c in (1, 4, 7, 10)) + (lev, rec["stats"][0])]
        return outs, lambda: R.run_schedule(n)[1]
    outs, log = R.run_schedule(n)
    rows = np.arange(n)
    return [(rows,) + tuple(z[:, :3] for z in o[:4]) + o[4:] for o in outs], lambda: log


def explain(log, L, outer, levels):
    """The log up to the end of outer step `outer` against the engine's levels there."""
    ends = [k for k, e in enumerate(log) if e["kind"] == "step" and e["t_next"] == 2 ** L]
    return R.first_divergence(log[:ends[outer] + 1], levels)


@pytest.mark.parametrize("n", sorted(R.SCHEDULES))
def test_the_whole_schedule_follows_the_restatement(n):
    p = R.SCHEDULES[n]
    rec = next(e for e in R.decisions_record()["schedules"] if e["n"] == n)
    outs, get_log = expected_schedule(n)
    b0, v0 = R.audit_system(n, p["seed"])
    later = max(X_TOL, R.FACTOR * rec["noise_position_dev"])        # what fp64-bound noise moves the positions over the later outer steps, x 8
    assert len(outs) == p["outer"] and rec["stats"][-1]["clamped"] == 0
    with hermite(n, "f64") as sim:
        sim.init(b0, v0)
        sim.set_params(2.0 ** p["dt_log2"], 1.0)
        sim.set_block_steps(eta=R.ETA, max_level=p["max_level"])
        for k, (rows, rx, rv, ra, rj, rl, rs) in enumerate(outs):
            sim.simulate(1)
            b, v, a = sim.read()
            j = sim.read_jerk()
            st, lev = sim.block_stats(), sim.read_levels()
            errs = [norm_err(g[rows, :3], w) for g, w in ((b, rx), (v, rv), (a, ra), (j, rj))]
            print("N=%d outer step %d: %s (restatement %s); positions %.3g, velocities %.3g, a %.3g, j %.3g; levels %s"
                  % (n, k + 1, st, rs, *errs, np.bincount(lev).tolist()))
            if not np.array_equal(lev, rl):
                print(explain(get_log(), p["max_level"], k, lev))
            assert np.array_equal(lev, rl), "levels differ for bodies %s" % np.nonzero(lev != rl)[0][:32].tolist()
            for c in COUNTS:
                assert st[c] == rs[c], (c, st, rs)
            assert errs[0] <= (X_TOL if k == 0 else later) and errs[1] <= V_TOL and errs[2] <= A_TOL and errs[3] <= J_TOL, errs
            assert b[:, 3].tobytes() == b0[:, 3].astype(np.float64).tobytes() and v[:, 3].tobytes() == v0[:, 3].astype(np.float64).tobytes()
            assert not a[:, 3].any() and not j[:, 3].any()


# ---- part B ---------------------------------------------------------------------------------------------------------------------
_inputs = {}


def inputs(n, prec):
    """(b0, v0, a0, j0) in the handle's precision: computed once per (n, precision), never written."""
    if (n, prec) not in _inputs:
        _inputs[n, prec] = R.step_inputs(n, prec)
    return _inputs[n, prec]


def compare_levels(what, got, want, margin, got_clamped, want_clamped):
    """Levels equal wherever the decision is further from a level boundary than the exclusion margin; at most 0.5 % are not."""
    out = margin < R.decisions_record()["exclusion_margin"]
    bad = np.nonzero((got != want) & ~out)[0]
    print("%s: %d of %d decisions inside the exclusion margin, %d levels differ outside it, clamped %d (expected %d), levels %s"
          % (what, out.sum(), len(got), len(bad), got_clamped, want_clamped, np.bincount(got).tolist()))
    for i in bad[:16]:
        print("  body %d: engine %d, expected %d, margin %.3g" % (i, got[i], want[i], margin[i]))
    assert out.mean() <= R.EXCLUDED_CAP, out.mean()
    assert not len(bad), bad[:32].tolist()
    assert abs(got_clamped - want_clamped) <= out.sum(), (got_clamped, want_clamped)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", R.STEP_SIZES)
def test_start_rule_on_uploaded_derivatives(n, prec):
    b0, v0, a0, j0 = inputs(n, prec)
    with hermite(n, prec) as sim:
        sim.init(b0, v0)
        sim.upload_derivs(a0, j0)
        for l2, L, lmin in R.START_RUNS:
            sim.set_params(2.0 ** l2, 1.0)
            sim.set_block_steps(eta=R.ETA, max_level=L, min_level=lmin)
            sim.block_stats(reset=True)
            lev = sim.read_levels()
            st = sim.block_stats()
            stats, log = {"clamped": 0}, []
            want = R.start_levels(a0[:, :3], j0[:, :3], 2.0 ** l2, R.ETA, lmin, L, stats, log=log)
            compare_levels("start rule N=%d %s dt 2^%d L %d min_level %d" % (n, prec, l2, L, lmin), lev, want, log[0]["margin"],
                           st["clamped"], stats["clamped"])
            assert (lev[list(R.ZERO_JERK)] == lmin).all()                  # |j| = 0
            assert st["finest_level"] == lev.max() and st["block_steps"] == 0, st
        assert sim.read()[2].tobytes() == a0.tobytes() and sim.read_jerk().tobytes() == j0.tobytes()      # the start rule writes no derivative


def ulps(got, want, scale):
    """|got - want| in units of the spacing of the handle's type at `scale`, the worst component."""
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(scale).astype(got.dtype)).astype(np.float64)).max())


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", R.STEP_SIZES)
def test_one_block_step_seen_from_both_sides(n, prec):
    """Every body at level 0: one outer step is one block step of h = dt with every body active.  The new levels are decide() of the
    uploaded (a0, j0) and the (a1, j1) the handle stored; the new state is correct() of the same values, rounded once."""
    b0, v0, a0, j0 = inputs(n, prec)
    x0, u0 = b0[:, :3].astype(np.float64), v0[:, :3].astype(np.float64)
    with hermite(n, prec) as sim:
        for l2, L in R.STEP_RUNS:
            dt = 2.0 ** l2
            sim.init(b0, v0)
            sim.set_params(dt, 1.0)
            sim.upload_derivs(a0, j0)
            sim.set_block_steps(eta=R.ETA, max_level=L)
            sim.upload_levels(np.zeros(n, np.uint8))
            sim.block_stats(reset=True)
            sim.simulate(1)
            b1, v1, a1 = sim.read()
            j1 = sim.read_jerk()
            st, lev = sim.block_stats(), sim.read_levels()
            assert st["block_steps"] == 1 and st["body_steps"] == n and st["outer_steps"] == 1, st
            d = R.decide(a0, j0, a1, j1, dt, 0, 2 ** L, dt, R.ETA, 0, L)
            compare_levels("one block step N=%d %s dt 2^%d L %d" % (n, prec, l2, L), lev, d["after"], d["margin"], st["clamped"],
                           int(d["clamped"].sum()))
            assert st["finest_level"] == lev.max(), st
            wx, wv = R.correct(b0, v0, a0, j0, a1, j1, dt)
            a01, j01, a10 = [np.asarray(z, np.float64)[:, :3] for z in (a0, j0, a1)]
            if prec == "f32":                                   # one rounding of the same fp64 polynomial: at most 1 ulp of the result
                ex, ev, bound = ulps(b1[:, :3], wx.astype(np.float32), wx), ulps(v1[:, :3], wv.astype(np.float32), wv), 1.0
            else:                                               # fma against separate roundings: at most 4 ulp of the sum's largest term
                tv = np.maximum.reduce([np.abs(u0), np.abs(dt / 2 * (a01 + a10)), np.abs(dt * dt / 12 * (j01 - j1[:, :3]))])
                tx = np.maximum.reduce([np.abs(x0), np.abs(dt / 2 * (u0 + wv)), np.abs(dt * dt / 12 * (a01 - a10))])
                ex, ev, bound = ulps(b1[:, :3], wx, tx), ulps(v1[:, :3], wv, tv), 4.0
            print("  corrector: positions %.3g ulp, velocities %.3g ulp (bound %g)" % (ex, ev, bound))
            assert ex <= bound and ev <= bound, (ex, ev)
            assert b1[:, 3].tobytes() == b0[:, 3].tobytes() and v1[:, 3].tobytes() == v0[:, 3].tobytes()
            assert not a1[:, 3].any() and not j1[:, 3].any()


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", R.STEP_SIZES)
def test_free_motion_from_mixed_levels_coarsens_one_level_at_aligned_times(n, prec):
    """G = 0 and zero derivatives: every (a1, j1) the handle stores is exactly zero, so every decision wants min_level, in both
    precisions and whatever the force kernel does.  From mixed uploaded levels the schedule is integer logic (block_ref.FREE_RUNS):
    not coarsened at the first, unaligned step, then ONE level per step although `want` is several below."""
    b0, v0, a0, j0 = inputs(n, prec)
    zero = np.zeros_like(a0)
    with hermite(n, prec) as sim:
        for L, lmin in R.FREE_RUNS:
            rb, rv, ra, rj, rl, rs = R.free_schedule(n, prec, L, lmin)
            sim.init(b0, v0)
            sim.set_params(2.0 ** R.FREE_DT_LOG2, 0.0)
            sim.upload_derivs(zero, zero)
            sim.set_block_steps(eta=R.ETA, max_level=L, min_level=lmin)
            sim.upload_levels(R.free_levels(n, L, lmin))
            sim.block_stats(reset=True)
            sim.simulate(1)
            b, v, a = sim.read()
            j = sim.read_jerk()
            st, lev = sim.block_stats(), sim.read_levels()
            ex, ev = norm_err(b[:, :3], rb[:, :3]), norm_err(v[:, :3], rv[:, :3])
            print("free motion N=%d %s L %d min_level %d: %s (restatement %s), positions %.3g, velocities %.3g" % (n, prec, L, lmin, st, rs, ex, ev))
            assert np.array_equal(lev, rl), np.nonzero(lev != rl)[0][:32].tolist()
            for c in COUNTS:
                assert st[c] == rs[c], (c, st, rs)
            assert not a.any() and not j.any()
            assert v.tobytes() == v0.tobytes()                  # v1 = v0 + h/2 (0 + 0) + h^2/12 (0 - 0)
            if prec == "f64":
                assert ex <= X_TOL, ex
            else:
                assert rel_pos_err(b, rb, 1.0) <= 1e-4          # the project's binary32 position bound (test_block_gpu.py)
