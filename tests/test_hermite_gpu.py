"""The Hermite integrator (integrator="hermite4") on the GPU: the force+jerk pass against an fp64 direct sum in numpy, stepping
against an fp64 restatement of the scheme, the order of convergence on a Kepler orbit, the bitwise invariants (step batching,
read-only calls between steps, checkpoint restore) and the errors.  Shapes are the smallest at which the tile (256 rows), the
workgroup (1,024 bodies f32 / 256 f64), the flush (1,024 terms) and the j-chunk logic can go wrong."""
import numpy as np
import pytest

from conftest import rel_pos_err

from nbody3d_amd import Simulation, capi, ic

pytestmark = pytest.mark.gpu

EPS2 = 1e-4                       # the engine's default softening (nbody3d.js:234)
TOL = {"f32": 2e-5, "f64": 1e-12}


# ---- the fp64 restatement: force + jerk by direct summation, and one Hermite step (Makino & Aarseth 1992) -------------------
def fj_ref(b, v, G, eps2, rows=None):
    x, m, u = np.asarray(b, np.float64)[:, :3], np.asarray(b, np.float64)[:, 3], np.asarray(v, np.float64)[:, :3]
    rows = np.arange(len(x)) if rows is None else np.asarray(rows)
    a, j = np.zeros((len(rows), 3)), np.zeros((len(rows), 3))
    for s in range(0, len(rows), 256):
        r = rows[s:s + 256]
        dr, dv = x[None, :, :] - x[r, None, :], u[None, :, :] - u[r, None, :]
        y2 = 1.0 / ((dr * dr).sum(2) + eps2)
        s3 = m[None, :] * y2 * np.sqrt(y2)
        q = (dr * dv).sum(2) * y2
        a[s:s + 256] = G * (s3[:, :, None] * dr).sum(1)
        j[s:s + 256] = G * (s3[:, :, None] * (dv - 3.0 * q[:, :, None] * dr)).sum(1)
    return a, j


def hermite_ref(b, v, G, eps2, h, steps, aj=None):
    """aj: the derivatives a handle carries over from an earlier step (None: evaluated from (b, v), as after an upload)."""
    b, v = np.array(b, np.float64), np.array(v, np.float64)
    a, j = fj_ref(b, v, G, eps2) if aj is None else aj
    for _ in range(steps):
        bp, vp = b.copy(), v.copy()
        bp[:, :3] = b[:, :3] + h * v[:, :3] + h * h / 2 * a + h ** 3 / 6 * j
        vp[:, :3] = v[:, :3] + h * a + h * h / 2 * j
        a1, j1 = fj_ref(bp, vp, G, eps2)
        v1 = v[:, :3] + h / 2 * (a + a1) + h * h / 12 * (j - j1)
        b[:, :3] = b[:, :3] + h / 2 * (v[:, :3] + v1) + h * h / 12 * (a - a1)
        v[:, :3], a, j = v1, a1, j1
    return b, v, a, j


def norm_err(got, ref):
    """The project's metric: max |delta|_inf / max |ref|_inf."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


_systems = {}


def system(n):
    """(bodies, vel, a_ref, j_ref at G = 1): computed once per size, shared, never written."""
    if n not in _systems:
        b, v = ic.plummer(n, seed=100 + n % 89)
        if n > 7:
            b[7, 3] = 0.05          # one body of 50 (N = 1,000) to 200 (N = 4,099) times the others' mass
        a, j = fj_ref(b, v, 1.0, EPS2)
        for arr in (b, v, a, j):
            arr.setflags(write=False)
        _systems[n] = (b, v, a, j)
    return _systems[n]


def hermite(n, prec, **kw):
    return Simulation(n, precision=prec, integrator="hermite4", **kw)


# ---- 1. derivatives without a step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1.0, 0.37])
@pytest.mark.parametrize("n", [1, 2, 77, 256, 1000, 1025, 4099])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_derivatives_match_the_fp64_direct_sum(prec, n, G):
    b, v, a_ref, j_ref = system(n)
    with hermite(n, prec) as sim:
        assert sim.variant.startswith("hermite4_")
        sim.init(b, v)
        sim.set_params(1e-3, G)
        gb, gv, ga = sim.read()
        gj = sim.read_jerk()
    assert gb.tobytes() == b.astype(sim.dtype).tobytes() and gv.tobytes() == v.astype(sim.dtype).tobytes()
    assert not ga[:, 3].any() and not gj[:, 3].any()
    if n == 1:
        assert not ga.any() and not gj.any()
        return
    ea, ej = norm_err(ga[:, :3], G * a_ref), norm_err(gj[:, :3], G * j_ref)
    print("derivatives %s N=%d G=%g: acceleration %.3g, jerk %.3g" % (prec, n, G, ea, ej))
    assert ea <= TOL[prec] and ej <= TOL[prec], (ea, ej)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_coincident_bodies_of_different_velocity(prec):
    """Two bodies at the same point: their mutual acceleration term is 0, the jerk term is m dv / eps^3 -- finite, as numpy has it."""
    b = np.array([[0.25, -0.5, 0.125, 0.3], [0.25, -0.5, 0.125, 0.2], [1.0, 0.5, -0.75, 0.5]], np.float32)
    v = np.array([[0.5, 0.0, -0.25, 0], [-0.25, 0.75, 0.5, 0], [0.0, -0.5, 0.25, 0]], np.float32)
    a_ref, j_ref = fj_ref(b, v, 1.0, EPS2)
    assert np.isfinite(j_ref).all() and np.abs(j_ref).max() > 1e4      # 0.3 * 0.75 / 1e-6
    with hermite(3, prec) as sim:
        sim.init(b, v)
        sim.set_params(1e-3, 1.0)
        ga = sim.read()[2]
        gj = sim.read_jerk()
    assert np.isfinite(ga).all() and np.isfinite(gj).all()
    ea, ej = norm_err(ga[:, :3], a_ref), norm_err(gj[:, :3], j_ref)
    print("coincident %s: acceleration %.3g, jerk %.3g" % (prec, ea, ej))
    assert ea <= TOL[prec] and ej <= TOL[prec], (ea, ej)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_derivatives_at_20000_bodies_on_sampled_rows(prec):
    """Several j-chunks of more than 1,024 bodies each: both levels of the f32 sums and the fp64 sum across chunks."""
    n = 20000
    b, v = ic.plummer(n, seed=5)
    b[7, 3] = 0.05
    rows = np.unique(np.concatenate([[7, n - 1], np.random.default_rng(3).choice(n, 62, replace=False)]))
    a_ref, j_ref = fj_ref(b, v, 1.0, EPS2, rows)
    with hermite(n, prec) as sim:
        sh = sim.shape_info()
        assert sh["jsplit"] >= 2 and sh["j_per_split"] > 1024 and sh["j_per_split"] % 256 == 0, sh
        sim.init(b, v)
        sim.set_params(1e-3, 1.0)
        ga = sim.read()[2]
        gj = sim.read_jerk()
    ea, ej = norm_err(ga[rows, :3], a_ref), norm_err(gj[rows, :3], j_ref)
    print("derivatives %s N=%d (%d chunks of %d): acceleration %.3g, jerk %.3g" % (prec, n, sh["jsplit"], sh["j_per_split"], ea, ej))
    assert ea <= TOL[prec] and ej <= TOL[prec], (ea, ej)


# ---- 2. stepping against the restatement ------------------------------------------------------------------------------------
_stepped = {}


def stepped_ref():
    if not _stepped:
        b, v = ic.plummer(300, seed=21)
        _stepped["x"] = (b, v) + hermite_ref(b, v, 1.0, EPS2, 1e-3, 20)
    return _stepped["x"]


def test_f64_steps_match_the_restatement():
    b0, v0, rb, rv, ra, rj = stepped_ref()
    with hermite(300, "f64") as sim:
        sim.init(b0, v0)
        sim.simulate(20, 1e-3, 1.0)
        b, v, a = sim.read()
        j = sim.read_jerk()
    ex, ev = norm_err(b[:, :3], rb[:, :3]), norm_err(v[:, :3], rv[:, :3])
    print("20 steps f64 N=300: positions %.3g, velocities %.3g, accelerations %.3g, jerks %.3g"
          % (ex, ev, norm_err(a[:, :3], ra), norm_err(j[:, :3], rj)))
    assert ex <= 1e-10 and ev <= 1e-10, (ex, ev)
    assert np.array_equal(b[:, 3], b0[:, 3].astype(np.float64)) and not v[:, 3].any()      # the mass lane and vel.w are carried


def test_f32_steps_match_the_restatement():
    b0, v0, rb, rv, ra, rj = stepped_ref()
    with hermite(300, "f32") as sim:
        sim.init(b0, v0)
        sim.simulate(20, 1e-3, 1.0)
        b, v, a = sim.read()
    e = rel_pos_err(b, rb, 1.0)
    print("20 steps f32 N=300: rel_pos_err %.3g, velocities %.3g" % (e, norm_err(v[:, :3], rv[:, :3])))
    assert e <= 1e-4, e
    assert np.array_equal(b[:, 3], b0[:, 3])


# ---- 3. order of convergence ------------------------------------------------------------------------------------------------
def test_fourth_order_convergence_on_a_kepler_orbit():
    """Masses 0.6 / 0.4, relative orbit a = 1, e = 0.5 from pericentre, one period 2 pi: halving the step divides the error by
    ~16 (the numpy restatement: 14.7 and 15.4); a second-order scheme gives 4."""
    m1, m2 = 0.6, 0.4
    r, w = 0.5, np.sqrt(3.0)                      # r_p = a (1 - e), v_p = sqrt(G M (1 + e) / (a (1 - e)))
    b0 = np.array([[-m2 * r, 0, 0, m1], [m1 * r, 0, 0, m2]], np.float64)
    v0 = np.array([[0, -m2 * w, 0, 0], [0, m1 * w, 0, 0]], np.float64)
    end = {}
    for steps in (256, 512, 1024, 4096):
        with hermite(2, "f64", eps2=1e-8) as sim:
            sim.init(b0, v0)
            sim.simulate(steps, 2 * np.pi / steps, 1.0)
            end[steps] = sim.read()[0][:, :3]
    e = {k: np.abs(end[k] - end[4096]).max() for k in (256, 512, 1024)}
    r1, r2 = e[256] / e[512], e[512] / e[1024]
    print("Kepler e=0.5: errors %s, ratios %.2f %.2f" % ({k: "%.3g" % x for k, x in e.items()}, r1, r2))
    assert 10 <= r1 <= 22 and 10 <= r2 <= 22, (e, r1, r2)


# ---- 4. invariants ----------------------------------------------------------------------------------------------------------
def state(sim):
    return tuple(x.tobytes() for x in sim.read()) + (sim.read_jerk().tobytes(),)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bitwise_invariants(prec):
    n = 1025
    b0, v0 = ic.plummer(n, seed=21)
    with hermite(n, prec) as one, hermite(n, prec) as two:
        for s in (one, two):
            s.init(b0, v0)
            s.set_params(1e-3, 1.0)
        one.simulate(7)
        for k in range(7):
            two.step()
            if k == 2:      # read-only calls between steps change no bit
                two.field(np.zeros((5, 4), two.dtype))
                two.diagnostics()
                two.request_frame()
        assert state(one) == state(two)                        # nb_step(7) == 7 x nb_step(1); two handles, same bits
        before = state(one)
        one.simulate(3, 0.0)                                   # dt = 0: a no-op
        assert state(one) == before
        one.set_params(1e-3, 1.0)
        assert one.force_pass(2) > 0.0                         # the force+jerk pass into scratch
        assert state(one) == before
        # checkpoint: (b, v, a, j) after 5 steps; a fresh handle with upload_derivs continues with the same bits
        one.init(b0, v0)
        one.simulate(5)
        cb, cv, ca = one.read()
        cj = one.read_jerk()
        one.simulate(5)
        with hermite(n, prec) as fresh:
            fresh.init(cb, cv)
            fresh.upload_derivs(ca, cj)
            fresh.simulate(5, 1e-3, 1.0)
            assert state(fresh) == state(one)


_restore = {}


def restore_ref():
    """The restatement's own checkpoint run on the 1,025-body sphere: 5 steps, then 5 more carrying (a, j) ("continuing") and 5
    more from (x, v) alone ("cold").  Computed once, shared by both precisions."""
    if not _restore:
        b0, v0 = ic.plummer(1025, seed=21)
        b5, v5, a5, j5 = hermite_ref(b0, v0, 1.0, EPS2, 1e-3, 5)
        _restore["x"] = (b0, v0, hermite_ref(b5, v5, 1.0, EPS2, 1e-3, 5, (a5, j5))[:2], hermite_ref(b5, v5, 1.0, EPS2, 1e-3, 5)[:2])
    return _restore["x"]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_restore_without_derivatives_stays_within_the_stepping_tolerances(prec):
    """A checkpoint restored WITHOUT upload_derivs re-evaluates (a, j) at the corrected state, where the continuing handle carries
    them from the predicted state: close, not bitwise.  Tolerances are the stepping tests', against the same reference, the fp64
    restatement: 1e-10 (f64, positions and velocities, max-normalised), rel_pos_err <= 1e-4 (f32).
      - the restored handle against the restatement's restore without derivatives, and the continuing handle against the
        restatement's continuing run: within the tolerances;
      - the restored handle against the continuing handle: within the tolerances PLUS what the restatement's own two runs differ by.
        That part is the scheme's truncation and no implementation of the scheme can be without it: x1 - xp is the predictor's local
        error (~ h^4 / 24 times the snap), the force gradient near a soft close pair is ~ m / eps^3 = 1e3, and every step moves v by
        h / 2 of the difference.  The restatement in numpy fp64 gives positions 2.775e-13, velocities 2.369e-10 for this system; the
        f64 engine measured the same two figures to all printed digits on an MI355X (a first version of this test held the two
        handles to a bare 1e-10 and failed on the velocities -- as the restatement itself does)."""
    n = 1025
    b0, v0, (kb, kv), (qb, qv) = restore_ref()
    with hermite(n, prec) as one, hermite(n, prec) as cold:
        one.init(b0, v0)
        one.simulate(5, 1e-3, 1.0)
        cb, cv, _ = one.read()
        one.simulate(5)
        cold.init(cb, cv)
        cold.simulate(5, 1e-3, 1.0)
        gb, gv, _ = cold.read()
        rb, rv, _ = one.read()
    assert gb.tobytes() != rb.tobytes() or gv.tobytes() != rv.tobytes()       # the derivatives were re-evaluated, not kept
    ref_x, ref_v = norm_err(qb[:, :3], kb[:, :3]), norm_err(qv[:, :3], kv[:, :3])
    ex, ev, er = norm_err(gb[:, :3], rb[:, :3]), norm_err(gv[:, :3], rv[:, :3]), rel_pos_err(gb, rb, 1.0)
    print("restore without derivatives %s N=%d, 5 steps, against the continuing handle: positions %.3g, velocities %.3g, rel_pos_err %.3g"
          " (the restatement's two runs: %.3g, %.3g)" % (prec, n, ex, ev, er, ref_x, ref_v))
    cx, cv_, kx, kv_ = norm_err(gb[:, :3], qb[:, :3]), norm_err(gv[:, :3], qv[:, :3]), norm_err(rb[:, :3], kb[:, :3]), norm_err(rv[:, :3], kv[:, :3])
    print("  against the restatement: restored %.3g / %.3g, continuing %.3g / %.3g" % (cx, cv_, kx, kv_))
    if prec == "f64":
        assert cx <= 1e-10 and cv_ <= 1e-10 and kx <= 1e-10 and kv_ <= 1e-10, (cx, cv_, kx, kv_)
        assert ex <= 1e-10 + ref_x and ev <= 1e-10 + ref_v, (ex, ev, ref_x, ref_v)
    else:
        assert rel_pos_err(gb, qb, 1.0) <= 1e-4 and rel_pos_err(rb, kb, 1.0) <= 1e-4
        assert er <= 1e-4 + rel_pos_err(qb, kb, 1.0), er


def test_dt_and_G_may_change_between_steps():
    """A changed G re-evaluates the derivatives: stepping with G = 0.5 after steps with G = 1 equals a fresh handle started from
    the same (x, v) with G = 0.5."""
    n = 300
    b0, v0 = stepped_ref()[:2]
    with hermite(n, "f64") as sim, hermite(n, "f64") as other:
        sim.init(b0, v0)
        sim.simulate(3, 1e-3, 1.0)
        b, v, _ = sim.read()
        sim.simulate(2, 2e-3, 0.5)
        other.init(b, v)
        other.simulate(2, 2e-3, 0.5)
        assert state(sim) == state(other)


# ---- 5. errors and the default ----------------------------------------------------------------------------------------------
def test_calls_that_do_not_apply_raise_state_errors():
    b0, v0 = stepped_ref()[:2]
    with hermite(300, "f32") as sim:
        sim.init(b0, v0)
        sim.set_params(1e-3, 1.0)
        with pytest.raises(capi.NBodyError) as e:
            sim.set_exchange(lambda *a: 0)
        assert e.value.code == 4
        with pytest.raises(capi.NBodyError) as e:
            sim.integrate_pass(1)
        assert e.value.code == 4
        assert sim.device_ptr("jerk") and sim.device_ptr("accel")
    with Simulation(300) as lf:
        lf.init(b0, v0)
        lf.set_params(1e-3, 1.0)
        with pytest.raises(capi.NBodyError) as e:
            lf.read_jerk()
        assert e.value.code == 4
        with pytest.raises(capi.NBodyError) as e:
            lf.upload_derivs(np.zeros((300, 4), np.float32), np.zeros((300, 4), np.float32))
        assert e.value.code == 4
        with pytest.raises(capi.NBodyError) as e:
            lf.device_ptr("jerk")
        assert e.value.code == 4


def test_leapfrog_keyword_is_the_default():
    b0, v0 = ic.plummer(1024, seed=2)
    out = []
    for kw in ({}, {"integrator": "leapfrog"}):
        with Simulation(1024, **kw) as sim:
            sim.init(b0, v0)
            sim.simulate(10, 1e-3, 1.0)
            out.append((sim.variant,) + tuple(x.tobytes() for x in sim.read()))
    assert out[0] == out[1] and not out[0][0].startswith("hermite4_")


def test_timing_reports_force_and_integrate_parts():
    b0, v0 = system(4099)[:2]
    with hermite(4099, "f32") as sim:
        sim.init(b0, v0)
        sim.set_params(1e-3, 1.0)
        sim.enable_timing(True)
        sim.simulate(3)
        t = sim.step_breakdown()
    assert t["launches"] == 3 and t["force_ms"] > 0 and t["integrate_ms"] > 0 and t["span_ms"] >= t["force_ms"], t
