"""Pair census on the GPU: every force pass, nb_field_eval and nb_diagnostics held to a metric that shows ONE missed, doubled or
misattributed pair (tests/census_ref.py; the tolerances are measured on the CPU, tests/golden/pair_census.json).

A case is one handle and K times (upload, one evaluation, read): run k gives mass to the rows i % K == k only, so a row is a sum of
n / K terms of bounded ratio and every single term is at least 8 tolerances of it; the K runs visit every ordered pair once.  The
reference is numpy fp64 on the stored rows, every row up to 6,200 bodies, a fixed sample of 512 rows above.  f32 kernels: the recorded
tolerance of the input (8 x the error of the reference's own binary32 arithmetic); f64 kernels: 1e-12.  The variant and split lists
are the ones the older tests pin; every case asserts the kernel family by name, so a fallback cannot pass for the kernel it replaced.

Measured on an MI355X (worst err_i of the family / the tolerance of that input / its min_share): ordered-pair f32 kernels (LDS, SGPR,
fused, j-packed) 1.9e-7 / 1.4e-6 / 2.0e-3 at n = 129 and 5.7e-7 / 4.6e-6 / 1.8e-4 at 4,099; symmetric pass, full reference 3.5e-7 /
4.5e-6 / 2.5e-4, row-sampled 3.2e-7 / 3.6e-6 / 1.1e-4; rank form 4.6e-7 / 4.4e-6 / 8.5e-5; Hermite acceleration 4.3e-7 / 3.0e-6 / 2.9e-4,
jerk 7.2e-7 / 7.9e-6; nb_field_eval accelerations 3.1e-7 / 4.6e-6 / 1.8e-4, potential 2.0e-7 / 5.3e-6 / 1.5e-3; nb_diagnostics 8.6e-9 /
1.8e-8 / 3.2e-6; every f64 kernel below 2e-14 / 1e-12.  No kernel needed a factor above 8.

Not covered (each needs a design of its own): the block-step force passes (active subsets), the layer-budget multi-pass sizes
(N >= 65,536), the headline sizes, and the equal-mass kernels, which the byte-identity tests of test_eqm_gpu.py tie to the general ones."""
import numpy as np
import pytest

import census_ref as cr
from nbody3d_amd import MultiSimulation, Simulation, capi
from test_parity_gpu import VARIANTS
from test_step_forms_gpu import F64_SHAPES
from test_sym_gpu import SYM_VARIANTS, UNIT_ARMS

pytestmark = pytest.mark.gpu

W, SINGLE = capi.NB_FLAG_WHOLE_SWEEPS, capi.NB_FLAG_SINGLE_SWEEPS
DT = {"f32": np.float32, "f64": np.float64}


def explain(hb, rows, got, r, err, what):
    """A row over the tolerance: its residual on the scale of its terms, and the single fp64 terms closest to that residual in size."""
    x, m = hb[:, :3].astype(np.float64), hb[:, 3].astype(np.float64)
    for at in np.argsort(err)[::-1][:3]:
        i = int(rows[at])
        q = np.nonzero(m)[0]
        q = q[q != i]
        dr = x[q] - x[i]
        r2 = (dr * dr).sum(1) + cr.EPS2
        t = (cr.G * m[q] / (r2 * np.sqrt(r2)))[:, None] * dr
        res = got[at, :3].astype(np.float64) - r["a"][at]
        size = np.sqrt((t * t).sum(1))
        near = np.argsort(np.abs(size - np.sqrt((res * res).sum())))[:3]
        print("  %s row %d: err %.3g, residual %s, scale %.3g, %d terms %.3g .. %.3g; nearest single terms: %s" % (
            what, i, err[at], res, r["scale"][at], len(q), size.min() if len(q) else 0, size.max() if len(q) else 0,
            [(int(q[c]), t[c].tolist(), float(size[c] / r["scale"][at])) for c in near]))


def census(n, prec, evaluate, what, jerk=False):
    """evaluate(hot rows (n, 4) in the handle's type) -> acc (n, 4) [, jerk (n, 4)] of one force evaluation on them."""
    ref, rec = cr.accel_reference(n), cr.entry("accel", n)
    rows, K = ref["rows"], ref["K"]
    tol = cr.TOL_F64 if prec == "f64" else rec["tol"]
    jtol = (cr.TOL_F64 if prec == "f64" else rec["jerk_tol"]) if jerk else None
    worst = worst_j = 0.0
    for seed in ref["seeds"]:
        b = cr.cached_bodies(n, seed)
        for k in range(K):
            hb, r = cr.hot(b, K, k), ref["runs"][(seed, k)]
            out = evaluate(hb.astype(DT[prec]))
            acc = out[0] if jerk else out
            assert acc.shape == (n, 4) and not acc[:, 3].any()
            err, w = cr.row_err(acc[rows, :3], r["a"], r["scale"])
            if w > tol:
                explain(hb, rows, acc[rows], r, err, "%s run %d" % (what, k))
            worst = max(worst, w)
            if jerk:
                assert not out[1][:, 3].any()
                worst_j = max(worst_j, cr.row_err(out[1][rows, :3], r["j"], r["j_scale"])[1])
    share = rec["min_share"] if rec["min_share"] is not None else float("inf")
    print("CENSUS %s n=%d K=%d rows=%d: worst err %.3g (tol %.3g, min_share %.3g)%s" % (
        what, n, K, len(rows), worst, tol, share, " jerk %.3g (tol %.3g)" % (worst_j, jtol) if jerk else ""))
    assert worst <= tol, (what, n, worst, tol)
    if jerk:
        assert worst_j <= jtol, (what, n, worst_j, jtol)


def leapfrog(sim):
    """One force evaluation of a leapfrog handle on freshly uploaded rows: a step's accelerations are those of the uploaded positions."""
    v = np.zeros((sim.n, 4), sim.dtype)

    def evaluate(hb):
        sim.init(hb, v)
        sim.simulate(1, 1e-3, cr.G)
        return sim.read(bodies=False, vel=False)[2]
    return evaluate


def family(variant):
    """What the name of a pinned ordered-pair variant must contain (include/nbody3d_hip.h: K II LL X; short codes are ABI 1)."""
    if variant == 0:
        return "fused"                                       # the default shape of a small system
    if variant < 100000:
        return "f32pk_lds256" if 20 <= variant < 30 else "f32pk_sgpr" if 30 <= variant < 40 else "f32_lds256"
    K, X = variant // 100000, variant % 10
    return {2: "f32pk_lds", 3: "f32pk_sgpr", 4: "fused_lds", 5: "fused_regs%d" % (1024 * X), 6: "jpairs_ws%d" % {4: 4, 8: 8, 6: 16}.get(X, 0)}[K]


# ---- ordered-pair kernels ---------------------------------------------------------------------------------------------------------
ORDERED = VARIANTS + [(601014, 1), (601014, 2), (601014, 5), (601018, 1), (601018, 2), (601018, 5), (601016, 1), (601016, 2), (601016, 5)]
assert {(402644, 0), (404324, 0), (408161, 0)} <= set(ORDERED)


@pytest.mark.parametrize("n", [1, 2, 129, 1001, 4099])        # 4,099: two 2,048-body LDS stages + 3 rows, ragged for every II, LL and X
@pytest.mark.parametrize("variant,jsplit", ORDERED)
def test_ordered_pair_kernels_f32(variant, jsplit, n):
    with Simulation(n, force_variant=variant, jsplit=jsplit) as sim:
        name = sim.variant
        assert family(variant) in name and "sym" not in name, name
        census(n, "f32", leapfrog(sim), name)


@pytest.mark.parametrize("variant,n", [(502641, 1000), (502642, 1500)])
def test_registers_only_fused_step(variant, n):
    with Simulation(n, force_variant=variant) as sim:
        name = sim.variant
        assert family(variant) in name, name
        census(n, "f32", leapfrog(sim), name)


@pytest.mark.parametrize("n", [1001, 4099])
@pytest.mark.parametrize("variant,jsplit", F64_SHAPES)
def test_ordered_pair_kernels_f64(variant, jsplit, n):
    with Simulation(n, precision="f64", force_variant=variant, jsplit=jsplit) as sim:
        name = sim.variant
        assert name.startswith("f64_lds"), name
        census(n, "f64", leapfrog(sim), name)


# ---- the symmetric pass -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1025, 2049, 5000])
@pytest.mark.parametrize("variant,jsplit", SYM_VARIANTS)
def test_symmetric_pass_f32(variant, jsplit, n):
    with Simulation(n, force_variant=variant, jsplit=jsplit) as sim:
        name = sim.variant
        rows_per_sb = 64 * (variant // 1000 % 100) * (4 if variant % 10 == 4 else 1)
        assert ("sym" in name) == (n > rows_per_sb), name            # one super-block: nothing to pair up, the ordered-pair kernel runs
        census(n, "f32", leapfrog(sim), name)


SHORT_ARMS = [(716013, 0, 0), (716083, 2, 0), (708013, 0, W), (708083, 1, 0), (704043, 3, 0), (708081, 1, 0)]     # test_sym_gpu.py's


@pytest.mark.parametrize("n", [1025, 2047, 3 * 1024 + 64, 6143])
@pytest.mark.parametrize("variant,jsplit,flags", SHORT_ARMS)
def test_symmetric_pass_short_block(variant, jsplit, flags, n):
    S = 64 * (variant // 1000 % 100)
    q = capi.plan_query(n, force_variant=variant, jsplit=jsplit, flags=flags)
    ch = 128 if variant % 10 == 1 else 64
    assert q["plan"]["nsb"] == n // S and q["plan"]["zc"] == -(-(n % S) // ch) > 0
    with Simulation(n, force_variant=variant, jsplit=jsplit, flags=flags) as sim:
        name = sim.variant
        assert "symw" in name, name
        census(n, "f32", leapfrog(sim), name)


@pytest.mark.parametrize("n", [8192, 12289])
@pytest.mark.parametrize("variant,jsplit,flags,suffix", UNIT_ARMS)
def test_symmetric_pass_sweep_unit_arms(variant, jsplit, flags, suffix, n):
    with Simulation(n, force_variant=variant, jsplit=jsplit, flags=flags) as sim:
        name = sim.variant
        assert "symw" in name and (name.endswith(suffix) if suffix else "_u" not in name.rsplit("_r", 1)[1]), name
        census(n, "f32", leapfrog(sim), name)


@pytest.mark.parametrize("variant,n,flags", [(716013, 12289, W), (708013, 20001, W), (716013, 12289, W | SINGLE), (708013, 20001, W | SINGLE)])
def test_symmetric_pass_paired_and_single_sweeps(variant, n, flags):
    with Simulation(n, force_variant=variant, flags=flags) as sim:
        name = sim.variant
        assert "symw_ipl%d_j1" % (8 if variant == 708013 else 16) in name and "_u" not in name.rsplit("_r", 1)[1], name
        census(n, "f32", leapfrog(sim), name + ("_single" if flags & SINGLE else "_paired"))


def test_symmetric_pass_default_plan_16384():
    """The default plan of a mid size cuts its sweeps in sub-sweep units (on the MI355X: 32 per sweep, the name ends in _u32)."""
    with Simulation(16384) as sim:
        name = sim.variant
        assert "symw" in name and "rank" not in name and "_u" in name.rsplit("_r", 1)[1], name
        census(16384, "f32", leapfrog(sim), name)


@pytest.mark.parametrize("n", [1025, 2049, 5 * 512 + 1])
def test_symmetric_pass_f64(n):
    with Simulation(n, precision="f64", force_variant=708013) as sim:
        name = sim.variant
        assert name.startswith("f64_symw"), name
        census(n, "f64", leapfrog(sim), name)


def test_symmetric_pass_f64_default_plan_16384():
    with Simulation(16384, precision="f64") as sim:
        name = sim.variant
        assert name.startswith("f64_symw") and "rank" not in name, name
        census(16384, "f64", leapfrog(sim), name)


# ---- the rank form and the ordered-pair shards: g virtual shards on one device -----------------------------------------------------
@pytest.mark.parametrize("n,g,precision,kw,expect", [(16384, 2, "f32", {}, "f32pk_symwrank"), (20000, 3, "f32", {}, "f32pk_symwrank"),
                                                     (1000, 3, "f32", dict(force_variant=1, jsplit=2), "f32_lds256"),
                                                     (2048, 2, "f32", dict(force_variant=1, jsplit=2), "f32_lds256"),
                                                     (16384, 4, "f64", {}, "f64_symwrank")])
def test_multi_handle_shards(n, g, precision, kw, expect):
    with MultiSimulation(n, g, precision=precision, **kw) as ms:
        name = ms.variant
        assert expect in name and ("symwrank" in expect or "sym" not in name), name
        census(n, precision, leapfrog(ms), "%s g=%d" % (name, g))


# ---- the Hermite force+jerk pass -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cr.HERMITE_SIZES)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_hermite_force_and_jerk(prec, n):
    """The derivatives without a step (an upload makes them stale, the reads evaluate them).  The acceleration carries the catch
    guarantee; the jerk is held on its own sum of term magnitudes to its own measured tolerance (a jerk term can cancel internally,
    so it has no min_share condition)."""
    v = cr.velocities(n, cr.ACCEL_INPUTS[n][1][0]).astype(DT[prec])
    with Simulation(n, precision=prec, integrator="hermite4") as sim:
        name = sim.variant
        assert name.startswith("hermite4_"), name

        def evaluate(hb):
            sim.init(hb, v)
            sim.set_params(1e-3, cr.G)
            return sim.read(bodies=False, vel=False)[2], sim.read_jerk()
        census(n, prec, evaluate, name + "_" + prec, jerk=True)


# ---- nb_field_eval ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cr.FIELD_SIZES)
@pytest.mark.parametrize("prec,f64", [("f32", False), ("f64", False), ("f32", True)])
def test_field_eval(prec, f64, n):
    """At the bodies (every row; the self pair left out inside the loop is one more per-pair decision) and at 300 arbitrary points;
    accelerations and potential.  Every term of the potential has one sign: its scale is |phi|."""
    ref, rec, fref, frec = cr.accel_reference(n), cr.entry("accel", n), cr.field_reference(n), cr.entry("field_points", n)
    K, seed, rows = ref["K"], ref["seeds"][0], ref["rows"]
    exact = prec == "f64" or f64
    tols = {"bodies": (rec["tol"], rec["phi_tol"]), "points": (frec["tol"], frec["phi_tol"])}
    b, pts = cr.cached_bodies(n, seed), fref["points"].astype(DT[prec])
    v = np.zeros((n, 4), DT[prec])
    worst = {("bodies", 0): 0.0, ("bodies", 1): 0.0, ("points", 0): 0.0, ("points", 1): 0.0}
    with Simulation(n, precision=prec) as sim:
        for k in range(K):
            sim.init(cr.hot(b, K, k).astype(DT[prec]), v)
            sim.set_params(1e-3, cr.G)
            for where, r, (a, phi) in (("bodies", ref["runs"][(seed, k)], sim.field(bodies=(0, n), f64=f64)),
                                       ("points", fref["runs"][k], sim.field(pts, f64=f64))):
                assert a.dtype == phi.dtype == (np.float64 if exact else np.float32) and not a[:, 3].any()
                worst[(where, 0)] = max(worst[(where, 0)], cr.row_err(a[:, :3], r["a"], r["scale"])[1])
                worst[(where, 1)] = max(worst[(where, 1)], cr.row_err(phi, r["phi"], np.abs(r["phi"]))[1])
        name = sim.variant
    assert len(rows) == n
    for (where, c), w in worst.items():
        tol = cr.TOL_F64 if exact else tols[where][c]
        print("CENSUS field_%s%s %s n=%d K=%d at the %s, %s: worst err %.3g (tol %.3g, min_share %.3g)" % (
            prec, "+F64" if f64 else "", name, n, K, where, ("accel", "phi")[c], w, tol,
            (rec if where == "bodies" else frec)[("min_share", "phi_min_share")[c]]))
    for (where, c), w in worst.items():
        assert w <= (cr.TOL_F64 if exact else tols[where][c]), (where, ("accel", "phi")[c], w)


# ---- nb_diagnostics ---------------------------------------------------------------------------------------------------------------
def check_ke_mom(ke, mom, hb, v):
    rke, rmom = cr.ke_mom_ref(hb, v)
    assert abs(ke - rke) <= 1e-9 * abs(rke) and np.abs(mom - rmom).max() < 1e-9, (ke, rke, mom, rmom)


@pytest.mark.parametrize("n", cr.DIAG_SIZES)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_diagnostics_potential_energy(prec, n):
    """All 136 unions of two residue classes of K = 16: every unordered pair is hot at least once, in a sum of which it is 8 tolerances
    or more.  The kernel's diagonal mask, its tile-skip rule and the row-block edges are per-pair decisions of this sum."""
    ref, rec = cr.diag_reference(n), cr.entry("diag", n)
    tol = cr.TOL_F64 if prec == "f64" else rec["tol"]
    v = ref["v"].astype(DT[prec])
    worst = 0.0
    with Simulation(n, precision=prec) as sim:
        for u, (pe_ref, scale, _) in ref["runs"].items():
            hb = cr.hot_union(ref["b"], cr.DIAG_K, *u)
            sim.init(hb.astype(DT[prec]), v)
            sim.set_params(1e-3, cr.G)
            ke, pe, mom = sim.diagnostics()
            if scale == 0:
                assert pe == 0, (u, pe)                                      # no pair: exactly nothing
            else:
                worst = max(worst, abs(pe - pe_ref) / scale)
            check_ke_mom(ke, mom, hb, v)
    print("CENSUS diag_%s n=%d K=%d: worst PE err %.3g (tol %.3g, min_share %.3g)" % (prec, n, cr.DIAG_K, worst, tol, rec["min_share"]))
    assert worst <= tol, (n, worst, tol)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_diagnostics_shards_add_up(prec):
    """A shard takes the pairs whose LOWER index it owns: three shards with unaligned begins and counts add up to the whole-system
    handle (the same pairs in another order of fp64 additions) and to the reference."""
    n, shards = 2049, [(0, 300), (300, 777), (1077, 972)]
    ref, rec = cr.diag_reference(n), cr.entry("diag", n)
    tol = cr.TOL_F64 if prec == "f64" else rec["tol"]
    v = ref["v"].astype(DT[prec])
    sims = [Simulation(n, precision=prec)] + [Simulation(n, precision=prec, shard=s) for s in shards]
    worst = worst_whole = 0.0
    try:
        for u, (pe_ref, scale, _) in ref["runs"].items():
            hb = cr.hot_union(ref["b"], cr.DIAG_K, *u)
            got = []
            for s in sims:
                s.init(hb.astype(DT[prec]), v)
                s.set_params(1e-3, cr.G)
                got.append(s.diagnostics())
            ke, pe, mom = sum(g[0] for g in got[1:]), sum(g[1] for g in got[1:]), sum(g[2] for g in got[1:])
            worst = max(worst, abs(pe - pe_ref) / scale)
            worst_whole = max(worst_whole, abs(pe - got[0][1]) / scale)
            check_ke_mom(ke, mom, hb, v)
            assert abs(ke - got[0][0]) <= 1e-12 * abs(got[0][0]) and np.abs(mom - got[0][2]).max() < 1e-12
    finally:
        for s in sims:
            s.close()
    print("CENSUS diag_shards_%s n=%d: shares against the reference %.3g (tol %.3g, min_share %.3g), against the whole handle %.3g" % (
        prec, n, worst, tol, rec["min_share"], worst_whole))
    assert worst <= tol and worst_whole <= 1e-12, (worst, worst_whole)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_diagnostics_counts_every_pair_at_the_multi_tile_chunk_size(prec):
    """N = 32,769: j-chunks of two tiles (diag_chunk = 512), the tile-skip rule live.  Every body at one point, eps2 = 1, G = 1, masses
    1 + i % 3: every pair contributes y m_i m_j with the same y = rsq(1), so PE / PE(two unit masses) is the INTEGER sum_{i<j} m_i m_j --
    one pair is 1.9e-9 of it, the bound is 1e-12.  The same for a shard and its two complements, whose shares add up to the whole."""
    n = 32769
    b = np.zeros((n, 4), DT[prec])
    b[:, :3] = (0.3, -0.2, 0.1)
    b[:, 3] = 1 + np.arange(n) % 3
    v = np.zeros((n, 4), DT[prec])
    m = b[:, 3].astype(np.int64)
    want = (int(m.sum()) ** 2 - int((m * m).sum())) // 2
    with Simulation(2, precision=prec, eps2=1.0) as two:
        two.init(np.array([[0.3, -0.2, 0.1, 1], [0.3, -0.2, 0.1, 1]], DT[prec]), np.zeros((2, 4), DT[prec]))
        two.set_params(1e-3, 1.0)
        unit = two.diagnostics()[1]
    assert abs(unit + 1.0) < 1e-6
    pes = []
    for shard in (None, (0, 1000), (1000, 20000), (21000, n - 21000)):
        with Simulation(n, precision=prec, eps2=1.0, shard=shard) as sim:
            sim.init(b, v)
            sim.set_params(1e-3, 1.0)
            pes.append(sim.diagnostics()[1] / unit)
    print("CENSUS diag_count_%s n=%d: pairs counted / expected - 1 = %.3g (whole), %.3g (three shards); one pair is %.3g" % (
        prec, n, pes[0] / want - 1, sum(pes[1:]) / want - 1, 1.0 / want))
    assert abs(pes[0] - want) <= 1e-12 * want and abs(sum(pes[1:]) - want) <= 1e-12 * want, (pes, want)
    above = np.cumsum(m[::-1])[::-1] - m                          # sum of the masses behind row i
    for p, (a, c) in zip(pes[1:], ((0, 1000), (1000, 21000), (21000, n))):
        own = int((m[a:c] * above[a:c]).sum())                    # each shard: the pairs whose LOWER index it owns
        assert abs(p - own) <= 1e-12 * want, (a, c, p, own)
