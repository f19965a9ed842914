"""The start of its own of order-6 handles (nb_set_start6; added within ABI 2.4, round 22) without a device: the exports and the
header text, the rejections that need no handle, the built code of the nb_h6_crk_* kernels, the numpy restatement's own formulas
(the crackle against a central difference of its own snap, and exact on two bodies on the x axis), the payoff of the two-rule start
on the hard-pair fixture, the start margins of the fixtures the GPU test compares exactly, the recorded figures and the binding
surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from nbody3d_amd import capi

import block6_ref as B6
import hermite6_ref as H6
import start6_ref as R
from test_hermite6_cpu import h6_kernels

HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
NAMES = ("nb_set_start6", "nb_start6")


def test_library_exports_the_entry_points_and_the_header_states_the_sum():
    L = capi.load_library()
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and name in text
        assert getattr(L, name) is not None
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 22)" in text and capi.abi_minor() == 4
    for line in ("#define NB_START6_ZERO    0u", "#define NB_START6_CRACKLE 1u", "int nb_set_start6(nb_sim *s, uint32_t mode);",
                 "int nb_start6(nb_sim *s, uint32_t *mode);", "alpha = (dr.dv) y^2", "beta  = (dv.dv + dr.da) y^2 + alpha^2",
                 "gamma = (3 dv.da + dr.dj) y^2 + alpha (3 beta - 4 alpha^2)", "t = dv - 3 alpha dr", "q = da - 6 alpha t - 3 beta dr",
                 "w = dj - 9 alpha q - 9 beta t - 3 gamma dr", "c_i = G sum_j m_j y^3 w",
                 "l_i = max(level_for((eta / 2) |a| / |j|), level_for(sqrt(eta (|a| |s| + |j|^2) / (|j| |c| + |s|^2))))"):
        assert line in text, line
    assert (capi.START6_ZERO, capi.START6_CRACKLE) == (0, 1)


def test_rejections_that_need_no_handle():
    L = capi.load_library()
    m = C.c_uint32(9)
    for mode in (0, 1, 2):
        assert L.nb_set_start6(None, mode) == 1 and b"nb_set_start6" in L.nb_last_error(None)
    assert L.nb_start6(None, C.byref(m)) == 1 and b"nb_start6" in L.nb_last_error(None) and m.value == 9


def test_binding_surface():
    assert callable(capi.Simulation.set_start6) and isinstance(capi.Simulation.start6, property)
    assert not hasattr(capi.MultiSimulation, "set_start6") and not hasattr(capi.MultiSimulation, "start6")


# ---- the built kernels -------------------------------------------------------------------------------------------------------------
def test_crackle_kernels_use_no_scratch_and_no_atomics():
    bodies, scratch = h6_kernels()
    for want in ("nb_h6_crk_pk", "nb_h6_crk64", "nb_h6_reduce1"):
        assert any(want in k for k in bodies), want
    for k, v in bodies.items():
        if "nb_h6_crk" in k or "nb_h6_reduce1" in k:
            assert scratch[k] == 0 and "scratch_" not in v and "atomic" not in v, k
        if "nb_h6_crk_pk" in k:
            assert "v_pk_fma_f32" in v and "v_rsq_f32" in v and "global_load_lds_dwordx4" in v, k
        if "nb_h6_crk64" in k:
            assert "v_rsq_f64" in v and "v_fma_f64" in v, k


def test_f32_crackle_loop_is_the_pair_arithmetic():
    """The innermost plain loop of nb_h6_crk_pk, by tests/test_hermite6_cpu.py's rule with 67 for 48: per two v_rsq_f32 at most 67
    packed instructions, at most one more VALU instruction in fourteen around them, nothing that touches global memory or scratch;
    and the tally DESIGN 7.14 and profiles/r22/start6.md derive the pass's bar from."""
    bodies, _ = h6_kernels()
    body = [v for k, v in bodies.items() if "nb_h6_crk_pk" in k][0]
    lines = [l.split(";")[0].strip() for l in body.splitlines()]
    lines = [l for l in lines if l and (not l.startswith(".") or l.startswith(".LBB"))]
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"s_cbranch_\w+\s+(\S+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append(lines[labels[m.group(1)]:i + 1])
    inner = [lp for lp in loops if not any(o is not lp and len(o) < len(lp) and o[0] in lp for o in loops)]
    plain = [lp for lp in inner if any(o.startswith("v_rsq_f32") for o in lp) and not any(o.startswith("v_cmp") for o in lp)]
    assert plain, [len(lp) for lp in inner]
    for lp in plain:
        ops = [l.split()[0] for l in lp if not l.endswith(":")]
        valu = [o for o in ops if o.startswith("v_")]
        rsq = sum(o.startswith("v_rsq_f32") for o in valu)
        pk = sum(o.startswith("v_pk_") for o in valu)
        print("nb_h6_crk_pk inner loop: %d instructions, %d VALU, %d v_pk_*, %d v_rsq_f32" % (len(ops), len(valu), pk, rsq))
        assert rsq >= 8 and rsq % 2 == 0 and 0 < pk <= 67 * (rsq // 2), (rsq, pk)
        assert len(valu) - pk - rsq <= (pk + rsq) // 14, (len(valu), pk, rsq)
        assert not any(o.startswith("scratch_") or o.startswith("global_") for o in ops)
        # 536 packed + 16 v_rsq_f32 + 15 other VALU per 8 two-pairs = 291.5 issue cycles, against the snap pass's 213.0
        assert (pk, rsq, len(valu) - pk - rsq) == (536, 16, 15), (pk, rsq, len(valu) - pk - rsq)
        assert (4 * pk + 8 * rsq + 4 * (len(valu) - pk - rsq)) / (rsq // 2) == 291.5


# ---- the restatement's own formulas ------------------------------------------------------------------------------------------------
def test_crackle_is_the_time_derivative_of_the_snap_along_a_trajectory():
    """The restatement's snap at t +- d on the trajectory that carries x, v and a by their Taylor polynomials through the crackle
    (what they leave out moves the central difference by O(d^2)), differenced, against the restatement's crackle.  d = 2^-12:
    truncation ~ d^2 times a few = 3e-7 of the scale, the rounding of the difference 1e-16 / d ~ 5e-13; a wrong coefficient in
    gamma or w is an error of order 1."""
    rng = np.random.default_rng(11)
    n = 9
    b = np.concatenate([rng.normal(size=(n, 3)), rng.uniform(0.05, 0.3, (n, 1))], 1)
    v = np.concatenate([rng.normal(size=(n, 3)) * 0.5, np.zeros((n, 1))], 1)
    G, eps2 = 0.8, 1e-2
    st = R.start(b, v, G, eps2)
    a, j, s, c = st["a"], st["j"], st["s"], st["c"]
    d = 2.0 ** -12
    ss = []
    for sg in (1.0, -1.0):
        h = sg * d
        bb, vv = b.copy(), v.copy()
        bb[:, :3] = b[:, :3] + h * v[:, :3] + h * h / 2 * a + h ** 3 / 6 * j + h ** 4 / 24 * s + h ** 5 / 120 * c
        vv[:, :3] = v[:, :3] + h * a + h * h / 2 * j + h ** 3 / 6 * s + h ** 4 / 24 * c
        aa = a + h * j + h * h / 2 * s + h ** 3 / 6 * c
        ss.append(H6.fjs(bb, vv, aa, G, eps2)[2])
    fd = (ss[0] - ss[1]) / (2 * d)
    err = float(np.abs(fd - c).max() / np.abs(c).max())
    print("crackle against the central difference of the snap: %.3g" % err)
    assert err <= 1e-6, err


def test_crackle_is_exact_for_two_bodies_on_the_x_axis():
    """Two bodies on the x axis, moving along it: with R = x_1 - x_0, the acceleration of body 0 is G m_1 f(R), f = R (R^2 + eps2)^-3/2,
    and everything is one-dimensional:  c = G m_1 (f' R''' + 3 f'' R' R'' + f''' R'^3)  with R', R'', R''' the differences of v, a
    and j.  f's derivatives in closed form (u = R^2 + eps2):
      f' = u^-3/2 - 3 R^2 u^-5/2,  f'' = -9 R u^-5/2 + 15 R^3 u^-7/2,  f''' = -9 u^-5/2 + 90 R^2 u^-7/2 - 105 R^4 u^-9/2."""
    G, eps2 = 0.7, 1e-3
    b = np.array([[0.1, 0, 0, 0.6], [0.9, 0, 0, 0.4]])
    v = np.array([[0.3, 0, 0, 0], [-0.5, 0, 0, 0]])
    st = R.start(b, v, G, eps2)
    Rr = b[1, 0] - b[0, 0]
    d1, d2, d3 = v[1, 0] - v[0, 0], st["a"][1, 0] - st["a"][0, 0], st["j"][1, 0] - st["j"][0, 0]
    u = Rr * Rr + eps2
    f1 = u ** -1.5 - 3 * Rr ** 2 * u ** -2.5
    f2 = -9 * Rr * u ** -2.5 + 15 * Rr ** 3 * u ** -3.5
    f3 = -9 * u ** -2.5 + 90 * Rr ** 2 * u ** -3.5 - 105 * Rr ** 4 * u ** -4.5
    want0 = G * b[1, 3] * (f1 * d3 + 3 * f2 * d1 * d2 + f3 * d1 ** 3)
    want1 = -G * b[0, 3] * (f1 * d3 + 3 * f2 * d1 * d2 + f3 * d1 ** 3)
    got = st["c"]
    print("two bodies: crackle %s, closed form %s" % (got[:, 0], (want0, want1)))
    assert abs(got[0, 0] - want0) <= 1e-12 * abs(want0) and abs(got[1, 0] - want1) <= 1e-12 * abs(want1)
    assert not got[:, 1:].any()
    # the snap the same way: s = G m_1 (f' R'' + f'' R'^2)
    assert abs(st["s"][0, 0] - G * b[1, 3] * (f1 * d2 + f2 * d1 ** 2)) <= 1e-12 * abs(st["s"][0, 0])


def test_start_modes_share_a_j_and_s():
    b, v = H6.system(257)
    z, c = R.start(b, v, 1.0, mode=R.ZERO), R.start(b, v, 1.0)
    assert not z["c"].any() and c["c"].any()
    for q in ("a", "j", "s"):
        assert z[q].tobytes() == c[q].tobytes()


def test_two_rule_levels():
    """The maximum of both rules; a zero denominator votes lmin; a body clamped by both rules counts once."""
    a = np.array([[1.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0]])
    j = np.array([[1.0, 0, 0], [64.0, 0, 0], [0.0, 0, 0], [1e9, 0, 0], [0.0, 0, 0]])
    s = np.array([[64.0, 0, 0], [1.0, 0, 0], [4.0, 0, 0], [1e18, 0, 0], [0.0, 0, 0]])
    c = np.array([[4096.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0], [1e27, 0, 0], [0.0, 0, 0]])
    stats = {"clamped": 0}
    lev, w1, w2 = R.start_levels2(a, j, s, c, 1.0, 1.0, 1, 8, stats)
    # body 0: rule 1 tau 0.5 -> 1; rule 2 tau = sqrt((64 + 1) / (4096 + 4096)) = 0.089 -> 4
    # body 1: rule 1 tau 1/128 -> 7; rule 2 tau = sqrt((1 + 4096) / (64 + 1)) -> lmin
    # body 2: |j| = 0: rule 1 votes lmin; rule 2 tau = sqrt(4 / 16) = 0.5 -> 1
    # body 3: both rules find no level: clamped once;  body 4: both denominators 0: lmin
    assert w1.tolist() == [1, 7, 1, 8, 1] and w2.tolist() == [4, 1, 1, 8, 1] and lev.tolist() == [4, 7, 1, 8, 1]
    assert stats["clamped"] == 1


# ---- the payoff and the margins ----------------------------------------------------------------------------------------------------
def test_two_rule_start_pays_on_the_hard_pair_fixture():
    """with_tight_pairs(1024, 21, 0.01, 0.001), eps2 1e-8, dt 2^-4, max_level 16, eta 0.05, one outer step: the first-step |dE/E0|
    of the new start is at most 1/10 of the specified start's (observed 1/136) for at most 1.05 x the body steps (observed 1.009 x)."""
    zero, new = R.hard_ref(R.ZERO), R.hard_ref(R.CRACKLE)
    de0, de1 = zero[3], new[3]
    s0, s1 = zero[2][2], new[2][2]
    print("hard pairs: |dE/E0| %.3g -> %.3g (1/%.0f), body steps %d -> %d (x %.4f), block steps %d -> %d"
          % (de0, de1, de0 / de1, s0["body_steps"], s1["body_steps"], s1["body_steps"] / s0["body_steps"], s0["block_steps"], s1["block_steps"]))
    assert de1 <= de0 / 10, (de0, de1)
    assert s1["body_steps"] <= 1.05 * s0["body_steps"], (s0, s1)
    assert s0["clamped"] == 0 and s1["clamped"] == 0
    rec = R.record()["hard"]
    assert rec["zero"]["stats"] == s0 and rec["crackle"]["stats"] == s1
    assert rec["zero"]["dE"] == pytest.approx(de0, rel=1e-3) and rec["crackle"]["dE"] == pytest.approx(de1, rel=1e-3)


def test_start_margins_of_the_exact_fixtures():
    """No start decision of a fixture whose start levels the GPU test compares exactly sits within 1e-6 of a level boundary (the
    restatement alone; two fp64 evaluations of a tau differ by ~1e-15)."""
    margins = {"tiny_%d_%d" % ns: R.tiny_start(*ns)[3] for ns in B6.TINY}
    margins["pair300"] = R.pair300_start()[3]
    margins["hard_zero"], margins["hard_crackle"] = R.hard_ref(R.ZERO)[4], R.hard_ref(R.CRACKLE)[4]
    print("smallest start margins: %s" % margins)
    assert all(m >= 1e-6 for m in margins.values()), margins


def test_the_record_is_what_the_restatement_measures():
    """Present, made by the committed generator, complete; the two smallest cases are run again."""
    rec = R.record()
    assert rec["generator"].startswith("tests/golden/measure_start6.py") and os.path.exists(os.path.join(ROOT, "tests", "golden", "measure_start6.py"))
    assert rec["fixtures"]["sizes"] == list(R.SIZES) and rec["fixtures"]["h"] == R.H and rec["fixtures"]["steps"] == list(R.STEPS)
    assert rec["fixtures"]["hard"] == R.HARD and rec["fixtures"]["factor"] == R.FACTOR
    for key in list(R.SIZES) + list(R.CENSUS):
        assert set(rec["pass"][str(key)]) == {"c"} and rec["pass"][str(key)]["c"] > 0
    for n in R.SIZES:
        for k in R.STEPS:
            assert set(rec["steps"][str(n)][str(k)]) == set(R.QUANTITIES)
    for n in (2, 3):
        b, v, a, j, c, sc = R.pass_ref(n)
        assert H6.row_err(R.pass_f32(n), c, sc) == pytest.approx(rec["pass"][str(n)]["c"], rel=1e-6)
        r64, r32 = R.steps_ref(n), R.steps_ref(n, np.float32)
        for k in R.STEPS:
            assert H6.distances(r32[k], r64[k], R.H) == pytest.approx(rec["steps"][str(n)][str(k)], rel=1e-6)
