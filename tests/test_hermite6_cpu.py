"""The 6th-order Hermite scheme (nb_set_hermite_order; added within ABI 2.4, round 20) without a device: the exports and the header
text, the rejections that need no handle, the built code of the nb_h6_* kernels, the numpy restatement's own formulas (the snap
against a finite difference of the jerk, the crackle on polynomials, the order of convergence on a Kepler orbit), the recorded
figures and the binding surface."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

from nbody3d_amd import capi

import hermite6_ref as R

CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
NAMES = ("nb_set_hermite_order", "nb_hermite_order", "nb_download_snap", "nb_upload_derivs6")


def test_library_exports_the_entry_points_and_the_header_states_the_scheme():
    L = capi.load_library()
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and name in text
        assert getattr(L, name) is not None
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 20)" in text
    for line in ("alpha = (dr.dv) / rho^2", "beta = (dv.dv + dr.da) / rho^2 + alpha^2", "S = m_j da / rho^3 - 6 alpha J - 3 beta A",
                 "xp = x + h v + h^2/2 a + h^3/6 j + h^4/24 s + h^5/120 c", "ap = a + h j + h^2/2 s + h^3/6 c",
                 "v1 = v + h/2 (a + a1) - h^2/10 (j1 - j) + h^3/120 (s + s1)", "x1 = x + h/2 (v + v1) - h^2/10 (a1 - a) + h^3/120 (j + j1)",
                 "c1 = (60 P - 36 Q + 9 R) / h^3"):
        assert line in text, line
    assert "integrator = 2" not in text and capi.abi_minor() == 4       # no new nb_integrator value, the minor stays


def test_rejections_that_need_no_handle():
    """NB_ERR_INVALID (1) for a NULL handle, the message naming the function.  (integrator = 2 stays NB_ERR_INVALID:
    tests/test_hermite_cpu.py.  Every NB_ERR_STATE case needs a handle: tests/test_hermite6_gpu.py.)"""
    L = capi.load_library()
    buf = (C.c_float * 4)()
    o = C.c_uint32(9)
    for order in (4, 6, 5):
        assert L.nb_set_hermite_order(None, order) == 1 and b"nb_set_hermite_order" in L.nb_last_error(None)
    assert L.nb_hermite_order(None, C.byref(o)) == 1 and b"nb_hermite_order" in L.nb_last_error(None) and o.value == 9
    assert L.nb_download_snap(None, buf, buf) == 1 and b"nb_download_snap" in L.nb_last_error(None)
    assert L.nb_upload_derivs6(None, buf, buf, buf, buf) == 1 and b"nb_upload_derivs6" in L.nb_last_error(None)


def h6_kernels():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    text = open(os.path.join(CSRC, "nb_engine.gfx950.s")).read()
    res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN2nb\d+nb_h6_\w+):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M)}
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+)", res, re.S):
        if re.match(r"_ZN2nb\d+nb_h6_", m.group(1)) and "Function Name" not in m.group(2):
            scratch[m.group(1)] = int(m.group(3))
    return bodies, scratch


def test_h6_kernels_use_no_scratch():
    bodies, scratch = h6_kernels()
    assert bodies and set(scratch) == set(bodies), (sorted(bodies), sorted(scratch))
    assert all(v == 0 for v in scratch.values()), scratch
    for want in ("nb_h6_fjs_pk", "nb_h6_fjs64", "nb_h6_reduce", "nb_h6_predict", "nb_h6_correct"):
        assert any(want in k for k in bodies), want
    for k, v in bodies.items():
        assert "scratch_" not in v, k
        assert "atomic" not in v, k
        if "nb_h6_fjs_pk" in k:
            assert "v_pk_fma_f32" in v and "v_rsq_f32" in v and "global_load_lds_dwordx4" in v, k
        if "nb_h6_fjs64" in k:
            assert "v_rsq_f64" in v and "v_fma_f64" in v, k


def test_f32_force_jerk_snap_loop_is_the_pair_arithmetic():
    """The innermost plain loop of nb_h6_fjs_pk: per two v_rsq_f32 (one packed group against one j-body) at most 48 packed
    instructions, at most one more VALU instruction in fourteen around them, and nothing that touches global memory or scratch
    (tests/test_hermite_cpu.py's rule with 48 for 26)."""
    bodies, _ = h6_kernels()
    body = [v for k, v in bodies.items() if "nb_h6_fjs_pk" in k][0]
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
        print("nb_h6_fjs_pk inner loop: %d instructions, %d VALU, %d v_pk_*, %d v_rsq_f32" % (len(ops), len(valu), pk, rsq))
        assert rsq >= 8 and rsq % 2 == 0 and 0 < pk <= 48 * (rsq // 2), (rsq, pk)
        assert len(valu) - pk - rsq <= (pk + rsq) // 14, (len(valu), pk, rsq)
        assert not any(o.startswith("scratch_") or o.startswith("global_") for o in ops)
        # the tally profiles/r20/hermite6.md and DESIGN 7.12 derive the pass's bar from (the `make asm` output is regenerated, not
        # tracked): 384 packed + 16 v_rsq_f32 + 10 other VALU per 8 two-pairs = 213.0 issue cycles.  A compiler that builds another
        # loop fails here: the documents' bar is then stale and has to be derived again.
        assert (pk, rsq, len(valu) - pk - rsq) == (384, 16, 10), (pk, rsq, len(valu) - pk - rsq)
        assert (4 * pk + 8 * rsq + 4 * (len(valu) - pk - rsq)) / (rsq // 2) == 213.0


# ---- the restatement's own formulas ---------------------------------------------------------------------------------------------
def test_snap_is_the_time_derivative_of_the_jerk_along_a_trajectory():
    """The jerk at t +- d on the trajectory x + d v + d^2/2 a + d^3/6 j, v + d a + d^2/2 j (no snap in it: what it leaves out moves
    the central difference by O(d^2)), differenced, against the restatement's snap.  d = 2^-12 = 2.4e-4: truncation ~ d^2 times a few = 3e-7 of the
    scale (measured 2.6e-7), the rounding of the difference 1e-16 / d ~ 5e-13; a wrong coefficient in S is an error of order 1."""
    rng = np.random.default_rng(11)
    n = 9
    b = np.concatenate([rng.normal(size=(n, 3)), rng.uniform(0.05, 0.3, (n, 1))], 1)
    v = np.concatenate([rng.normal(size=(n, 3)) * 0.5, np.zeros((n, 1))], 1)
    G, eps2 = 0.8, 1e-2
    a, j, _ = R.fjs(b, v, None, G, eps2)
    s = R.fjs(b, v, a, G, eps2)[2]
    d = 2.0 ** -12
    js = []
    for sg in (1.0, -1.0):
        h = sg * d
        bb, vv = b.copy(), v.copy()
        bb[:, :3] = b[:, :3] + h * v[:, :3] + h * h / 2 * a + h ** 3 / 6 * j
        vv[:, :3] = v[:, :3] + h * a + h * h / 2 * j
        js.append(R.fjs(bb, vv, None, G, eps2)[1])
    fd = (js[0] - js[1]) / (2 * d)
    err = float(np.abs(fd - s).max() / np.abs(s).max())
    print("snap against the central difference of the jerk: %.3g" % err)
    assert err <= 1e-6, err
    # and the jerk against the difference of the acceleration, the same way (it fixes the sign conventions the snap builds on)
    as_ = []
    for sg in (1.0, -1.0):
        bb = b.copy()
        bb[:, :3] = b[:, :3] + sg * d * v[:, :3] + d * d / 2 * a
        as_.append(R.fjs(bb, v, None, G, eps2)[0])
    assert float(np.abs((as_[0] - as_[1]) / (2 * d) - j).max() / np.abs(j).max()) <= 1e-6


@pytest.mark.parametrize("p", [3, 4, 5])
def test_crackle_is_exact_on_polynomials_up_to_the_fifth_degree(p):
    """a(t) = t^p on [t0, t0 + h]: the quintic through (a, j, s) at both ends IS a, so c1 = a'''(t0 + h) to rounding.  The sums that
    make c1 cancel to ~h^3 of their terms: rounding is 2^-53 max|term| / h^3, bounded here by 1e-12 of |c1| for h = 1/4, t0 ~ 1."""
    t0, h = np.array([0.75, 1.0, 1.5]), 0.25
    t1 = t0 + h
    a = lambda t: t ** p
    j = lambda t: p * t ** (p - 1)
    s = lambda t: p * (p - 1) * t ** (p - 2)
    c = p * (p - 1) * (p - 2) * t1 ** (p - 3)
    got = R.crackle(a(t0), j(t0), s(t0), a(t1), j(t1), s(t1), h)
    err = float(np.abs(got - c).max() / np.abs(c).max())
    print("crackle on t^%d: %.3g" % (p, err))
    assert err <= 1e-12, err


def test_sixth_order_convergence_of_the_restatement_on_a_kepler_orbit():
    """Masses 0.6 / 0.4, e = 0.5 from pericentre, one period: halving the step divides the position error by ~2^6 = 64.  The errors
    at these steps (2e-5 .. 5e-9) are >= 1e3 x what fp64 rounding accumulates over 512 steps (~1e-13); they are held against the
    run with 4 x the steps of the last, whose own error is 1 / 4,096 of it."""
    ends = R.kepler_ends()
    fine = ends[4 * R.KEPLER_STEPS[-1]]["b"][:, :3]
    e = [float(np.abs(ends[k]["b"][:, :3] - fine).max()) for k in R.KEPLER_STEPS]
    r1, r2 = e[0] / e[1], e[1] / e[2]
    print("Kepler e=0.5, steps %s: errors %s, ratios %.2f %.2f" % (R.KEPLER_STEPS, ["%.3g" % x for x in e], r1, r2))
    assert min(e) >= 1e3 * 1e-13
    assert 40 <= r1 <= 100 and 40 <= r2 <= 100, (e, r1, r2)
    rec = R.record()["kepler"]
    assert np.allclose(e, [rec["errors"][str(k)] for k in R.KEPLER_STEPS], rtol=1e-3)       # the record is this restatement's
    assert all(40 <= r <= 100 for r in rec["ratios"])


def test_the_record_is_what_the_restatement_measures():
    """The two smallest stepping cases and the smallest pass cases are run again; every recorded figure is there and none is zero
    where binary32 rounds."""
    rec = R.record()
    assert rec["fixtures"]["sizes"] == list(R.SIZES) and rec["fixtures"]["h"] == R.H and rec["fixtures"]["steps"] == list(R.STEPS)
    assert rec["fixtures"]["census"] == {k: {"n": v[0], "row": v[1], "mass": 1e3} for k, v in R.CENSUS.items()}
    for key in list(R.SIZES) + list(R.CENSUS):
        assert set(rec["pass"][str(key)]) == {"a", "j", "s"}
    for n in R.SIZES:
        for k in R.STEPS:
            assert set(rec["steps"][str(n)][str(k)]) == set(R.QUANTITIES)
    for n in (2, 3):
        b, v, a, j, s, sc = R.pass_ref(n)
        ga, gj, gs = R.pass_f32(n)
        got = {"a": R.row_err(ga, a, sc[0]), "j": R.row_err(gj, j, sc[1]), "s": R.row_err(gs, s, sc[2])}
        assert got == pytest.approx(rec["pass"][str(n)], rel=1e-6), (n, got)
        r64, r32 = R.steps_ref(n), R.steps_ref(n, np.float32)
        for k in R.STEPS:
            assert R.distances(r32[k], r64[k], R.H) == pytest.approx(rec["steps"][str(n)][str(k)], rel=1e-6)


def test_binding_surface():
    for name in ("set_hermite_order", "hermite_order", "read_snap", "upload_derivs6"):
        assert callable(getattr(capi.Simulation, name)), name
        assert not hasattr(capi.MultiSimulation, name), name
    assert list(inspect.signature(capi.Simulation.upload_derivs6).parameters)[1:] == ["accel", "jerk", "snap", "crackle"]
    with pytest.raises(ValueError):
        capi.Simulation(16, integrator="rk4")          # refused by the binding, before nb_create
    try:
        capi.Simulation(16, integrator="hermite6").close()      # accepted by the binding: a handle, or no device
    except capi.NBodyError as e:
        assert e.code == 2, e
    assert "hermite6" not in capi.INTEGRATORS            # shorthand for hermite4 + order 6: no new nb_integrator value
