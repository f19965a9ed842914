"""Block individual time steps on order-6 handles (nb_set_block_steps6; added within ABI 2.4, round 21) without a device: the
export and the header text, the rejection that needs no handle, the built code of the nb_blk6_* kernels, and the restatement's
own formulas and findings (a4 and a5 on polynomials, pinned levels against shared steps, the Kepler comparison with order 4, what
binary32 storage does to the criterion, the recorded figures)."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

from nbody3d_amd import capi, ic

import block_ref as B
import block6_ref as R
import hermite6_ref as H6

CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")


def test_library_exports_the_entry_point_and_the_header_states_the_scheme():
    L = capi.load_library()
    text = open(HEADER).read()
    assert "nb_set_block_steps6" in capi.SYMBOLS and "int nb_set_block_steps6(nb_sim *s, const nb_block_steps *cfg" in text
    assert L.nb_set_block_steps6 is not None
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 21)" in text and capi.abi_minor() == 4
    for line in ("a4 = (360 P - 192 Q + 36 R) / h^4", "a5 = (720 P - 360 Q + 60 R) / h^5",
                 "tau = cbrt(sqrt(eta^3 (|a1| |s1| + |j1|^2) / (|c1| |a5| + |a4|^2)))", "c1 = (60 P - 36 Q + 9 R) / h^3"):
        assert line in text, line
    sig = inspect.signature(capi.Simulation.set_block_steps6)
    assert list(sig.parameters) == ["self", "args", "kw"] and "frozen=False" in capi.Simulation.set_block_steps6.__doc__


def test_a_null_handle_is_invalid():
    L = capi.load_library()
    cfg = capi.nb_block_steps()
    assert L.nb_set_block_steps6(None, None) == 1 and b"nb_set_block_steps6" in L.nb_last_error(None)
    assert L.nb_set_block_steps6(None, cfg) == 1 and b"nb_set_block_steps6" in L.nb_last_error(None)


def blk6_kernels():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    text = open(os.path.join(CSRC, "nb_engine.gfx950.s")).read()
    res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN2nb\d+nb_blk6_\w+):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M)}
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+)", res, re.S):
        if re.match(r"_ZN2nb\d+nb_blk6_", m.group(1)) and "Function Name" not in m.group(2):
            scratch[m.group(1)] = int(m.group(3))
    return bodies, scratch


def test_blk6_kernels_use_no_scratch():
    bodies, scratch = blk6_kernels()
    assert bodies and set(scratch) == set(bodies), (sorted(bodies), sorted(scratch))
    assert all(v == 0 for v in scratch.values()), scratch
    for want in ("nb_blk6_fjs_pkILi2E", "nb_blk6_fjs_pkILi1E", "nb_blk6_fjs64", "nb_blk6_predict", "nb_blk6_correct"):
        assert any(want in k for k in bodies), want
    for k, v in bodies.items():
        assert "scratch_" not in v, k
        if "nb_blk6_fjs_pk" in k:
            assert "v_pk_fma_f32" in v and "v_rsq_f32" in v and "global_load_lds_dwordx4" in v, k
        if "nb_blk6_fjs64" in k:
            assert "v_rsq_f64" in v and "v_fma_f64" in v, k


# ---- the restatement's own formulas ---------------------------------------------------------------------------------------------
def test_a4_and_a5_are_exact_on_polynomials():
    """a(t) = sum_k q_k t^k / k!, k <= 5, over [0, h]: the quintic through (a, j, s) at both ends IS a(t), so a4 = q4 + q5 h and
    a5 = q5 at the end of the step, and c1 = q3 + q4 h + q5 h^2 / 2 -- up to the rounding of the differences."""
    rng = np.random.default_rng(5)
    q = rng.normal(size=(6, 4, 3))
    h = 0.37
    f = lambda t, d: sum(q[k] * t ** (k - d) / np.prod(np.arange(1, k - d + 1)) for k in range(d, 6))
    a0, j0, s0, a1, j1, s1 = f(0.0, 0), f(0.0, 1), f(0.0, 2), f(h, 0), f(h, 1), f(h, 2)
    a4, a5 = R.derivs45(a0, j0, s0, a1, j1, s1, h)
    c1 = H6.crackle(a0, j0, s0, a1, j1, s1, h)
    scale = np.abs(q).max() / h ** 5
    assert np.abs(a4 - (q[4] + q[5] * h)).max() <= 1e-12 * scale
    assert np.abs(a5 - q[5]).max() <= 1e-12 * scale
    assert np.abs(c1 - f(h, 3)).max() <= 1e-12 * scale
    for k in (4, 5):      # t^4 and t^5 alone
        z = np.zeros((1, 3))
        e4, e5 = R.derivs45(z, z, z, z + h ** k, z + k * h ** (k - 1), z + k * (k - 1) * h ** (k - 2), h)
        want4, want5 = (24.0, 0.0) if k == 4 else (120.0 * h, 120.0)
        assert np.abs(e4 - want4).max() <= 1e-11 * 120 and np.abs(e5 - want5).max() <= 1e-10 * 120, (k, e4, e5)
    # tau: a zero denominator is inf
    assert np.isinf(R.tau6(z, z, z, z, z, z, z, h, 0.02)).all()


def test_pinned_levels_reproduce_shared_steps_exactly():
    b0, v0 = ic.plummer(40, seed=21)
    st, lev, stats = R.block6_ref(b0, v0, 1.0, R.EPS2, 4e-3, 3, max_level=2, min_level=2)
    ref = H6.run(b0, v0, 1.0, 1e-3, 12)
    assert stats["block_steps"] == 12 and stats["body_steps"] == 12 * 40 and (lev == 2).all()
    d = H6.distances(st, ref, 1e-3)
    print(d)
    assert all(v == 0.0 for v in d.values()), d


def test_order_6_needs_fewer_steps_than_order_4_on_the_kepler_orbit():
    """block_ref.KEPLER: order 6 at eta 0.1 against order 4 at eta 0.02 -- more accurate in fewer body steps (the restatements
    alone)."""
    _, _, (_, _, _, _, _, s4), de4 = B.kepler_ref()
    _, _, (_, _, s6), de6 = R.kepler6_ref(0.1)
    _, _, (_, _, s6b), de6b = R.kepler6_ref()
    print("order 4 eta 0.02: |dE/E| %.3g %s;  order 6 eta 0.1: %.3g %s;  order 6 eta 0.02: %.3g %s" % (de4, s4, de6, s6, de6b, s6b))
    assert de6 < de4 and s6["body_steps"] < s4["body_steps"], (de6, de4, s6, s4)
    assert s6["clamped"] == 0 and s6b["clamped"] == 0 and de6b < de6


def test_binary32_storage_turns_the_criterion_into_noise():
    """tight_pair(plummer(64, seed 21)), dt 2^-4, one outer step, L = 8: with binary32 storage a4 and a5 are differences of
    rounded values over h^4 and h^5, the criterion asks for ever smaller steps and more than half of all decisions are clamped (the
    fp64 restatement of the same system clamps none).  So nb_set_block_steps6 refuses dynamic levels on NB_F32 handles."""
    b0, v0 = B.tight_pair(*ic.plummer(64, seed=21))
    log32, log64 = [], []
    _, lev32, s32 = R.block6_ref(b0, v0, 1.0, R.EPS2, 2.0 ** -4, 1, max_level=8, store=np.float32, log=log32)
    _, lev64, s64 = R.block6_ref(b0, v0, 1.0, R.EPS2, 2.0 ** -4, 1, max_level=8, log=log64)
    n32, c32 = R.decisions(log32)
    n64, c64 = R.decisions(log64)
    print("binary32: %d of %d decisions clamped, levels %s; fp64: %d of %d, levels %s"
          % (c32, n32, np.bincount(lev32).tolist(), c64, n64, np.bincount(lev64).tolist()))
    assert 2 * c32 > n32 and c64 == 0
    assert s32["body_steps"] > 4 * s64["body_steps"]


def test_the_recorded_figures_are_the_restatements():
    """tests/golden/block6.json against the module's fixtures, and one case measured again."""
    rec = R.record()
    fx = rec["fixtures"]
    assert fx["frozen_sizes"] == list(R.FROZEN_SIZES) and fx["dt_frozen"] == R.DT_FROZEN and fx["dt_census"] == R.DT_CENSUS
    assert set(rec["frozen"]) == {str(n) for n in R.FROZEN_SIZES} and set(rec["census"]) == set(R.CENSUS)
    assert fx["pair300"] == R.PAIR300 and fx["factor"] == R.FACTOR
    for case in list(rec["frozen"].values()) + list(rec["census"].values()):
        assert set(case) == set(R.QUANTITIES) and all(0 < v < 1e-4 for v in case.values()), case
    assert rec["pair300"]["stats"]["clamped"] == 0 and 0 < rec["pair300"]["noise_position_dev"] < 1e-10
    r64, r32 = R.frozen_ref(77)[3], R.frozen_ref(77, np.float32)[3]
    d = R.distances(r32[0], r64[0], R.DT_FROZEN, R.L_FROZEN)
    assert all(abs(d[q] - rec["frozen"]["77"][q]) <= 1e-12 + 1e-6 * d[q] for q in R.QUANTITIES), (d, rec["frozen"]["77"])
