"""The mixed-precision force+jerk pass of f64 Hermite handles (nb_set_pass_precision; added within ABI 2.4, round 23) without a
device: the exports and the header text, the rejections that need no handle, the binding surface, the record tests/golden/mixed.json
as a fresh measurement of the restatement (tests/mixed_ref.py), the discriminating power of the bound the GPU test takes from it, and
the built code of the nb_mx_* kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from nbody3d_amd import capi

import mixed_ref as M

HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
CSRC = os.path.join(ROOT, "nbody3d-webgpu_amd", "csrc")
NAMES = ("nb_set_pass_precision", "nb_pass_precision")


# ---- exports, errors, binding surface ------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points_and_the_header_states_the_arithmetic():
    L = capi.load_library()
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and name in text
        assert getattr(L, name) is not None
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 23)" in text
    assert capi.ABI_MINOR == 3 and capi.abi_minor() == 4
    for line in ("#define NB_PASS_NATIVE 0u", "#define NB_PASS_MIXED  1u", "int nb_set_pass_precision(nb_sim *s, uint32_t mode);",
                 "int nb_pass_precision(nb_sim *s, uint32_t *mode);", "xl = (float)(x - (double)xh)",
                 "dr = (xh_j - xh_i) + (xl_j - xl_i)", "dv = vf_j - vf_i", "An energy audit to 1e-12 needs the native pass"):
        assert line in text, line
    assert (capi.PASS_NATIVE, capi.PASS_MIXED) == (0, 1)


def test_rejections_that_need_no_handle():
    L = capi.load_library()
    m = C.c_uint32(9)
    for mode in (0, 1, 2):
        assert L.nb_set_pass_precision(None, mode) == 1 and b"nb_set_pass_precision" in L.nb_last_error(None)
    assert L.nb_pass_precision(None, C.byref(m)) == 1 and b"nb_pass_precision" in L.nb_last_error(None) and m.value == 9


def test_binding_surface():
    assert callable(capi.Simulation.set_pass_precision) and callable(capi.Simulation.pass_precision)
    assert not hasattr(capi.MultiSimulation, "set_pass_precision") and not hasattr(capi.MultiSimulation, "pass_precision")
    sim = object.__new__(capi.Simulation)      # never created: the string is refused by the binding, before any library call
    for bad in ("double", "MIXED", ""):
        with pytest.raises(ValueError):
            capi.Simulation.set_pass_precision(sim, bad)


# ---- the restatement and its record --------------------------------------------------------------------------------------------
def test_restatement_self_term_is_zero_and_lo_word_matters():
    """Two bodies 2e-3 apart at |x| ~ 3, built in float64: with the lo word the pair's acceleration is the fp64 one to binary32
    rounding of the pair arithmetic; without it the error is that of the rounded positions, ~ ulp(3) / 2e-3."""
    b = np.array([[3.0 + 1e-3 + 1e-9, -2.0, 1.0, 0.5], [3.0 - 1e-3 + 3e-9, -2.0, 1.0, 0.5]])
    v = np.array([[0.0, 0.3, 0, 0], [0.0, -0.3, 0, 0]])
    ra, rj = M.fj_ref(b, v, 1.0, 1e-8)
    for acc in M.ACCS:
        a, j = M.fj_mixed(b, v, 1.0, 1e-8, acc=acc)
        assert M.row_err(a, ra, [0, 1]) <= 1e-6 and M.row_err(j, rj, [0, 1]) <= 1e-6, acc
    a, _ = M.fj_mixed(b, v, 1.0, 1e-8, lo=False)
    assert M.row_err(a, ra, [0, 1]) >= 1e-5
    one, _ = M.fj_mixed(b[:1], v[:1], 1.0, 1e-8)
    assert not one.any()


def test_fixtures_keep_their_lo_words():
    b, _ = M.hard(300, M.SEED, M.PAIRS, M.HALF)
    xh, xl, _, _ = M.split(b, np.zeros_like(b))
    assert xl[:2 * M.PAIRS].any(axis=1).all()            # every pair member carries a lo word (float32 rounding would zero them)
    d = b[0, :3] - b[1, :3]
    assert abs(np.sqrt((d * d).sum()) - 2 * M.HALF) <= 1e-12
    bs, _ = M.hard(300, M.SEED, M.PAIRS, M.HALF, M.SHIFT)
    assert M.split(bs, np.zeros_like(bs))[1].any(axis=1).mean() > 0.9
    assert M.BLOCK == dict(n=512, seed=21, pairs=4, half=1e-3, eps2=1e-8, dt=2 ** -4, max_level=16, eta=0.02, outer=4)


def test_the_record_is_a_fresh_measurement():
    """Present, made by the committed generator, complete; two pass cases and BLOCK's row for the double-single sum are run again."""
    rec = M.record()
    assert os.path.exists(os.path.join(ROOT, "tests", "golden", "measure_mixed.py"))
    assert rec["factor"] == M.FACTOR and rec["block_config"] == M.BLOCK and rec["pairs"] == M.PAIRS and rec["halves"] == M.HALVES
    assert {(r["kind"], r["n"]) for r in rec["pass"]} == {(k, n) for k in M.KINDS for n in M.SIZES}
    assert set(rec["block"]) == {"fp64", "hi_only", "f32_handle"} | {"mixed_" + a for a in M.ACCS}
    for kind, n in (("tight", 300), ("hard_shifted", 1025)):
        got, want = M.measure_pass(kind, n), M.pass_record(kind, n)
        for lo in ("lo", "hi_only"):
            for k, x in want[lo].items():
                assert got[lo][k] == pytest.approx(x, rel=1e-6), (kind, n, lo, k)
    got, want = M.measure_block(M.with_acc("fp64")), rec["block"]["mixed_fp64"]
    print("BLOCK, double-single differences with fp64 sums: %s" % got)
    assert {k: got[k] for k in ("block_steps", "body_steps", "clamped", "finest_level")} == {k: want[k] for k in ("block_steps", "body_steps", "clamped", "finest_level")}
    assert got["dE"] == pytest.approx(want["dE"], rel=1e-3)


def test_block_record_separates_the_failure_modes():
    """What test_mixed_gpu.py's dynamic-level test asks (block steps within 2 %, body steps within 0.5 %, |dE/E0| <= 2 x the fp64
    figure) holds for every double-single restatement with room and fails for a dropped lo word and for binary32 storage."""
    blk = M.record()["block"]
    ref = blk["fp64"]
    ok = lambda r: (abs(r["block_steps"] - ref["block_steps"]) <= 0.02 * ref["block_steps"]
                    and abs(r["body_steps"] - ref["body_steps"]) <= 0.005 * ref["body_steps"] and r["clamped"] == 0 and r["dE"] <= 2 * ref["dE"])
    for acc in M.ACCS:
        r = blk["mixed_" + acc]
        print("mixed_%s: block steps %+.3f %%, body steps %+.3f %%, dE x %.2f" % (acc, 100 * (r["block_steps"] / ref["block_steps"] - 1), 100 * (r["body_steps"] / ref["body_steps"] - 1), r["dE"] / ref["dE"]))
        assert ok(r), (acc, r, ref)
        assert abs(r["body_steps"] - ref["body_steps"]) <= 0.001 * ref["body_steps"] and r["dE"] <= 1.5 * ref["dE"]      # with room
    for bad in ("hi_only", "f32_handle"):
        r = blk[bad]
        print("%s: block steps %+.1f %%, body steps %+.1f %%, dE x %.2f" % (bad, 100 * (r["block_steps"] / ref["block_steps"] - 1), 100 * (r["body_steps"] / ref["body_steps"] - 1), r["dE"] / ref["dE"]))
        assert not ok(r), (bad, r, ref)
        assert r["block_steps"] >= 1.5 * ref["block_steps"] and r["body_steps"] >= 1.05 * ref["body_steps"]              # by a wide gap


def sum_bound(kind, n):
    """What the pass's own binary32 sums may leave on a pair member's row, relative to the row, by reasoning: the register that holds
    the partner's term takes up to n more terms, each rounded to 2^-24 of it -- a random walk of 6e-8 sqrt(n), allowed twice; on the
    pairs at +-1e-4 the partner's term is m d / rho^3 = 1.79e7 / n, most other terms lie below half an ulp of it, and up to the whole
    field of the rest of the system (at most 1 in these units) is lost: n / 1.79e7."""
    walk = 2 * 2.0 ** -24 * np.sqrt(n)
    return walk if M.HALVES[kind] == M.HALF else walk + n / 1.79e7


@pytest.mark.parametrize("kind", M.DISCRIMINATING)
@pytest.mark.parametrize("n", M.SIZES)
def test_a_dropped_lo_word_misses_the_gpu_bound_by_a_wide_gap(kind, n):
    """The GPU test holds the pair members' rows to FACTOR x the recorded lo=True figure; the restatement WITHOUT the lo word is at
    least 4 x that bound away from the fp64 sum on the same rows, accelerations and jerks alike (a ratio of at least 32 between the
    two recorded figures), so a kernel that drops or mis-stages the lo stream cannot pass.  The inputs are mixed_ref.DISCRIMINATING,
    the two shifted by (3, -2, 1): pairs at +-1e-3 and at +-1e-4.  The unshifted inputs do not give 32 everywhere (their figures are
    printed by the test below) and are accuracy cases only."""
    r = M.pass_record(kind, n)
    for q in ("pair_a", "pair_j"):
        ratio = r["hi_only"][q] / r["lo"][q]
        print("%s N=%d %s: with the lo word %.3g, without %.3g (x %.0f)" % (kind, n, q, r["lo"][q], r["hi_only"][q], ratio))
        assert r["lo"][q] <= sum_bound(kind, n), r
        assert r["hi_only"][q] >= 4 * M.FACTOR * r["lo"][q], r


def test_every_accuracy_only_input_has_a_discriminating_twin():
    """A hard kind that is not discriminating is the unshifted twin of one that is; its own ratios are printed, not asserted, and
    its lo=True figures are those of the shifted twin (the lo word carries the shift away)."""
    for kind in set(M.HARD_KINDS) - set(M.DISCRIMINATING):
        assert kind + "_shifted" in M.DISCRIMINATING
        for n in M.SIZES:
            r, tw = M.pass_record(kind, n), M.pass_record(kind + "_shifted", n)
            print("%s N=%d: ratios a x %.1f, j x %.1f" % (kind, n, r["hi_only"]["pair_a"] / r["lo"]["pair_a"], r["hi_only"]["pair_j"] / r["lo"]["pair_j"]))
            for q in ("pair_a", "pair_j"):
                assert r["lo"][q] <= sum_bound(kind, n), r
                assert r["lo"][q] == pytest.approx(tw["lo"][q], rel=1e-3), (r, tw)


# ---- the built kernels ---------------------------------------------------------------------------------------------------------
NEW = ("nb_mx_split", "nb_mx_predict", "nb_mx_blk_predict", "nb_mx_fjILi2E", "nb_mx_blk_fjILi2E", "nb_mx_blk_fjILi1E", "nb_fj_reduceIfdE", "nb_blk_correctIfdE")
_built = {}


def mixed_kernels():
    """As test_hermite_cpu.hermite_kernels: `make asm`, the bodies and the scratch sizes of the kernels this round adds."""
    if not _built:
        if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
            pytest.skip("hipcc not available")
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
        text = open(os.path.join(CSRC, "nb_engine.gfx950.s")).read()
        res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
        pick = lambda name: any(w in name for w in NEW)
        bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN2nb\d+nb_\w+):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M) if pick(m.group(1))}
        scratch = {}
        for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+)", res, re.S):
            if pick(m.group(1)) and "Function Name" not in m.group(2):
                scratch[m.group(1)] = int(m.group(3))
        _built["k"] = (bodies, scratch)
    return _built["k"]


def test_new_kernels_use_no_scratch_and_stage_by_lds_dma():
    """ScratchSize 0 for every kernel this round adds (the compiler's resource report), and the LDS-DMA load in the three passes."""
    bodies, scratch = mixed_kernels()
    assert bodies and set(scratch) == set(bodies), (sorted(bodies), sorted(scratch))
    for want in NEW:
        assert any(want in k for k in bodies), want
    assert all(v == 0 for v in scratch.values()), scratch
    for k, v in bodies.items():
        if "nb_mx_fj" in k or "nb_mx_blk_fj" in k:
            assert "global_load_lds_dwordx4" in v, k


@pytest.mark.parametrize("name", ["nb_mx_fjILi2E", "nb_mx_blk_fjILi2E", "nb_mx_blk_fjILi1E"])
def test_mixed_loop_is_the_pair_arithmetic(name):
    """The innermost loop of nb_mx_fj<2> and of nb_mx_blk_fj<2> and <1>, by test_hermite_cpu's rule with 32 for 26: per two v_rsq_f32
    at most 32 packed instructions (nb_fj_pk's 26 and the six of the double-single difference), at most one more VALU instruction
    in fourteen around them, nothing that touches global memory."""
    bodies, _ = mixed_kernels()
    body = [v for k, v in bodies.items() if name in k][0]
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
        print("%s inner loop: %d instructions, %d VALU, %d v_pk_*, %d v_rsq_f32" % (name, len(ops), len(valu), pk, rsq))
        assert rsq >= 8 and rsq % 2 == 0 and 0 < pk <= 32 * (rsq // 2), (rsq, pk)
        assert len(valu) - pk - rsq <= (pk + rsq) // 14, (len(valu), pk, rsq)
        assert not any(o.startswith("global_") for o in ops)
