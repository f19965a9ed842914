"""The guarded sums of the mixed-precision force+jerk pass (nb_set_pass_guard; added within ABI 2.4, round 24) without a device: the
exports and the header text, the rejections that need no handle, the binding surface, the record tests/golden/guard.json as a fresh
measurement of the restatement (tests/guard_ref.py), the discriminating power of the bounds the GPU test takes from it, a condition
on the sum scheme itself, and the built code of the nb_mxg_* kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from nbody3d_amd import capi

import guard_ref as Gd
import mixed_ref as M

HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
CSRC = os.path.join(ROOT, "nbody3d-webgpu_amd", "csrc")
NAMES = ("nb_set_pass_guard", "nb_pass_guard")
R0 = Gd.R_NEARS[0]


# ---- exports, errors, binding surface ------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points_and_the_header_states_the_sums():
    L = capi.load_library()
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and name in text
        assert getattr(L, name) is not None
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 24)" in text
    for line in ("int nb_set_pass_guard(nb_sim *s, double r_near);", "int nb_pass_guard(nb_sim *s, double *r_near);",
                 "NEAR iff binary32 d2 < (float)(r_near * r_near)", "s = hi + p;  bb = s - hi;  e = (hi - (s - bb)) + (p - bb);  hi = s;  lo += e",
                 "((double)far + (double)hi) + (double)lo", "plain NB_PASS_MIXED's bit for bit", "not on which rows share its wave",
                 "The self pair is near when r_near^2 > eps2 and contributes exactly 0"):
        assert line in text, line
    assert "#define NB_PASS_MIXED  1u" in text and "NB_PASS_GUARD" not in text      # no third pass precision


def test_rejections_that_need_no_handle():
    L = capi.load_library()
    r = C.c_double(9.0)
    for bad in (0.0, 0.01, -1.0, float("nan")):
        assert L.nb_set_pass_guard(None, bad) == 1 and b"nb_set_pass_guard" in L.nb_last_error(None)
    assert L.nb_pass_guard(None, C.byref(r)) == 1 and b"nb_pass_guard" in L.nb_last_error(None) and r.value == 9.0


def test_binding_surface():
    assert callable(capi.Simulation.set_pass_guard) and callable(capi.Simulation.pass_guard)
    assert not hasattr(capi.MultiSimulation, "set_pass_guard") and not hasattr(capi.MultiSimulation, "pass_guard")
    sim = object.__new__(capi.Simulation)      # never created: refused by the binding, before any library call
    for bad in ("near", None, [0.01], ""):
        with pytest.raises(ValueError):
            capi.Simulation.set_pass_guard(sim, bad)


# ---- the restatement and its record --------------------------------------------------------------------------------------------
def test_a_guard_that_holds_no_pair_is_the_plain_mixed_sum():
    """r_near^2 <= eps2: d2 >= eps2 for every pair, the self pair included, so nothing is near -- exactly fj_mixed(acc="f32"), for
    r_near = 0, sqrt(eps2) and something smaller; and a radius just above sqrt(eps2) holds the self pair, which contributes 0."""
    n, eps2 = 1025, 1e-8
    b, v = M.pass_system("tight_shifted", n)
    rows = np.r_[0:2 * M.PAIRS, n - 3:n]
    a0, j0 = M.fj_mixed(b, v, 1.0, eps2, rows, acc="f32")
    for r_near in (0.0, 1e-5, float(np.sqrt(eps2)), 1.01e-4):
        a, j = Gd.fj_guarded(b, v, 1.0, eps2, r_near, rows)
        assert a.tobytes() == a0.tobytes() and j.tobytes() == j0.tobytes(), r_near
    a, _ = Gd.fj_guarded(b, v, 1.0, eps2, R0, rows)
    assert a.tobytes() != a0.tobytes()
    one, _ = Gd.fj_guarded(b[:1], v[:1], 1.0, eps2, R0)
    assert not one.any()


def test_barycentre_rows():
    b = np.zeros((2 * M.PAIRS, 4))
    b[:, 3] = np.arange(1, 2 * M.PAIRS + 1)
    a = np.arange(2 * M.PAIRS * 3, dtype=np.float64).reshape(-1, 3)
    g = Gd.bary(a, b)
    assert g.shape == (M.PAIRS, 3)
    assert np.allclose(g[1], (3 * a[2] + 4 * a[3]) / 7)
    assert Gd.bary_err(a, a, b) == 0.0 and Gd.bary_err(1.5 * a, a, b) == pytest.approx(0.5)


def test_the_record_is_a_fresh_measurement():
    """Present, made by the committed generator, complete; the 1,025-body cases are run again."""
    rec = Gd.record()
    assert os.path.exists(os.path.join(ROOT, "tests", "golden", "measure_guard.py"))
    assert rec["factor"] == M.FACTOR and rec["block_config"] == M.BLOCK and rec["r_nears"] == list(Gd.R_NEARS) == [0.01, 0.03, 1e3]
    assert {(r["kind"], r["n"]) for r in rec["pass"]} == {(k, n) for k in M.HARD_KINDS for n in M.SIZES}
    assert [r["n"] for r in rec["plummer"]] == list(M.SIZES) and [r["n"] for r in rec["steps"]] == list(Gd.STEPS_SIZES)
    assert set(rec["block"]) == {Gd.key(R0)}
    for kind in M.HARD_KINDS:
        got, want = Gd.measure_pass(kind, 1025), Gd.pass_record(kind, 1025)
        assert set(want) == {"kind", "n", "eps2", "f32", "fp64"} | {Gd.key(r) for r in Gd.R_NEARS}
        for s in set(want) - {"kind", "n", "eps2"}:
            for q in Gd.QUANTITIES:
                assert got[s][q] == pytest.approx(want[s][q], rel=1e-6), (kind, s, q)
    got, want = Gd.measure_plummer(1025), rec["plummer"][1]
    assert got["a"] == pytest.approx(want["a"], rel=1e-6) and got["j"] == pytest.approx(want["j"], rel=1e-6)


@pytest.mark.parametrize("n", M.SIZES)
@pytest.mark.parametrize("kind", M.HARD_KINDS)
def test_todays_sums_miss_the_gpu_bound_by_a_wide_gap(kind, n):
    """The GPU test holds the barycentre rows to FACTOR x the recorded guarded figure.  The plain mixed pass's binary32 sums are at
    least 4 x that bound away from the fp64 sum on the barycentre jerk of every hard kind at every size, and on the barycentre
    acceleration at 1,025 and 4,099: a kernel whose near terms still enter the binary32 registers cannot pass."""
    r = Gd.pass_record(kind, n)
    for q in ("bary_j",) + (("bary_a",) if n >= 1025 else ()):
        ratio = r["f32"][q] / r[Gd.key(R0)][q]
        print("%s N=%d %s: guarded %.3g, binary32 sums %.3g (x %.0f)" % (kind, n, q, r[Gd.key(R0)][q], r["f32"][q], ratio))
        assert r["f32"][q] >= 4 * M.FACTOR * r[Gd.key(R0)][q], (q, r)


@pytest.mark.parametrize("n", M.SIZES)
@pytest.mark.parametrize("kind", M.HARD_KINDS)
def test_the_guarded_sum_is_close_to_the_fp64_sum_of_the_same_terms(kind, n):
    """A condition, not a measurement: every guarded barycentre figure at r_near = 0.01 is within 64 x the figure the fp64 sum of
    the same pair terms leaves (what remains there is the binary32 pair arithmetic).  A sum scheme weaker than the one specified
    -- CPU prototypes of Kahan sums left 2e-2 ... 0.2 on the barycentre jerk, of spans folded into fp64 6e-4 ... 3e-3 on the
    barycentre acceleration -- is thousands of times away and cannot be the record."""
    r = Gd.pass_record(kind, n)
    for q in ("bary_a", "bary_j"):
        print("%s N=%d %s: guarded %.3g, fp64 sum of the same terms %.3g (x %.1f)" % (kind, n, q, r[Gd.key(R0)][q], r["fp64"][q], r[Gd.key(R0)][q] / r["fp64"][q]))
        assert r[Gd.key(R0)][q] <= 64 * r["fp64"][q], (q, r)


# ---- the built kernels ---------------------------------------------------------------------------------------------------------
NEW = ("nb_mxg_fjILi2E", "nb_mxg_blk_fjILi2E", "nb_mxg_blk_fjILi1E")
_built = {}


def guard_kernels():
    """As test_mixed_cpu.mixed_kernels: `make asm`, the bodies and the resource reports of the kernels this round adds."""
    if not _built:
        if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
            pytest.skip("hipcc not available")
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
        text = open(os.path.join(CSRC, "nb_engine.gfx950.s")).read()
        res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
        pick = lambda name: any(w in name for w in NEW)
        bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN2nb\d+nb_\w+):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M) if pick(m.group(1))}
        report = {}
        for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", res, re.S):
            if pick(m.group(1)) and "Function Name" not in m.group(2):
                report[m.group(1)] = (int(m.group(3)), int(m.group(4)))
        _built["k"] = (bodies, report)
    return _built["k"]


def test_new_kernels_use_no_scratch_and_keep_the_near_words_in_lds():
    """ScratchSize 0 (the compiler's resource report); LDS: the 24 KiB of tiles and 24 KiB of near words per packed group; the
    LDS-DMA staging; no atomics."""
    bodies, report = guard_kernels()
    assert bodies and set(report) == set(bodies), (sorted(bodies), sorted(report))
    for want in NEW:
        assert any(want in k for k in bodies), want
    res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
    fold = re.search(r"Function Name: \S*nb_mxg_fold\S*(.*?)ScratchSize \[bytes/lane\]: (\d+)", res, re.S)
    assert fold and "Function Name" not in fold.group(1) and int(fold.group(2)) == 0
    for k, (scratch, lds) in report.items():
        ng = 1 if "ILi1E" in k else 2
        assert scratch == 0 and lds == 24576 * (1 + ng), (k, scratch, lds)
    for k, v in bodies.items():
        assert "global_load_lds_dwordx4" in v and "atomic" not in v, k


def fast_path(body):
    """The instructions of the stage loop along its fast path: from the loop's header (the last label before the first
    v_rsq_f32), taking every s_cbranch_vccz that follows the OR of the compares' masks into vcc (no lane has a near pair) and every
    s_branch, to the loop's backward branch.  Returns (opcodes, the number of mask branches taken)."""
    lines = [l.split(";")[0].strip() for l in body.splitlines()]
    lines = [l for l in lines if l and (not l.startswith(".") or l.startswith(".LBB"))]
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    first = next(i for i, l in enumerate(lines) if l.startswith("v_rsq_f32"))
    start = max(i for i in labels.values() if i < first)
    i, ops, taken = start + 1, [], 0
    while len(ops) < 10000:
        l = lines[i]
        if l.endswith(":"):
            if i == start:
                break
            i += 1
            continue
        op = l.split()[0]
        ops.append(op)
        if op == "s_cbranch_vccz" and lines[i - 1].startswith("s_or_b64 vcc"):
            taken += 1
            i = labels[l.split()[1]]
        elif op == "s_branch":
            i = labels[l.split()[1]]
        elif op.startswith("s_cbranch") and labels[l.split()[1]] <= i:
            break
        else:
            i += 1
    return ops, taken


@pytest.mark.parametrize("name", NEW)
def test_fast_path_is_the_mixed_loop_plus_compares(name):
    """Along the fast path of the stage loop: per two v_rsq_f32 at most nb_mx_fj's 32 packed instructions, one v_cmp per pair whose
    mask goes to the scalar unit, one mask branch per stage (8 pairs), test_mixed_cpu's allowance of other VALU instructions (one
    in fourteen: moves), and nothing of the slow sums -- no v_cndmask, no LDS write, only the tiles' LDS reads, no global memory."""
    bodies, _ = guard_kernels()
    body = [v for k, v in bodies.items() if name in k][0]
    ops, taken = fast_path(body)
    valu = [o for o in ops if o.startswith("v_")]
    rsq = sum(o.startswith("v_rsq_f32") for o in valu)
    pk = sum(o.startswith("v_pk_") for o in valu)
    cmp_ = sum(o.startswith("v_cmp_") for o in valu)
    print("%s fast path: %d instructions, %d VALU, %d v_pk_*, %d v_rsq_f32, %d v_cmp_*, %d mask branches" % (name, len(ops), len(valu), pk, rsq, cmp_, taken))
    assert rsq >= 8 and rsq % 8 == 0 and 0 < pk <= 32 * (rsq // 2), (rsq, pk)
    assert cmp_ == rsq and taken == rsq // 8, (cmp_, taken, rsq)
    assert len(valu) - pk - rsq - cmp_ <= (pk + rsq) // 14, (len(valu), pk, rsq, cmp_)
    assert not any(o.startswith(("v_cndmask", "ds_write", "global_", "scratch_", "buffer_")) for o in ops)
    assert all(o.startswith("ds_read") for o in ops if o.startswith("ds_"))
    # the slow sums are in the loop, off that path: the selects, and the near words' LDS writes
    assert "v_cndmask_b32" in body and "ds_write" in body
