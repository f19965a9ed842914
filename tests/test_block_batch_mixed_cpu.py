"""Batched block steps on mixed-precision handles (nb_set_block_batch_mixed; added within ABI 2.4, round 27) without a device: the
export and the header text, the rejections that need no handle, what the binding refuses before any library call, the built code
of the slot's three new launches (nb_blkqm_predict, nb_blkqm_fj<1>, nb_blkq_correct<float, double>: no scratch, no floating-point
atomics, the pass's inner loop is the double-single pair arithmetic and fits the two waves per SIMD it declares), and the census
condition the GPU test's two-tile case relies on."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from nbody3d_amd import capi

import block_ref as R
import mixed_ref as M
import block_batch_mixed_ref as Q

HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
CSRC = os.path.join(ROOT, "nbody3d-webgpu_amd", "csrc")
NAME = "nb_set_block_batch_mixed"


def test_library_exports_the_entry_point_and_the_header_carries_the_round():
    L = capi.load_library()
    text = open(HEADER).read()
    assert NAME in capi.SYMBOLS and NAME in text
    assert getattr(L, NAME) is not None
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 27)" in text
    assert re.search(r"2\.4 \(round 27\) likewise within 2\.4: nb_set_block_batch_mixed\.  Detected by the presence of the symbol", text)
    assert capi.abi_minor() == 4
    assert "int nb_set_block_batch_mixed(nb_sim *s, const nb_block_batch *cfg /* NULL: off */);" in text
    assert C.sizeof(capi.nb_block_batch) == 16


def test_rejections_that_need_no_handle():
    L = capi.load_library()
    cfg = capi.nb_block_batch()
    cfg.struct_size = C.sizeof(cfg)
    assert L.nb_set_block_batch_mixed(None, C.byref(cfg)) == 1 and b"nb_set_block_batch_mixed" in L.nb_last_error(None)
    assert L.nb_set_block_batch_mixed(None, None) == 1 and b"nb_set_block_batch_mixed" in L.nb_last_error(None)


def test_binding_refuses_bad_depth_and_small_max():
    assert callable(capi.Simulation.set_block_batch_mixed)
    assert not hasattr(capi.MultiSimulation, "set_block_batch_mixed")
    sim = object.__new__(capi.Simulation)      # never created: the values are refused by the binding, before any handle is touched
    sim._L = capi.load_library()
    for kw in (dict(depth=1025), dict(depth=-1), dict(small_max=1025), dict(small_max=-1), dict(small_max=0xffffffff)):
        with pytest.raises(ValueError):
            capi.Simulation.set_block_batch_mixed(sim, **kw)


# ---- the built kernels ---------------------------------------------------------------------------------------------------------
NEW = ("nb_blkqm_predict", "nb_blkqm_fjILi1E", "nb_blkq_correctIfd")
PASS = "nb_blkqm_fjILi1E"
WAVES = 2                                      # the amdgpu_waves_per_eu the pass declares
# how the other CPU tests pick kernels of the built library: substrings of the mangled name, or the head of the kernel's own name
OTHERS = {"test_block_batch_cpu": ("nb_blkq_sched", "nb_blkq_predictIf", "nb_blkq_predictId", "nb_blkq_fj_pkILi1E", "nb_blkq_fj64IdE",
                                   "nb_blkq_correctIff", "nb_blkq_correctIdd", "nb_blkq_fj_pk", "nb_blkq_fj64"),
          "test_block_batch6_cpu": ("nb_blkq6_",),
          "test_mixed_cpu": ("nb_mx_split", "nb_mx_predict", "nb_mx_blk_predict", "nb_mx_fjILi2E", "nb_mx_blk_fjILi2E", "nb_mx_blk_fjILi1E",
                             "nb_fj_reduceIfdE", "nb_blk_correctIfdE", "nb_mx_fj", "nb_mx_blk_fj"),
          "test_guard_cpu": ("nb_mxg_fjILi2E", "nb_mxg_blk_fjILi2E", "nb_mxg_blk_fjILi1E")}
HEADS = {"test_block_cpu": ("nb_blk_",), "test_hermite_cpu": ("nb_fj", "nb_hermite")}
_built = {}


def batch_mixed_kernels():
    """As test_block_batch6_cpu.batch6_kernels: `make asm`, then the bodies and the resource report of the kernels this round adds."""
    if not _built:
        if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
            pytest.skip("hipcc not available")
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
        text = open(os.path.join(CSRC, "nb_engine.gfx950.s")).read()
        res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
        pick = lambda name: any(w in name for w in NEW)
        bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN2nb\d+nb_\w+):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M) if pick(m.group(1))}
        rep = {}
        for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", res, re.S):
            if pick(m.group(1)) and "Function Name" not in m.group(2):
                field = lambda k: int(re.search(re.escape(k) + r": (\d+)", m.group(2)).group(1))
                rep[m.group(1)] = dict(scratch=field("ScratchSize [bytes/lane]"), vgprs=field(" VGPRs"), agprs=field("AGPRs"), lds=int(m.group(3)))
        _built["k"] = (bodies, rep)
    return _built["k"]


def test_new_kernels_exist_and_use_no_scratch():
    bodies, rep = batch_mixed_kernels()
    assert bodies and set(rep) == set(bodies), (sorted(bodies), sorted(rep))
    assert len(bodies) == len(NEW), sorted(bodies)
    for want in NEW:
        assert any(want in k for k in bodies), want
    assert all(r["scratch"] == 0 for r in rep.values()), rep
    fj = [v for k, v in bodies.items() if PASS in k][0]
    assert "global_load_lds_dwordx4" in fj and "v_rsq_f32" in fj and "v_pk_fma_f32" in fj
    for k, v in bodies.items():          # no floating-point atomics anywhere in the slot
        assert not re.search(r"atomic_(add|pk_add|min|max)_f", v), k


def test_names_keep_out_of_the_sets_other_tests_select():
    bodies, _ = batch_mixed_kernels()
    for k in bodies:
        name = re.match(r"_ZN2nb\d+(nb_\w+)", k).group(1)
        for test, words in OTHERS.items():
            for w in words:
                assert w not in k, (k, test, w)
        for test, heads in HEADS.items():
            for w in heads:
                assert not name.startswith(w), (k, test, w)


def test_the_small_pass_fits_its_declared_waves():
    """gfx950: 512 VGPRs per SIMD lane, shared by the waves of a SIMD, and 160 KiB of LDS per CU; the pass declares two waves per
    SIMD, which two workgroups of four waves per CU are.  36 KiB of LDS: 24 KiB of tiles and 12 KiB of the waves' sums."""
    _, rep = batch_mixed_kernels()
    r = [v for k, v in rep.items() if PASS in k][0]
    print("%s: %s" % (PASS, r))
    assert r["vgprs"] + r["agprs"] <= 512 // WAVES, r
    assert r["lds"] == 36 * 1024 and 2 * r["lds"] <= 160 * 1024, r


def test_the_small_pass_loop_is_the_pair_arithmetic():
    """test_mixed_cpu's rule on the innermost loop of nb_blkqm_fj<1>: per two v_rsq_f32 at most 32 packed instructions (nb_fj_pk's 26
    and the six of the double-single difference), at most one more VALU instruction in fourteen around them, nothing that touches
    global memory.  Built: 256 packed + 16 v_rsq_f32 + 11 others = 283 vector instructions per 16 pairs of rows, where
    nb_blkq_fj_pk<1> has 208 + 16 + 11 = 235 (x 1.20)."""
    bodies, _ = batch_mixed_kernels()
    body = [v for k, v in bodies.items() if PASS in k][0]
    lines = [l.split(";")[0].strip() for l in body.splitlines()]
    lines = [l for l in lines if l and (not l.startswith(".") or l.startswith(".LBB"))]
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"s_cbranch_\w+\s+(\S+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append(lines[labels[m.group(1)]:i + 1])
    inner = [lp for lp in loops if not any(o is not lp and len(o) < len(lp) and o[0] in lp for o in loops)]
    plain = [lp for lp in inner if any(o.startswith("v_rsq_f32") for o in lp)]      # (its own counter is a vector compare: a wave's rows start at 64 x wave)
    assert len(plain) == 1, [len(lp) for lp in inner]
    for lp in plain:
        ops = [l.split()[0] for l in lp if not l.endswith(":")]
        valu = [o for o in ops if o.startswith("v_")]
        rsq = sum(o.startswith("v_rsq_f32") for o in valu)
        pk = sum(o.startswith("v_pk_") for o in valu)
        print("%s inner loop: %d instructions, %d VALU, %d v_pk_*, %d v_rsq_f32" % (PASS, len(ops), len(valu), pk, rsq))
        assert rsq >= 8 and rsq % 2 == 0 and 0 < pk <= 32 * (rsq // 2), (rsq, pk)
        assert len(valu) - pk - rsq <= (pk + rsq) // 14, (len(valu), pk, rsq)
        assert not any(o.startswith("global_") for o in ops)


# ---- the census condition of the two-tile case ---------------------------------------------------------------------------------
def test_chunk_rule_gives_two_tiles_and_a_ragged_chunk():
    for cus in (2, 64, 104, 256, 304):
        n = 256 * cus + 257
        chunks, per = Q.bb_shape(n, cus)
        assert per == 512 and chunks == -(-n // 512) and n - (chunks - 1) * per == 257, (cus, chunks, per)
    assert Q.bb_shape(1025, 256) == (5, 256) and Q.bb_shape(2, 256) == (1, 256) and Q.bb_shape(65536, 256) == (256, 256)


def test_one_missed_or_doubled_heavy_row_misses_the_gpu_bound():
    """The GPU test holds the velocities of the 64 small-step bodies of the two-tile system to max(1e-9, FACTOR x the distance
    between the mixed handle without the mode and a native handle).  That distance is estimated here from the restatements: the
    two handles' passes differ on the active rows by d = fj_mixed (the kernel's binary32 sums) - fj_ref, the start and the two
    block steps of the outer step each take such a difference into v by at most h / 2 |d| (the jerk's h^2 / 12 share is smaller), so
    the distance is at most 2 h max |d| / max |v|.  Leaving out or doubling any ONE heavy row moves the corrected velocity of at
    least one active body by at least 4 x the bound (Q.census_moves); the GPU test asserts the same with the bound it measures."""
    system = Q.two_tile_system()
    n, b0, v0, lev, heavy = system
    act = np.nonzero(lev == 1)[0]
    assert n == 65793 and len(act) == Q.ACTIVE and len(heavy) == 7 + 257
    assert np.allclose(b0[heavy, 3], Q.HEAVY / n) and np.allclose(np.delete(b0[:, 3], heavy), 1.0 / n)
    assert M.split(b0, v0)[1].any(axis=1).mean() > 0.9            # the lo words are in play
    am, _ = M.fj_mixed(b0, v0, 1.0, Q.EPS2, rows=act)
    ar, _ = R.fj_ref(b0, v0, 1.0, Q.EPS2, act)
    d = np.abs(am - ar[:, :3]).max()
    bound = max(1e-9, M.FACTOR * 2 * (Q.DT / 2) * d / np.abs(v0[act, :3]).max())
    moves = Q.census_moves(system)
    print("two-tile census, N=%d: pass difference %.3g of max |a| %.3g, estimated bound %.3g; one heavy row moves a velocity by %.3g .. %.3g (x %.1f the bound at least)"
          % (n, d, np.abs(ar).max(), bound, moves.min(), moves.max(), moves.min() / bound))
    assert moves.min() >= 4 * bound, (moves.min(), bound, heavy[np.argmin(moves)])
