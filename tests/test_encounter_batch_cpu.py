"""The encounter watch inside batched block steps (nb_set_block_batch_watch; added within ABI 2.4, round 29) without a device: the
export and the header text, the rejection that needs no handle, what the binding refuses before any library call, the census
inputs (which block steps are small, where the ties sit), and the built code of the four new kernels against the unwatched
small kernels they share their bodies with."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from nbody3d_amd import capi

import encounter_ref as E
import encounter_batch_ref as B

HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
CSRC = os.path.join(ROOT, "nbody3d-webgpu_amd", "csrc")
NAME = "nb_set_block_batch_watch"


def test_library_exports_the_entry_point_and_the_header_carries_the_round():
    L = capi.load_library()
    text = open(HEADER).read()
    assert NAME in capi.SYMBOLS and getattr(L, NAME) is not None
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 29) likewise within 2.4: nb_set_block_batch_watch." in text
    assert "int nb_set_block_batch_watch(nb_sim *s, const nb_block_batch *cfg /* NULL: off */);" in text
    assert "Not built: the watch in batched slots" not in text
    # nothing of the watch's or the batch's structs moved
    assert C.sizeof(capi.nb_encounter_watch) == 24 and C.sizeof(capi.nb_encounter_stats) == 32 and capi.NB_ENC_STOP == 1
    assert C.sizeof(capi.nb_block_batch) == 16


def test_rejection_that_needs_no_handle():
    L = capi.load_library()
    cfg = capi.nb_block_batch()
    cfg.struct_size = C.sizeof(cfg)
    for call in (lambda: L.nb_set_block_batch_watch(None, C.byref(cfg)), lambda: L.nb_set_block_batch_watch(None, None)):
        assert call() == 1 and NAME.encode() in L.nb_last_error(None)


def test_binding_refuses_bad_arguments():
    assert callable(capi.Simulation.set_block_batch_watch) and not hasattr(capi.MultiSimulation, "set_block_batch_watch")
    sim = object.__new__(capi.Simulation)      # never created: the values are refused by the binding, before any handle is touched
    sim._L, sim.n, sim.dtype = capi.load_library(), 4, np.float32
    for kw in (dict(depth=1025), dict(depth=-1), dict(depth="x"), dict(small_max=1025), dict(small_max=-1), dict(small_max="x"),
               dict(bogus=1)):
        with pytest.raises((ValueError, TypeError)):
            capi.Simulation.set_block_batch_watch(sim, **kw)
        with pytest.raises((ValueError, TypeError)):      # ... exactly as set_block_batch does
            capi.Simulation.set_block_batch(sim, **kw)


# ---- the census inputs ---------------------------------------------------------------------------------------------------------
def test_the_level_sets_take_the_paths_the_census_names():
    lev = E.lattice_levels(1025)
    assert B.active_counts(lev) == [256, 512, 256, 768, 256, 512, 256, 1025] and B.expected_path(lev, 1024) == (7, 1)
    lev = E.lattice_levels(4099)
    assert B.active_counts(lev)[0::2] == [1024] * 4 and min(B.active_counts(lev)[1::2]) > 1024
    assert B.expected_path(lev, 1024) == (4, 4) and B.expected_path(lev, 1023) == (0, 8)
    lev = B.small_set_levels(1025, 129, 127)
    assert B.active_counts(lev) == [129, 256, 129, 257, 129, 256, 129, 1025] and B.expected_path(lev, 256) == (6, 2)
    assert all(lev[i] == 3 for i in B.CORE)
    lev = B.small_set_levels(1025, 1, 63)
    assert B.active_counts(lev) == [1, 64, 1, 65, 1, 64, 1, 1025] and B.expected_path(lev, 64) == (6, 2) and lev[0] == 3
    # chunks against the 16 sum lanes of the small corrector, with the CU count of an MI355X
    assert B.bb_shape(1025, 256)[0] == 5 and B.bb_shape(4099, 256)[0] == 17 and B.bb_shape(66307, 256) == (130, 512)


def test_the_lattice_holds_the_ties_the_merges_need():
    b, _, pairs = E.lattice(1025)
    quarter, tile = B.ties(b, E.lattice_radii(1025, "one"))
    print("h = 4: %d bodies tied between quarters of one tile %s, %d between tiles" % (len(quarter), quarter, len(tile)))
    assert {60, 67, 185, 645} <= set(quarter) and {1, 97, 98, 112} <= set(tile) and len(tile) >= 20
    assert {i for p in pairs for i in p} <= set(B.CORE) and {60, 67} <= set(B.CORE)


# ---- the built kernels ---------------------------------------------------------------------------------------------------------
NEW = ("nb_encq_fj_pkILi1E", "nb_encq_fj64IdE", "nb_encq_correctIff", "nb_encq_correctIdd")


def pick(d, part):
    got = [k for k in d if part in k]
    assert len(got) == 1, (part, got)
    return d[got[0]]


def count(s, op):
    return len(re.findall(r"^\s+%s\b" % op, s, re.M))


def test_new_kernels_fit_their_budget():
    """Two waves per SIMD as the small passes declare, <= 256 VGPRs + AGPRs, no scratch, two workgroups' LDS within 160 KiB; no
    floating-point atomics anywhere.  The earlier kernels picked by name stay as many as they were."""
    _, bodies, rep = B.built(CSRC)
    assert sorted(k for k in bodies if "nb_encq_" in k) == sorted(k for k in rep if "nb_encq_" in k)
    assert len([k for k in bodies if "nb_encq_" in k]) == len(NEW)
    assert len([k for k in bodies if "nb_enc_" in k]) == 5
    for want in NEW:
        r = pick(rep, want)
        print(want, r)
        assert r["scratch"] == 0 and r["vgprs"] + r["agprs"] <= 256 and 2 * r["lds"] <= 160 * 1024, (want, r)
        assert not re.search(r"atomic_(add|pk_add|min|max)_f", pick(bodies, want)), want
    for want in NEW[:2]:
        assert pick(rep, want)["occupancy"] == 2
    # the bests of the four waves beside red: 4 x (4 + 4) B per slot
    assert pick(rep, NEW[0])["lds"] == pick(rep, "nb_blkq_fj_pkILi1E")["lds"] + 4 * 8 * 128
    assert pick(rep, NEW[1])["lds"] == pick(rep, "nb_blkq_fj64IdE")["lds"] + 4 * 12 * 64
    for want in NEW[2:]:      # the fold's integer atomics are in the corrector: a count and a minimum
        assert "atomic_add_x2" in pick(bodies, want) and "atomic_umin_x2" in pick(bodies, want)


def test_the_f32_hot_loop_gains_compares_and_one_branch_per_stage():
    """nb_encq_fj_pk<1> against nb_blkq_fj_pk<1>: the same packed arithmetic and reciprocal roots; on the path without a hit a stage
    of four chains (8 v_rsq_f32) has eight v_cmp_lt_f32 (one per packed half) and ONE s_cbranch_vccz over the slow path."""
    _, bodies, _ = B.built(CSRC)
    enc, blk = pick(bodies, "nb_encq_fj_pkILi1E"), pick(bodies, "nb_blkq_fj_pkILi1E")
    assert count(enc, "v_pk_fma_f32") == count(blk, "v_pk_fma_f32") > 0
    assert count(enc, "v_rsq_f32_e64") + count(enc, "v_rsq_f32_e32") == count(blk, "v_rsq_f32_e64") + count(blk, "v_rsq_f32_e32") > 0
    assert count(blk, "v_cmp_lt_f32") == 0 and "global_load_lds_dwordx4" in enc
    ops = B.no_hit_path(enc, "v_rsq_f32")
    n = lambda head: sum(o.startswith(head) for o in ops)
    stages = n("v_rsq_f32") // 8
    print("the path without a hit: %d instructions, %d stages, %d v_pk_*, %d v_cmp_lt_f32, %d s_or_b64, %d s_cbranch_vccz, %d LDS writes"
          % (len(ops), stages, n("v_pk_"), n("v_cmp_lt_f32"), n("s_or_b64"), n("s_cbranch_vccz"), n("ds_write")))
    assert stages >= 1 and n("v_rsq_f32") == 8 * stages
    assert n("v_cmp_lt_f32") == 8 * stages and n("s_cbranch_vccz") == stages
    assert not n("ds_write") and not n("global_store")


def test_the_f64_pass_keeps_its_arithmetic():
    """nb_encq_fj64 against nb_blkq_fj64: as many fused multiply-adds (in either encoding, and each encoding by itself) and as
    many reciprocal roots -- the watched loop is unrolled as the unwatched one is -- and compares the unwatched pass has none of."""
    _, bodies, _ = B.built(CSRC)
    enc, blk = pick(bodies, "nb_encq_fj64IdE"), pick(bodies, "nb_blkq_fj64IdE")
    for op in (r"v_fma_f64", r"v_fmac_f64\w*", r"v_fmac?_f64\w*", r"v_rsq_f64\w*", r"v_mul_f64\w*"):
        print(op, count(enc, op), count(blk, op))
        assert count(enc, op) == count(blk, op) > 0, op
    assert count(enc, r"v_cmp_lt_f64\w*") > 0 and count(blk, r"v_cmp_\w+_f64\w*") == 0
