"""The encounter watch of block steps (nb_set_encounter_watch; added within ABI 2.4, round 28) without a device: the exports and the
header text, the rejections that need no handle, what the binding refuses before any library call, the CPU restatement
(tests/encounter_ref.py) against the O(n^2) int64 brute force on the census lattice, the restatement's own distance from the
analytic pericentre (the GPU test's tolerance is twice it), and the built code of the three new kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from nbody3d_amd import capi

import encounter_ref as E

HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
CSRC = os.path.join(ROOT, "nbody3d-webgpu_amd", "csrc")
NAMES = ("nb_set_encounter_watch", "nb_encounter_stats", "nb_download_encounters", "nb_upload_encounters", "nb_reset_encounters")


def test_library_exports_the_entry_points_and_the_header_carries_the_round():
    L = capi.load_library()
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and name in text and getattr(L, name) is not None, name
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 28)" in text and capi.abi_minor() == 4
    assert "int nb_set_encounter_watch(nb_sim *s, const nb_encounter_watch *cfg /* NULL: off */);" in text
    assert "enum { NB_ENC_STOP = 1u };" in text and capi.NB_ENC_STOP == 1
    assert C.sizeof(capi.nb_encounter_watch) == 24 and C.sizeof(capi.nb_encounter_stats) == 32
    assert capi.nb_encounter_watch.radii.offset == 8 and capi.nb_encounter_watch.flags.offset == 16
    assert capi.nb_encounter_stats.first_time.offset == 16 and capi.nb_encounter_stats.steps_left.offset == 28


def test_rejections_that_need_no_handle():
    L = capi.load_library()
    cfg = capi.nb_encounter_watch()
    st = capi.nb_encounter_stats()
    calls = (lambda: L.nb_set_encounter_watch(None, C.byref(cfg)), lambda: L.nb_set_encounter_watch(None, None),
             lambda: L.nb_encounter_stats(None, C.byref(st), 0), lambda: L.nb_download_encounters(None, None, None, None, None),
             lambda: L.nb_upload_encounters(None, None, None, None, None), lambda: L.nb_reset_encounters(None))
    for name, call in zip((NAMES[0],) + NAMES, calls):
        assert call() == 1 and name.encode() in L.nb_last_error(None), name


def test_binding_refuses_bad_arguments():
    for m in ("set_encounter_watch", "encounter_stats", "download_encounters", "upload_encounters", "reset_encounters"):
        assert callable(getattr(capi.Simulation, m)) and not hasattr(capi.MultiSimulation, m), m
    sim = object.__new__(capi.Simulation)      # never created: the values are refused by the binding, before any handle is touched
    sim._L, sim.n, sim.dtype = capi.load_library(), 4, np.float32
    bad = (dict(), dict(radius=0.1, radii=np.zeros(4)), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
           dict(radius="x"), dict(radii=np.zeros(3)), dict(radii=[0, 1, -1, 0]), dict(radii=[0, 1, np.nan, 0]))
    for kw in bad:
        with pytest.raises(ValueError):
            capi.Simulation.set_encounter_watch(sim, **kw)
    ok = np.zeros(4)
    for args in ((ok[:3], ok, ok, ok), (ok, ok[:3], ok, ok), (ok, ok, ok[:3], ok), (ok, ok, ok, ok[:3])):
        with pytest.raises(ValueError):
            capi.Simulation.upload_encounters(sim, *args)


# ---- the restatement against the brute force -----------------------------------------------------------------------------------
def test_thresholds_are_exact_on_the_lattice():
    for case in E.LATTICE_CASES:
        rad = E.lattice_radii(1025, case)
        w64, w32 = E.thresholds(rad, E.LATTICE_EPS2, np.float64), E.thresholds(rad, E.LATTICE_EPS2, np.float32)
        assert np.array_equal(w64, w32.astype(np.float64)) and np.array_equal(w64[rad > 0], (rad * rad + E.LATTICE_EPS2)[rad > 0])
        assert not w64[rad == 0].any()
    assert (E.lattice_radii(1025, "per_body") == 0).sum() > 100


def test_lattice_holds_what_the_census_needs():
    for n in (1025, 4099):
        b, v, pairs = E.lattice(n)
        x = b[:, :3].astype(np.int64)
        assert np.array_equal(x, b[:, :3]) and x.min() >= 0 and x.max() < 64 and not v.any()
        assert not x[0].any() and tuple(x[1]) == (1, 0, 0)
        sites, counts = np.unique(x, axis=0, return_counts=True)
        assert len(sites) == n - 4 and sorted(counts)[-4:] == [2, 2, 2, 2] and len(pairs) == 4
        assert all(i != j and np.array_equal(x[i], x[j]) for i, j in pairs)
        assert any(min(i, j) < 256 and max(i, j) >= n - n % 256 for i, j in pairs)      # first and last tile: different j-chunks
        assert n % 256 in (1, 3)


@pytest.mark.parametrize("second", [False, True])
def test_restatement_equals_the_brute_force(second):
    n = 1025
    b, v, _ = E.lattice(n)
    lev = E.lattice_levels(n, second)
    zero = np.zeros((n, 3))
    for case, store in ((c, s) for c in E.LATTICE_CASES for s in ((np.float32, np.float64) if not second else (np.float32,))):
        rad = E.lattice_radii(n, case)
        out, rec, st = E.watch_ref(b, v, 0.0, E.LATTICE_EPS2, E.LATTICE_DT, 1, rad, store=store, max_level=E.LATTICE_L, levels=lev,
                                   frozen=True, aj=(zero, zero))
        want, hits, passes = E.lattice_brute(b, lev, rad)
        assert np.array_equal(out[0], b)                           # nothing moved
        for k in want:
            assert np.array_equal(np.asarray(rec[k], want[k].dtype), want[k]), (case, store, k)
        assert st["hits"] == hits > 0 and st["passes"] == passes == 8 and st["first_time"] == want["time"].min()
        have = want["partner"] != E.NONE
        assert np.array_equal(want["count"][have], 2 ** lev[have].astype(np.int64)) and not want["count"][~have].any()
        assert want["partner"][0] == 1 and want["rho2"][0] == 1.25 or rad[0] < 1
    if not second:
        want = E.lattice_brute(b, lev, E.lattice_radii(n, "coincident"))[0]
        assert sorted(np.nonzero(want["partner"] != E.NONE)[0]) == sorted(i for p in E.lattice(n)[2] for i in p)
        assert np.all(want["rho2"][want["partner"] != E.NONE] == E.LATTICE_EPS2)


def test_the_restatement_sees_the_pericentre():
    """The distance the GPU test doubles for its tolerance: the restatement's recorded rho2 - eps2 of the second passage against
    (a (1 - e))^2; the passage falls inside outer step 16, and the record's time is the sample next to t = 2 pi."""
    b0, v0, out, rec, st = E.kepler_watch_ref()
    k = E.KEPLER
    d = np.abs(rec["rho2"] - k["eps2"] - E.PERICENTRE2)
    print("kepler restatement: rho2 - eps2 = %s at t = %s outer steps (2 pi / dt = %.6f), distance %s, %d hits in %d passes"
          % (rec["rho2"] - k["eps2"], rec["time"], 2 * np.pi / k["dt"], d, st["hits"], st["passes"]))
    assert np.array_equal(rec["partner"], [1, 0]) and rec["time"][0] == rec["time"][1]
    assert k["outer"] - 1 < rec["time"][0] < k["outer"] and abs(rec["time"][0] * k["dt"] - 2 * np.pi) < 1e-3
    assert np.allclose(d, E.KEPLER_DISTANCE, rtol=1e-3, atol=0)


# ---- the built kernels ---------------------------------------------------------------------------------------------------------
NEW = ("nb_enc_fj_pkILi2E", "nb_enc_fj_pkILi1E", "nb_enc_fj64IdE", "nb_enc_foldIff", "nb_enc_foldIdd")
_built = {}


def enc_kernels():
    if not _built:
        if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
            pytest.skip("hipcc not available")
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
        text = open(os.path.join(CSRC, "nb_engine.gfx950.s")).read()
        res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
        pick = lambda name: "nb_enc_" in name
        bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN2nb\d+nb_\w+):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M) if pick(m.group(1))}
        rep = {}
        for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", res, re.S):
            if pick(m.group(1)) and "Function Name" not in m.group(2):
                field = lambda k: int(re.search(re.escape(k) + r": (\d+)", m.group(2)).group(1))
                rep[m.group(1)] = dict(scratch=field("ScratchSize [bytes/lane]"), vgprs=field(" VGPRs"), agprs=field("AGPRs"), lds=int(m.group(3)))
        _built["k"] = (bodies, rep)
    return _built["k"]


def test_new_kernels_fit_their_budget():
    """<= 256 VGPRs at the two waves per SIMD the f32 passes declare, no scratch; the watch's words sit in LDS beside the 16 KiB of
    tiles (12 B x 2 NG per lane); no floating-point atomics anywhere."""
    bodies, rep = enc_kernels()
    assert set(rep) == set(bodies) and len(bodies) == len(NEW), sorted(bodies)
    for want in NEW:
        assert any(want in k for k in bodies), want
    for k, r in rep.items():
        print(k, r)
        assert r["scratch"] == 0 and r["vgprs"] + r["agprs"] <= 256, (k, r)
    for ng in (1, 2):
        k = [k for k in bodies if "nb_enc_fj_pkILi%dE" % ng in k][0]
        assert rep[k]["lds"] == 16384 + 3 * 8 * ng * 256 and 2 * rep[k]["lds"] <= 160 * 1024
        assert "global_load_lds_dwordx4" in bodies[k] and "v_cmp_lt_f32" in bodies[k] and "v_pk_fma_f32" in bodies[k]
    for k, v in bodies.items():
        assert not re.search(r"atomic_(add|pk_add|min|max)_f", v), k


def no_hit_path(body):
    """The instructions of one trip round the innermost loop on the path WITHOUT a hit: from the first skip of a slow path
    (s_cbranch_vccz, taken), following unconditional branches and back edges, until the walk returns to where it began."""
    lines = [l.split(";")[0].strip() for l in body.splitlines()]
    lines = [l for l in lines if l and (not l.startswith(".") or l.startswith(".LBB"))]
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    for start in (i for i, l in enumerate(lines) if l.startswith("s_cbranch_vccz")):
        i, ops = start, []
        for _ in range(5000):
            l = lines[i]
            if not l.endswith(":"):
                ops.append(l.split()[0])
            m = re.match(r"(s_cbranch_vccz|s_branch|s_cbranch_scc[01])\s+(\S+)", l)
            if m and m.group(2) in labels and (not m.group(1).startswith("s_cbranch_scc") or labels[m.group(2)] < i):
                i = labels[m.group(2)]      # a skip of the slow path, a jump, a back edge: taken; the loop's exit: not
            else:
                i += 1
            if i == start:
                if any(o.startswith("v_rsq_f32") for o in ops):
                    return ops
                break
            if i >= len(lines):
                break
    raise AssertionError("no loop found behind a skip of the slow path")


def test_the_hot_loop_gains_compares_and_one_branch_per_stage():
    """The innermost loops of nb_enc_fj_pk<NG> against nb_blk_fj_pk<NG>: the same packed arithmetic and reciprocal roots; on the path
    without a hit a stage of four chains (8 v_rsq_f32) has exactly eight v_cmp_lt_f32 (one per packed half), their masks ORed on the
    scalar unit by seven s_or_b64, and ONE s_cbranch_vccz over the slow path."""
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    enc_kernels()
    text = open(os.path.join(CSRC, "nb_engine.gfx950.s")).read()
    body = lambda name: re.search(r"^_ZN2nb\d+%s\w*:.*?$(.*?)^\.Lfunc_end" % name, text, re.S | re.M).group(1)
    count = lambda s, op: len(re.findall(r"^\s+%s\b" % op, s, re.M))
    for ng in (1, 2):
        enc, blk = body("nb_enc_fj_pkILi%dE" % ng), body("nb_blk_fj_pkILi%dE" % ng)
        assert count(enc, "v_pk_fma_f32") == count(blk, "v_pk_fma_f32") and count(enc, "v_rsq_f32_e64") == count(blk, "v_rsq_f32_e64")
        ops = no_hit_path(enc)
        n = lambda head: sum(o.startswith(head) for o in ops)
        stages = n("v_rsq_f32") // 8
        print("NG=%d, the path without a hit: %d instructions, %d stages, %d v_pk_*, %d v_cmp_lt_f32, %d s_or_b64, %d s_cbranch_vccz, %d LDS, %d global"
              % (ng, len(ops), stages, n("v_pk_"), n("v_cmp_lt_f32"), n("s_or_b64"), n("s_cbranch_vccz"), n("ds_"), n("global_")))
        assert stages >= 1 and n("v_rsq_f32") == 8 * stages
        assert n("v_cmp_lt_f32") == 8 * stages and n("s_or_b64") == 7 * stages and n("s_cbranch_vccz") == stages
        assert n("v_pk_") == 104 * stages and not n("ds_write") and not n("global_store")
