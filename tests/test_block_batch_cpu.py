"""Batched block steps (nb_set_block_batch, nb_block_batch_stats; added within ABI 2.4, round 25) without a device: the exports
and the header text, the rejections that need no handle, what the binding refuses before any library call, and the built code of
the nb_blkq_* kernels (no scratch; the two small passes within the registers their declared waves per SIMD leave them)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

from nbody3d_amd import capi

HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
CSRC = os.path.join(ROOT, "nbody3d-webgpu_amd", "csrc")
NAMES = ("nb_set_block_batch", "nb_block_batch_stats")


def test_library_exports_the_entry_points_and_the_header_carries_the_round():
    L = capi.load_library()
    text = open(HEADER).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and name in text
        assert getattr(L, name) is not None
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 25)" in text
    assert capi.abi_minor() == 4
    for line in ("int nb_set_block_batch(nb_sim *s, const nb_block_batch *cfg /* NULL: off */);",
                 "int nb_block_batch_stats(nb_sim *s, struct nb_block_batch_stats *out, int reset);",
                 "#define NB_BLOCK_BATCH_SMALL_DEFAULT 0xffffffffu", "agree to the pass's accuracy, not bit for bit"):
        assert line in text, line
    assert capi.BLOCK_BATCH_SMALL_DEFAULT == 0xffffffff
    assert C.sizeof(capi.nb_block_batch) == 16 and C.sizeof(capi.nb_block_batch_stats) == 48


def test_rejections_that_need_no_handle():
    L = capi.load_library()
    cfg = capi.nb_block_batch()
    cfg.struct_size = C.sizeof(cfg)
    assert L.nb_set_block_batch(None, C.byref(cfg)) == 1 and b"nb_set_block_batch" in L.nb_last_error(None)
    assert L.nb_set_block_batch(None, None) == 1 and b"nb_set_block_batch" in L.nb_last_error(None)
    st = capi.nb_block_batch_stats()
    st.struct_size = C.sizeof(st)
    assert L.nb_block_batch_stats(None, C.byref(st), 0) == 1 and b"nb_block_batch_stats" in L.nb_last_error(None)


def test_binding_refuses_bad_depth_and_small_max():
    assert callable(capi.Simulation.set_block_batch) and callable(capi.Simulation.block_batch_stats)
    assert not hasattr(capi.MultiSimulation, "set_block_batch")
    sim = object.__new__(capi.Simulation)      # never created: the values are refused by the binding, before any handle is touched
    sim._L = capi.load_library()
    for kw in (dict(depth=1025), dict(depth=-1), dict(small_max=1025), dict(small_max=-1), dict(small_max=0xffffffff)):
        with pytest.raises(ValueError):
            capi.Simulation.set_block_batch(sim, **kw)


# ---- the built kernels ---------------------------------------------------------------------------------------------------------
NEW = ("nb_blkq_sched", "nb_blkq_predictIf", "nb_blkq_predictId", "nb_blkq_fj_pkILi1E", "nb_blkq_fj64IdE", "nb_blkq_correctIff", "nb_blkq_correctIdd")
PASSES = {"nb_blkq_fj_pkILi1E": 2, "nb_blkq_fj64IdE": 2}      # the amdgpu_waves_per_eu each small pass declares
_built = {}


def batch_kernels():
    """As test_mixed_cpu.mixed_kernels: `make asm`, then the resource report of the kernels this round adds."""
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
    bodies, rep = batch_kernels()
    assert bodies and set(rep) == set(bodies), (sorted(bodies), sorted(rep))
    for want in NEW:
        assert any(want in k for k in bodies), want
    assert all(r["scratch"] == 0 for r in rep.values()), rep
    f32 = [v for k, v in bodies.items() if "nb_blkq_fj_pk" in k][0]
    assert "global_load_lds_dwordx4" in f32 and "v_rsq_f32" in f32 and "v_pk_fma_f32" in f32
    f64 = [v for k, v in bodies.items() if "nb_blkq_fj64" in k][0]
    assert "v_rsq_f64" in f64 and "v_fma_f64" in f64
    for k, v in bodies.items():          # no floating-point atomics anywhere in the slot
        assert not re.search(r"atomic_(add|pk_add|min|max)_f", v), k


@pytest.mark.parametrize("name", sorted(PASSES))
def test_small_passes_fit_their_declared_waves(name):
    """gfx950: 512 VGPRs per SIMD lane, shared by the waves of a SIMD, and 160 KiB of LDS per CU; the passes declare two waves per
    SIMD, which two workgroups of four waves per CU are."""
    _, rep = batch_kernels()
    r = [v for k, v in rep.items() if name in k][0]
    print("%s: %s" % (name, r))
    assert r["vgprs"] + r["agprs"] <= 512 // PASSES[name], r
    assert 2 * r["lds"] <= 160 * 1024, r
