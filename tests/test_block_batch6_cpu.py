"""Batched block steps on order-6 handles (nb_set_block_batch6; added within ABI 2.4, round 26) without a device: the export and
the header text, the rejections that need no handle, what the binding refuses before any library call, and the built code of the
nb_blkq6_* kernels (no scratch, no floating-point atomics; the two small passes within the registers and the LDS that their
declared two waves per SIMD leave them)."""
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
NAME = "nb_set_block_batch6"


def test_library_exports_the_entry_point_and_the_header_carries_the_round():
    L = capi.load_library()
    text = open(HEADER).read()
    assert NAME in capi.SYMBOLS and NAME in text
    assert getattr(L, NAME) is not None
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 26)" in text
    assert capi.abi_minor() == 4
    assert "int nb_set_block_batch6(nb_sim *s, const nb_block_batch *cfg /* NULL: off */);" in text
    assert C.sizeof(capi.nb_block_batch) == 16


def test_rejections_that_need_no_handle():
    L = capi.load_library()
    cfg = capi.nb_block_batch()
    cfg.struct_size = C.sizeof(cfg)
    assert L.nb_set_block_batch6(None, C.byref(cfg)) == 1 and b"nb_set_block_batch6" in L.nb_last_error(None)
    assert L.nb_set_block_batch6(None, None) == 1 and b"nb_set_block_batch6" in L.nb_last_error(None)


def test_binding_refuses_bad_depth_and_small_max():
    assert callable(capi.Simulation.set_block_batch6)
    assert not hasattr(capi.MultiSimulation, "set_block_batch6")
    sim = object.__new__(capi.Simulation)      # never created: the values are refused by the binding, before any handle is touched
    sim._L = capi.load_library()
    for kw in (dict(depth=1025), dict(depth=-1), dict(small_max=1025), dict(small_max=-1), dict(small_max=0xffffffff)):
        with pytest.raises(ValueError):
            capi.Simulation.set_block_batch6(sim, **kw)


# ---- the built kernels ---------------------------------------------------------------------------------------------------------
NEW = ("nb_blkq6_predictIf", "nb_blkq6_predictId", "nb_blkq6_fjs_pkILi1E", "nb_blkq6_fjs64IdE", "nb_blkq6_correctIff", "nb_blkq6_correctIdd")
PASSES = {"nb_blkq6_fjs_pkILi1E": 2, "nb_blkq6_fjs64IdE": 2}      # the amdgpu_waves_per_eu each small pass declares
_built = {}


def batch6_kernels():
    """As test_block_batch_cpu.batch_kernels: `make asm`, then the bodies and the resource report of the kernels this round adds."""
    if not _built:
        if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
            pytest.skip("hipcc not available")
        subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
        text = open(os.path.join(CSRC, "nb_engine.gfx950.s")).read()
        res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
        pick = lambda name: "nb_blkq6_" in name
        bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN2nb\d+nb_\w+):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M) if pick(m.group(1))}
        rep = {}
        for m in re.finditer(r"Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", res, re.S):
            if pick(m.group(1)) and "Function Name" not in m.group(2):
                field = lambda k: int(re.search(re.escape(k) + r": (\d+)", m.group(2)).group(1))
                rep[m.group(1)] = dict(scratch=field("ScratchSize [bytes/lane]"), vgprs=field(" VGPRs"), agprs=field("AGPRs"), lds=int(m.group(3)))
        _built["k"] = (bodies, rep)
    return _built["k"]


def test_new_kernels_exist_and_use_no_scratch():
    bodies, rep = batch6_kernels()
    assert bodies and set(rep) == set(bodies), (sorted(bodies), sorted(rep))
    assert len(bodies) == len(NEW), sorted(bodies)          # the four kernels, each for f32 and f64 handles (one pass per precision)
    for want in NEW:
        assert any(want in k for k in bodies), want
    assert all(r["scratch"] == 0 for r in rep.values()), rep
    f32 = [v for k, v in bodies.items() if "nb_blkq6_fjs_pk" in k][0]
    assert "global_load_lds_dwordx4" in f32 and "v_rsq_f32" in f32 and "v_pk_fma_f32" in f32
    f64 = [v for k, v in bodies.items() if "nb_blkq6_fjs64" in k][0]
    assert "v_rsq_f64" in f64 and "v_fma_f64" in f64
    for k, v in bodies.items():          # no floating-point atomics anywhere in the slot
        assert not re.search(r"atomic_(add|pk_add|min|max)_f", v), k


def test_names_keep_out_of_the_sets_other_tests_select():
    """tests/test_block6_cpu.py and tests/test_block_batch_cpu.py pick kernels of the built library by these substrings."""
    bodies, _ = batch6_kernels()
    for k in bodies:
        for other in ("nb_blk6_", "nb_blkq_sched", "nb_blkq_predictI", "nb_blkq_fj_pk", "nb_blkq_fj64", "nb_blkq_correctI"):
            assert other not in k, (k, other)


@pytest.mark.parametrize("name", sorted(PASSES))
def test_small_passes_fit_their_declared_waves(name):
    """gfx950: 512 VGPRs per SIMD lane, shared by the waves of a SIMD, and 160 KiB of LDS per CU; the passes declare two waves per
    SIMD, which two workgroups of four waves per CU are."""
    _, rep = batch6_kernels()
    r = [v for k, v in rep.items() if name in k][0]
    print("%s: %s" % (name, r))
    assert r["vgprs"] + r["agprs"] <= 512 // PASSES[name], r
    assert 2 * r["lds"] <= 160 * 1024, r
