"""nb_neighbors (added within ABI 2.4) without a device: the exports, the request structure, the argument checks that come before
any device call, the binding surface, the built code of the nb_nbr* kernels (no scratch, packed arithmetic, no transcendental) and
the host logic of close_pairs."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

from nbody3d_amd import capi

CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
FIELDS = ["struct_size", "m", "flags", "first_body", "points", "radii", "radius", "index", "dist2", "count"]


def test_library_exports_the_neighbour_entry_points():
    L = capi.load_library()
    assert L.nb_abi_version() == 2 and L.nb_abi_minor() == 4          # additions within 2.4: detected by the symbol
    for name in ("nb_neighbors", "nb_multi_neighbors", "nb_neighbors_shape"):
        assert name in capi.SYMBOLS
        assert getattr(L, name) is not None
    text = open(HEADER).read()
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 9)" in text
    for flag, value in (("NB_NBR_AT_BODIES", 1), ("NB_NBR_DEVICE", 4)):
        assert re.search(r"#define %s\s+%du" % (flag, value), text), flag
        assert getattr(capi, flag) == value
    assert capi.NB_NBR_NONE == 0xffffffff


def test_request_structure_matches_the_header(tmp_path):
    """sizeof and every field offset of nb_neighbor_request as a C compiler lays the header's structure out."""
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbody3d_hip.h"\n'
                   'int main(void) { printf("%zu", sizeof(nb_neighbor_request));\n'
                   + "".join('printf(" %%zu", offsetof(nb_neighbor_request, %s));\n' % f for f in FIELDS)
                   + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    R = capi.nb_neighbor_request
    assert got == [C.sizeof(R)] + [getattr(R, f).offset for f, _ in R._fields_]
    assert [f for f, _ in R._fields_] == FIELDS
    assert C.sizeof(R) == 64


def test_null_handle_and_null_request_are_invalid_without_a_device():
    L = capi.load_library()
    req = capi.nb_neighbor_request()
    req.struct_size = C.sizeof(capi.nb_neighbor_request)
    req.m = 1
    assert L.nb_neighbors(None, C.byref(req)) == 1                      # NB_ERR_INVALID
    assert b"nb_neighbors" in L.nb_last_error(None)
    assert L.nb_neighbors(None, None) == 1
    assert L.nb_multi_neighbors(None, C.byref(req)) == 1
    assert b"nb_multi_neighbors" in L.nb_multi_last_error(None)
    assert L.nb_multi_neighbors(None, None) == 1
    assert L.nb_neighbors_shape(None, 1, None, None, None) == 1
    assert b"nb_neighbors_shape" in L.nb_last_error(None)


def test_binding_surface():
    for cls in (capi.Simulation, capi.MultiSimulation):
        assert callable(getattr(cls, "neighbors"))
    assert callable(capi.Simulation.neighbors_device) and callable(capi.Simulation.close_pairs)
    assert callable(capi.Simulation.neighbors_shape) and callable(capi.mutual_pairs)
    assert capi.ABI_MINOR == 3          # the binding still loads a 2.3 library; neighbors() asks for the symbol itself


def nbr_kernels():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    text = open(os.path.join(CSRC, "nb_engine.gfx950.s")).read()
    res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN2nb\d+nb_nbr\w+):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M)}
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+)", res, re.S):
        if "nb_nbr" in m.group(1) and "Function Name" not in m.group(2):
            scratch[m.group(1)] = int(m.group(3))
    return bodies, scratch


def test_neighbour_kernels_use_no_scratch_and_the_f32_loop_is_packed():
    bodies, scratch = nbr_kernels()
    assert bodies and set(scratch) == set(bodies), (sorted(bodies), sorted(scratch))
    assert all(v == 0 for v in scratch.values()), scratch
    for k in bodies:
        assert "scratch_" not in bodies[k], k
    f32 = [k for k in bodies if "nb_nbr_pk" in k]
    assert len(f32) == 2, f32                       # nearest only, nearest and count
    for k in f32:
        assert "v_pk_fma_f32" in bodies[k] and "global_load_lds_dwordx4" in bodies[k], k
        assert "v_rsq" not in bodies[k] and "v_sqrt" not in bodies[k], k          # nowhere, so in no loop either
    f64 = [k for k in bodies if "nb_nbr64" in k]
    assert f64 and any("nb_nbr_reduce" in k for k in bodies)
    for k in f64:            # the fp64 fused multiply-add, in whichever encoding the compiler picks (v_fmac_f64 where the addend is the destination)
        assert re.search(r"v_fmac?_f64", bodies[k]) and "v_rsq" not in bodies[k] and "v_sqrt" not in bodies[k], k


def test_close_pairs_logic_on_a_stubbed_result():
    """mutual_pairs is host code: i < j, each the other's nearest body, strictly inside the radius, sorted by i."""
    #        0  1  2  3  4  5           6  7
    index = [1, 0, 3, 4, 3, 0xffffffff, 7, 6]
    dist2 = np.array([0.25, 0.25, 0.01, 0.04, 0.04, np.inf, 1.0, 1.0], np.float32)
    pairs, d2 = capi.mutual_pairs(index, dist2, 1.0)
    assert pairs.dtype == np.uint32 and pairs.shape == (2, 2)
    assert pairs.tolist() == [[0, 1], [3, 4]]                    # 2 -> 3 is not mutual; (6, 7) sits AT the radius: strict
    assert d2.tolist() == [np.float32(0.25), np.float32(0.04)]
    pairs, d2 = capi.mutual_pairs(index, dist2, 1.5)
    assert pairs.tolist() == [[0, 1], [3, 4], [6, 7]]
    pairs, d2 = capi.mutual_pairs(index, dist2, 0.1)
    assert pairs.shape == (0, 2) and d2.shape == (0,)

    class Stub(capi.Simulation):
        def __init__(self):
            self.n = 8

        def neighbors(self, points=None, *, bodies=None, radius=None, radii=None):
            assert points is None and bodies == (0, 8)
            return np.array(index, np.uint32), dist2, None

        def __del__(self):
            pass

    pairs, d2 = Stub().close_pairs(0.6)
    assert pairs.tolist() == [[0, 1], [3, 4]] and d2.dtype == np.float32
