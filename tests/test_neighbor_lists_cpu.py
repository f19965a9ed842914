"""nb_neighbor_lists (added within ABI 2.4) without a device: the exports, the request structure, the argument checks that come
before any device call, the binding surface, the host helpers (lists_to_csr, pairs_from_lists, all_close_pairs), the brute-force
reference against a plain loop, and the built code of the nb_nbl_* kernels (no scratch)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

from nbody3d_amd import capi
from neighbor_lists_ref import NONE, lattice_lists, naive_lists

CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
FIELDS = ["struct_size", "m", "flags", "first_body", "points", "radii", "radius", "cap", "reserved", "list", "count", "index", "dist2"]
ENTRY = ("nb_neighbor_lists", "nb_multi_neighbor_lists", "nb_neighbor_lists_shape")


def test_library_exports_the_neighbour_list_entry_points():
    L = capi.load_library()
    assert L.nb_abi_version() == 2 and L.nb_abi_minor() == 4          # an addition within 2.4: detected by the symbol
    for name in ENTRY:
        assert name in capi.SYMBOLS
        assert getattr(L, name) is not None
    text = open(HEADER).read()
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 12)" in text
    for name in ENTRY + ("nb_neighbor_list_request",):
        assert name in text


def test_request_structure_matches_the_header(tmp_path):
    """sizeof and every field offset of nb_neighbor_list_request as a C compiler lays the header's structure out."""
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbody3d_hip.h"\n'
                   'int main(void) { printf("%zu", sizeof(nb_neighbor_list_request));\n'
                   + "".join('printf(" %%zu", offsetof(nb_neighbor_list_request, %s));\n' % f for f in FIELDS)
                   + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    R = capi.nb_neighbor_list_request
    assert got == [C.sizeof(R)] + [getattr(R, f).offset for f, _ in R._fields_]
    assert [f for f, _ in R._fields_] == FIELDS
    assert C.sizeof(R) == 80


def test_null_handle_and_null_request_are_invalid_without_a_device():
    L = capi.load_library()
    req = capi.nb_neighbor_list_request()
    req.struct_size = C.sizeof(capi.nb_neighbor_list_request)
    req.m = 1
    assert L.nb_neighbor_lists(None, C.byref(req)) == 1                 # NB_ERR_INVALID
    assert b"nb_neighbor_lists" in L.nb_last_error(None)
    assert L.nb_neighbor_lists(None, None) == 1
    assert L.nb_multi_neighbor_lists(None, C.byref(req)) == 1
    assert b"nb_multi_neighbor_lists" in L.nb_multi_last_error(None)
    assert L.nb_multi_neighbor_lists(None, None) == 1
    assert L.nb_neighbor_lists_shape(None, 1, 1, None, None, None) == 1
    assert b"nb_neighbor_lists_shape" in L.nb_last_error(None)


def test_binding_surface():
    for cls in (capi.Simulation, capi.MultiSimulation):
        assert callable(getattr(cls, "neighbor_lists"))
    assert callable(capi.Simulation.neighbor_lists_device) and callable(capi.Simulation.neighbor_lists_shape)
    assert callable(capi.Simulation.all_close_pairs) and callable(capi.lists_to_csr) and callable(capi.pairs_from_lists)
    import inspect
    sig = inspect.signature(capi.Simulation.neighbor_lists)
    assert list(sig.parameters) == ["self", "points", "bodies", "radius", "radii", "cap", "nearest"]
    assert sig.parameters["cap"].default == 64 and sig.parameters["nearest"].default is False
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("bodies", "radius", "radii", "cap", "nearest"))


def test_lists_to_csr_and_pair_extraction_on_hand_made_rows():
    #                     body 0        1             2              3 (truncated: 3 members, cap 2)   4
    lists = np.array([[1, 3], [0, 3], [NONE, NONE], [0, 1], [3, NONE]], np.uint32)
    count = np.array([2, 2, 0, 3, 1], np.uint32)
    offsets, indices, truncated = capi.lists_to_csr(lists, count)
    assert offsets.tolist() == [0, 2, 4, 4, 6, 7] and indices.dtype == np.uint32
    assert indices.tolist() == [1, 3, 0, 3, 0, 1, 3]
    assert truncated.tolist() == [False, False, False, True, False]
    with pytest.raises(ValueError) as e:
        capi.pairs_from_lists(lists, count)
    assert "cap" in str(e.value)
    lists = np.array([[1, 3, NONE], [0, 3, NONE], [NONE] * 3, [0, 1, 4], [3, NONE, NONE]], np.uint32)
    pairs = capi.pairs_from_lists(lists, count)
    assert pairs.dtype == np.uint32 and pairs.tolist() == [[0, 1], [0, 3], [1, 3], [3, 4]]
    empty = capi.pairs_from_lists(np.full((3, 2), NONE, np.uint32), np.zeros(3, np.uint32))
    assert empty.shape == (0, 2)
    with pytest.raises(ValueError):
        capi.lists_to_csr(lists, count[:3])

    class Stub(capi.Simulation):
        def __init__(self, rows):
            self.n = 5
            self.rows = rows

        def neighbor_lists(self, points=None, *, bodies=None, radius=None, radii=None, cap=64, nearest=False):
            assert points is None and bodies == (0, 5) and radius == 0.5 and cap == self.rows.shape[1]
            return self.rows, count

        def __del__(self):
            pass

    assert Stub(lists).all_close_pairs(0.5, cap=3).tolist() == [[0, 1], [0, 3], [1, 3], [3, 4]]
    with pytest.raises(ValueError):
        Stub(lists[:, :2].copy()).all_close_pairs(0.5, cap=2)


def test_reference_equals_a_plain_loop():
    rng = np.random.default_rng(50)
    b = rng.integers(-3, 4, (50, 3))
    b[7] = b[3]                                                  # a duplicate: a member at d2 = 0
    pts = rng.integers(-3, 4, (20, 3))
    radii = rng.integers(1, 5, 20)
    for cap in (1, 4, 64):
        for got, want in ((lattice_lists(b, b, np.full(50, 3), cap, skip0=0), naive_lists(b, b, np.full(50, 3), cap, skip0=0)),
                          (lattice_lists(b, pts, radii, cap), naive_lists(b, pts, radii, cap)),
                          (lattice_lists(b, b[10:30], np.full(20, 2), cap, skip0=10), naive_lists(b, b[10:30], np.full(20, 2), cap, skip0=10))):
            assert got[0].dtype == np.uint32 and got[0].shape == want[0].shape
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    lists, count = lattice_lists(b, b, np.full(50, 3), 64, skip0=0)
    assert count.max() <= 64 and 7 in lists[3] and 3 in lists[7]             # the duplicate is a member, both ways
    assert not any(k in lists[k] for k in range(50))                          # never itself
    short, count4 = lattice_lists(b, b, np.full(50, 3), 4, skip0=0)
    assert count.max() > 4 and np.array_equal(count4, count) and np.array_equal(short, lists[:, :4])      # truncation keeps the smallest


def nbl_kernels():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    text = open(os.path.join(CSRC, "nb_engine.gfx950.s")).read()
    res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN2nb\d+nb_nbl\w+):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M)}
    usage = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", res, re.S):
        if "nb_nbl" in m.group(1) and "Function Name" not in m.group(2):
            usage[m.group(1)] = (int(m.group(3)), int(m.group(4)))
    return bodies, usage


def test_list_kernels_use_no_scratch_and_the_f32_fill_pass_is_packed():
    bodies, usage = nbl_kernels()
    assert bodies and set(usage) == set(bodies), (sorted(bodies), sorted(usage))
    assert all(scratch == 0 for scratch, _ in usage.values()), usage
    for k in bodies:
        assert "scratch_" not in bodies[k], k
    f32 = [k for k in bodies if "nb_nbl_pk" in k]
    assert len(f32) == 1, f32
    assert usage[f32[0]][1] == 4, usage                              # four waves per SIMD, as the count pass
    assert "v_pk_fma_f32" in bodies[f32[0]] and "global_load_lds_dwordx4" in bodies[f32[0]]
    assert "v_rsq" not in bodies[f32[0]] and "v_sqrt" not in bodies[f32[0]]
    assert "atomic" not in bodies[f32[0]]
    f64 = [k for k in bodies if "nb_nbl64" in k]
    assert f64 and len([k for k in bodies if "nb_nbl_offsets" in k]) == 2
    for k in f64:
        assert re.search(r"v_fmac?_f64", bodies[k]) and "atomic" not in bodies[k], k
