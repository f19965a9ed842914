"""nb_split_lists (added within ABI 2.4) without a device: the exports, the request structure, the argument checks that come before any
device call, the binding surface and the built code of the nb_spl* kernels (no scratch at the waves per SIMD nb_split_pk is
compiled for; the kernels it restates and the list kernels keep their registers)."""
import ctypes as C
import inspect
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
FIELDS = ["struct_size", "m", "flags", "first_body", "points", "point_vel", "radii", "radius", "accel_irr", "accel_reg", "jerk_irr", "jerk_reg",
          "cap", "reserved", "list", "count"]
ENTRY = ("nb_split_lists", "nb_multi_split_lists", "nb_split_lists_shape", "nb_neighbor_scheme_fused")


def test_library_exports_the_split_lists_entry_points():
    L = capi.load_library()
    assert L.nb_abi_version() == 2 and L.nb_abi_minor() == 4          # an addition within 2.4: detected by the symbol
    for name in ENTRY:
        assert name in capi.SYMBOLS
        assert getattr(L, name) is not None
    text = open(HEADER).read()
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 17)" in text
    for name in ENTRY + ("nb_split_lists_request",):
        assert name in text
    assert re.search(r"#define NB_FLAG_AC_TWO_CALLS 4096u", text) and capi.NB_FLAG_AC_TWO_CALLS == 4096
    assert "none defined: must be 0" in text                            # nb_neighbor_scheme.flags stays as it was


def test_request_structure_matches_the_header(tmp_path):
    """sizeof and every field offset of nb_split_lists_request as a C compiler lays the header's structure out."""
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbody3d_hip.h"\n'
                   'int main(void) { printf("%zu", sizeof(nb_split_lists_request));\n'
                   + "".join('printf(" %%zu", offsetof(nb_split_lists_request, %s));\n' % f for f in FIELDS)
                   + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    Q = capi.nb_split_lists_request
    assert got == [C.sizeof(Q)] + [getattr(Q, f).offset for f, _ in Q._fields_]
    assert [f for f, _ in Q._fields_] == FIELDS
    assert C.sizeof(Q) == 104
    F = capi.nb_split_force_request                                     # the head is nb_split_force_request, field for field
    assert all(getattr(Q, f).offset == getattr(F, f).offset for f, _ in F._fields_)


def test_null_handle_and_null_request_are_invalid_without_a_device():
    L = capi.load_library()
    req = capi.nb_split_lists_request()
    req.struct_size = C.sizeof(capi.nb_split_lists_request)
    req.m, req.radius, req.cap = 1, 1.0, 4
    assert L.nb_split_lists(None, C.byref(req)) == 1                   # NB_ERR_INVALID
    assert b"nb_split_lists" in L.nb_last_error(None)
    assert L.nb_split_lists(None, None) == 1
    assert L.nb_multi_split_lists(None, C.byref(req)) == 1
    assert b"nb_multi_split_lists" in L.nb_multi_last_error(None)
    assert L.nb_multi_split_lists(None, None) == 1
    assert L.nb_split_lists_shape(None, 1, 4, None, None, None, None) == 1
    assert b"nb_split_lists_shape" in L.nb_last_error(None)
    fused = C.c_int(7)
    assert L.nb_neighbor_scheme_fused(None, C.byref(fused)) == 1
    assert b"nb_neighbor_scheme_fused" in L.nb_last_error(None)


def test_binding_surface():
    for cls in (capi.Simulation, capi.MultiSimulation):
        sig = inspect.signature(cls.split_lists)
        assert list(sig.parameters) == ["self", "points", "bodies", "point_vel", "radius", "radii", "jerk", "cap"]
        assert all(sig.parameters[p].kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters)[2:])
    assert inspect.signature(capi.Simulation.split_lists).parameters["jerk"].default is None
    for name in ("split_lists_device", "split_lists_shape"):
        assert callable(getattr(capi.Simulation, name))
    assert isinstance(capi.Simulation.neighbor_scheme_fused, property)


def test_a_library_without_the_symbol_is_a_clear_error(monkeypatch):
    class Old:                                                          # a library of before round 17
        nb_split_force = nb_neighbor_lists = nb_set_neighbor_scheme = object()

    monkeypatch.setattr(capi, "_lib", Old())
    with pytest.raises(capi.NBodyError) as e:
        capi._need("nb_split_lists", "split_lists()")
    assert e.value.code == 1 and "split_lists()" in str(e.value) and "no nb_split_lists" in str(e.value)


def test_the_request_builder_checks_what_it_can_without_a_device():
    req, keep, out = capi._split_lists_request(np.float32, None, (3, 5), None, 0.5, None, True, 24)
    assert (req.m, req.flags, req.first_body, req.radius, req.cap, req.reserved) == (5, capi.NB_SPLIT_AT_BODIES, 3, 0.5, 24, 0) and req.struct_size == 104
    assert list(out) == list(capi.SPLIT_OUTPUTS) + ["list", "count"]
    assert out["list"].shape == (5, 24) and out["list"].dtype == np.uint32 and out["count"].shape == (5,) and out["count"].dtype == np.uint32
    assert req.accel_irr and req.jerk_reg and req.list and req.count and not req.points and not req.point_vel and not req.radii
    req, keep, out = capi._split_lists_request(np.float64, np.zeros((5, 3)), None, None, None, np.arange(5), False, 4097)
    assert req.flags == 0 and req.points and req.radii and req.cap == 4097 and out["list"].shape == (5, 1) and not req.jerk_irr
    for bad in (dict(), dict(bodies=(-1, 5)), dict(points=np.zeros((5, 5))), dict(points=np.zeros((5, 3)), point_vel=np.zeros((4, 3))),
                dict(bodies=(0, 5), radii=np.zeros(4)), dict(bodies=(0, 5), cap=-1)):
        kw = dict(points=None, bodies=None, point_vel=None, radii=None, cap=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            capi._split_lists_request(np.float32, kw["points"], kw["bodies"], kw["point_vel"], 1.0, kw["radii"], False, kw["cap"])


def usage():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", res, re.S):
        if "Function Name" not in m.group(2):
            out[m.group(1)] = (int(re.search(r" VGPRs: (\d+)", m.group(2)).group(1)), int(m.group(3)), int(m.group(4)))
    return out


def test_split_lists_kernels_use_no_scratch():
    u = usage()
    new = {k: v for k, v in u.items() if re.match(r"_ZN2nb\d+nb_spl(_pk|64|_rows)I", k)}
    assert len(new) == 5, sorted(new)                                    # (f32, f64) x (with, without the jerk) + the gather
    assert all(scratch == 0 for _, scratch, _ in new.values()), new
    pk = {k: v for k, v in new.items() if "nb_spl_pk" in k}
    ref = {k: v for k, v in u.items() if re.match(r"_ZN2nb\d+nb_split_pkI", k)}
    assert len(pk) == 2 and len(ref) == 2
    assert {occ for _, _, occ in pk.values()} == {occ for _, _, occ in ref.values()} == {2}      # the waves per SIMD nb_split_pk is compiled for
