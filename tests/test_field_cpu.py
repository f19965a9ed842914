"""nb_field_eval (ABI 2.4) without a device: the exports, the request structure, the argument checks that come before any
device call, and the built code of the nb_field* kernels (no scratch, packed arithmetic)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

from nbody3d_amd import capi

CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")


def test_library_exports_the_field_entry_points_and_abi_minor_4():
    L = capi.load_library()
    assert L.nb_abi_version() == 2 and L.nb_abi_minor() >= 4
    for name in ("nb_field_eval", "nb_multi_field_eval"):
        assert name in capi.SYMBOLS
        assert getattr(L, name) is not None
    text = open(HEADER).read()
    assert re.search(r"#define NB_ABI_MINOR 4u", text)
    for flag, value in (("NB_FIELD_AT_BODIES", 1), ("NB_FIELD_F64", 2), ("NB_FIELD_DEVICE", 4)):
        assert re.search(r"#define %s\s+%du" % (flag, value), text), flag
        assert getattr(capi, flag) == value


def test_request_structure_matches_the_header(tmp_path):
    """sizeof and every field offset of nb_field_request as a C compiler lays the header's structure out."""
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbody3d_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(nb_field_request), offsetof(nb_field_request, struct_size), '
                   'offsetof(nb_field_request, m), offsetof(nb_field_request, flags), offsetof(nb_field_request, first_body), '
                   'offsetof(nb_field_request, points), offsetof(nb_field_request, accel), offsetof(nb_field_request, phi)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    R = capi.nb_field_request
    assert got == [C.sizeof(R)] + [getattr(R, f).offset for f, _ in R._fields_]
    assert [f for f, _ in R._fields_] == ["struct_size", "m", "flags", "first_body", "points", "accel", "phi"]


def test_null_handle_and_null_request_are_invalid_without_a_device():
    L = capi.load_library()
    req = capi.nb_field_request()
    req.struct_size = C.sizeof(capi.nb_field_request)
    req.m = 1
    assert L.nb_field_eval(None, C.byref(req)) == 1                     # NB_ERR_INVALID
    assert b"nb_field_eval" in L.nb_last_error(None)
    assert L.nb_field_eval(None, None) == 1
    assert L.nb_multi_field_eval(None, C.byref(req)) == 1
    assert b"nb_multi_field_eval" in L.nb_multi_last_error(None)
    assert L.nb_multi_field_eval(None, None) == 1


def test_binding_surface():
    for cls in (capi.Simulation, capi.MultiSimulation):
        assert callable(getattr(cls, "field"))
    assert callable(capi.Simulation.field_device) and callable(capi.Simulation.body_energies)
    assert capi.ABI_MINOR == 3          # the binding still loads a 2.3 library; field() asks for 2.4 itself


def field_kernels():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    text = open(os.path.join(CSRC, "nb_engine.gfx950.s")).read()
    res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN2nb\d+nb_field\w+):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M)}
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+)", res, re.S):
        if "nb_field" in m.group(1) and "Function Name" not in m.group(2):
            scratch[m.group(1)] = int(m.group(3))
    return bodies, scratch


def test_field_kernels_use_no_scratch_and_the_f32_loop_is_packed():
    bodies, scratch = field_kernels()
    assert bodies and set(scratch) == set(bodies), (sorted(bodies), sorted(scratch))
    assert all(v == 0 for v in scratch.values()), scratch
    f32 = [k for k in bodies if "nb_field_pk" in k]
    assert len(f32) == 3, f32                       # both outputs, acceleration only, potential only
    for k in f32:
        assert "v_pk_fma_f32" in bodies[k] and "v_rsq_f32" in bodies[k] and "global_load_lds_dwordx4" in bodies[k], k
        assert "scratch_" not in bodies[k], k
    assert any("nb_field64" in k for k in bodies) and any("nb_field_reduce" in k for k in bodies)
    for k in bodies:
        if "nb_field64" in k:
            assert "v_rsq_f64" in bodies[k] and "v_fma_f64" in bodies[k], k


def test_f32_field_loop_is_the_pair_arithmetic():
    """The plain (unmasked) loop of the two-output kernel: per packed group and j-body 13 packed instructions and 2 v_rsq_f32 --
    ONE reciprocal root per pair serves both outputs -- and at most one more VALU instruction in fourteen around them."""
    bodies, _ = field_kernels()
    body = [v for k, v in bodies.items() if "nb_field_pkILb1ELb1E" in k][0]
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
        assert rsq >= 8 and rsq % 2 == 0 and pk == 13 * (rsq // 2), (rsq, pk)
        assert len(valu) - pk - rsq <= (pk + rsq) // 14, (len(valu), pk, rsq)
        assert not any(o.startswith("scratch_") or o.startswith("global_") for o in ops)
