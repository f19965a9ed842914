"""nb_list_force (added within ABI 2.4) without a device: the exports, the request structure, the argument checks that come before any
device call, the binding surface, the request builder, the reference against a plain loop, the census record (tolerances measured
from a binary32 restatement, never from a device) and the built code of the nb_lf* kernels (no scratch)."""
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
import list_force_ref as R

CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
FIELDS = ["struct_size", "m", "flags", "first_body", "points", "point_vel", "list", "count", "cap", "reserved", "accel", "jerk", "phi"]
ENTRY = ("nb_list_force", "nb_multi_list_force", "nb_list_force_shape")


def test_library_exports_the_list_force_entry_points():
    L = capi.load_library()
    assert L.nb_abi_version() == 2 and L.nb_abi_minor() == 4          # an addition within 2.4: detected by the symbol
    for name in ENTRY:
        assert name in capi.SYMBOLS
        assert getattr(L, name) is not None
    text = open(HEADER).read()
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 14)" in text
    for name in ENTRY + ("nb_list_force_request",):
        assert name in text
    assert re.search(r"#define NB_LISTF_AT_BODIES 1u", text) and re.search(r"#define NB_LISTF_DEVICE +4u", text)
    assert (capi.NB_LISTF_AT_BODIES, capi.NB_LISTF_DEVICE) == (1, 4)


def test_request_structure_matches_the_header(tmp_path):
    """sizeof and every field offset of nb_list_force_request as a C compiler lays the header's structure out."""
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbody3d_hip.h"\n'
                   'int main(void) { printf("%zu", sizeof(nb_list_force_request));\n'
                   + "".join('printf(" %%zu", offsetof(nb_list_force_request, %s));\n' % f for f in FIELDS)
                   + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    Q = capi.nb_list_force_request
    assert got == [C.sizeof(Q)] + [getattr(Q, f).offset for f, _ in Q._fields_]
    assert [f for f, _ in Q._fields_] == FIELDS
    assert C.sizeof(Q) == 80


def test_null_handle_and_null_request_are_invalid_without_a_device():
    L = capi.load_library()
    req = capi.nb_list_force_request()
    req.struct_size = C.sizeof(capi.nb_list_force_request)
    req.m, req.cap = 1, 8
    assert L.nb_list_force(None, C.byref(req)) == 1                    # NB_ERR_INVALID
    assert b"nb_list_force" in L.nb_last_error(None)
    assert L.nb_list_force(None, None) == 1
    assert L.nb_multi_list_force(None, C.byref(req)) == 1
    assert b"nb_multi_list_force" in L.nb_multi_last_error(None)
    assert L.nb_multi_list_force(None, None) == 1
    assert L.nb_list_force_shape(None, 1, 8, None, None) == 1
    assert b"nb_list_force_shape" in L.nb_last_error(None)


def test_binding_surface():
    for cls in (capi.Simulation, capi.MultiSimulation):
        assert callable(getattr(cls, "list_force"))
        sig = inspect.signature(cls.list_force)
        assert list(sig.parameters) == ["self", "lists", "bodies", "points", "point_vel", "count", "accel", "jerk", "phi"]
        assert all(sig.parameters[p].kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters)[2:])
        assert (sig.parameters["accel"].default, sig.parameters["jerk"].default, sig.parameters["phi"].default) == (True, False, False)
    for name in ("list_force_device", "list_force_shape", "irregular_force"):
        assert callable(getattr(capi.Simulation, name))
    sig = inspect.signature(capi.Simulation.irregular_force)
    assert list(sig.parameters)[:3] == ["self", "radius", "cap"] and sig.parameters["cap"].default == 128
    assert {"jerk", "phi"} <= set(sig.parameters)


def test_a_library_without_the_symbol_is_a_clear_error(monkeypatch):
    class Old:                                                          # a library of before round 14
        nb_neighbors = nb_neighbor_lists = nb_knn = object()

    monkeypatch.setattr(capi, "_lib", Old())
    with pytest.raises(capi.NBodyError) as e:
        capi._need("nb_list_force", "list_force()")
    assert e.value.code == 1 and "list_force()" in str(e.value) and "no nb_list_force" in str(e.value)
    with pytest.raises(capi.NBodyError):
        capi._list_force_request(np.float32, np.zeros((1, 4), np.uint32), (0, 1), None, None, None, True, False, False)


def test_the_request_builder_checks_what_it_can_without_a_device():
    rows = np.arange(35, dtype=np.uint32).reshape(5, 7)
    req, keep, a, j, f = capi._list_force_request(np.float32, rows, (3, 5), None, None, None, True, False, True)
    assert (req.m, req.cap, req.flags, req.first_body, req.reserved) == (5, 7, capi.NB_LISTF_AT_BODIES, 3, 0) and req.struct_size == 80
    assert a.shape == (5, 4) and a.dtype == np.float32 and j is None and f.shape == (5,)
    assert req.list and req.accel and req.phi and not req.jerk and not req.points and not req.point_vel and not req.count
    req, keep, a, j, f = capi._list_force_request(np.float64, rows, None, np.zeros((5, 3)), np.zeros((5, 4)), np.arange(5), False, True, False)
    assert req.flags == 0 and req.points and req.point_vel and req.count and req.jerk and not req.accel and not req.phi
    assert j.dtype == np.float64 and keep[1].shape == (5, 4) and keep[2].shape == (5, 4) and keep[3].dtype == np.uint32 and a is None
    req, _, a, _, _ = capi._list_force_request(np.float32, np.zeros((2, 5000), np.uint32), (0, 2), None, None, None, True, False, False)
    assert req.cap == 5000                                               # the engine's to refuse: passed on
    for bad in (dict(lists=np.zeros(6, np.uint32)), dict(bodies=(0, 4)), dict(bodies=(-1, 5)), dict(points=np.zeros((4, 3))),
                dict(points=np.zeros((5, 5))), dict(points=np.zeros((5, 3)), point_vel=np.zeros((4, 3))), dict(count=np.zeros(4))):
        kw = dict(lists=rows, bodies=None, points=None, point_vel=None, count=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            capi._list_force_request(np.float32, kw["lists"], kw["bodies"], kw["points"], kw["point_vel"], kw["count"], True, False, False)


def test_reference_equals_a_plain_loop():
    rng = np.random.default_rng(14)
    n = 40
    b, v = R.bodies(n, 9), R.velocities(n, 9)
    rows = rng.integers(0, n, (12, 9)).astype(np.uint32)                 # unordered, with duplicates and own indices
    rows[rng.random(rows.shape) < 0.3] = R.NONE                          # padding anywhere
    rows[2] = R.NONE                                                     # an empty row
    rows[3, 1], rows[4, 0] = n, 0xfffffffe                               # no bodies either
    count = rng.integers(0, 12, 12)
    pts, pv = R.points(n, 12, 9), R.point_velocities(12, 9)
    for kw in (dict(first=5), dict(first=5, count=count), dict(pts=pts, pvel=pv), dict(pts=pts, pvel=pv, count=count)):
        ref = R.list_ref(b, v, rows, **kw)
        a, j, phi = R.naive_ref(b, v, rows, **kw)
        assert np.allclose(ref["a"], a, rtol=1e-12, atol=0) and np.allclose(ref["j"], j, rtol=1e-11, atol=1e-18)
        assert np.allclose(ref["phi"], phi, rtol=1e-12, atol=0)
        assert not ref["a"][2].any() and ref["scale"][2] == 0 and ref["terms"][2] == 0
        fa, fj, fp = R.list_f32(b, v, rows, **kw)
        ea, ej, ep = R.errors(fa, fj, fp, ref)
        assert max(ea, ej, ep) < 2e-6 and not fa[2].any() and not fj[2].any() and fp[2] == 0
    lists, count = R.radius_rows(b, 2.0 * R.SPACING, 16)
    x = b[:, :3].astype(np.float64)
    for k in (0, 17, 39):
        d2 = ((x - x[k]) ** 2).sum(1)
        want = [j for j in range(n) if j != k and d2[j] < float(np.float32(2.0 * R.SPACING)) ** 2]
        assert count[k] == len(want) and list(lists[k, :len(want)]) == want[:16] and (lists[k, len(want):] == R.NONE).all()


def test_census_record_is_current_and_can_show_one_entry():
    """The committed tolerances equal a fresh measurement, and every input keeps min_share >= 8 tol for a, the jerk and phi, at the
    bodies and at the points: one missed, doubled or misattributed entry moves its row by more than the tolerance."""
    rec = R.record()
    fresh = R.measure_all()
    assert rec["G"] == R.G == 0.37 and rec["eps2"] == R.EPS2 == 1e-4 and rec["tol_f64"] == 1e-12
    assert [(e["n"], e["spacings"]) for e in rec["inputs"]] == [(n, sp) for n in (77, 1025, 4099) for sp in (1.6, 2.4)]
    for e, f in zip(rec["inputs"], fresh["inputs"]):
        assert set(e) == set(f)
        assert e["factor"] == R.TOL_FACTOR == 8.0 and e["cap"] == 128 and e["max_count"] <= 128
        for k in e:
            if isinstance(e[k], float):
                assert e[k] == pytest.approx(f[k], rel=1e-6), (e["n"], e["spacings"], k)
            else:
                assert e[k] == f[k], (e["n"], e["spacings"], k)
        for pre in ("", "pt_"):
            for out in ("a", "jerk", "phi"):
                tol, err, share = e[pre + out + "_tol"], e[pre + out + "_ref_f32_err"], e[pre + out + "_min_share"]
                assert tol == pytest.approx(8.0 * err, rel=1e-12) and 0 < err < 1e-6
                assert share >= 8.0 * tol, (e["n"], e["spacings"], pre + out, share / tol)
    counts = [e["mean_count"] for e in rec["inputs"]]
    assert 6.5 < min(counts) < 7.5 and 41 < max(counts) < 43


def lf_usage():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
    usage = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", res, re.S):
        if re.match(r"_ZN2nb\d+nb_lf(32|64)I", m.group(1)) and "Function Name" not in m.group(2):
            usage[m.group(1)] = (int(m.group(3)), int(m.group(4)))
    return usage


def test_list_force_kernels_use_no_scratch_and_no_lds():
    usage = lf_usage()
    assert len(usage) == 14, sorted(usage)                               # 7 output sets x 2 precisions
    assert all(scratch == 0 and lds == 0 for scratch, lds in usage.values()), usage
