"""nb_knn (added within ABI 2.4) without a device: the exports, the request structure, the argument checks that come before any
device call, the binding surface, the host helpers (density_from_knn), the brute-force reference against a plain loop, and the built
code of the nb_knn* kernels (no scratch, no atomics)."""
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
from knn_ref import NONE, lattice_knn, naive_knn

CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
FIELDS = ["struct_size", "m", "flags", "first_body", "points", "k", "reserved", "index", "dist2"]
ENTRY = ("nb_knn", "nb_multi_knn", "nb_knn_shape")


def test_library_exports_the_knn_entry_points():
    L = capi.load_library()
    assert L.nb_abi_version() == 2 and L.nb_abi_minor() == 4          # an addition within 2.4: detected by the symbol
    for name in ENTRY:
        assert name in capi.SYMBOLS
        assert getattr(L, name) is not None
    text = open(HEADER).read()
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 13)" in text
    for name in ENTRY + ("nb_knn_request",):
        assert name in text


def test_request_structure_matches_the_header(tmp_path):
    """sizeof and every field offset of nb_knn_request as a C compiler lays the header's structure out."""
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbody3d_hip.h"\n'
                   'int main(void) { printf("%zu", sizeof(nb_knn_request));\n'
                   + "".join('printf(" %%zu", offsetof(nb_knn_request, %s));\n' % f for f in FIELDS)
                   + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    R = capi.nb_knn_request
    assert got == [C.sizeof(R)] + [getattr(R, f).offset for f, _ in R._fields_]
    assert [f for f, _ in R._fields_] == FIELDS
    assert C.sizeof(R) == 48


def test_null_handle_and_null_request_are_invalid_without_a_device():
    L = capi.load_library()
    req = capi.nb_knn_request()
    req.struct_size = C.sizeof(capi.nb_knn_request)
    req.m, req.k = 1, 6
    assert L.nb_knn(None, C.byref(req)) == 1                           # NB_ERR_INVALID
    assert b"nb_knn" in L.nb_last_error(None)
    assert L.nb_knn(None, None) == 1
    assert L.nb_multi_knn(None, C.byref(req)) == 1
    assert b"nb_multi_knn" in L.nb_multi_last_error(None)
    assert L.nb_multi_knn(None, None) == 1
    assert L.nb_knn_shape(None, 1, 6, None, None, None) == 1
    assert b"nb_knn_shape" in L.nb_last_error(None)


def test_binding_surface():
    for cls in (capi.Simulation, capi.MultiSimulation):
        assert callable(getattr(cls, "knn"))
    for name in ("knn_device", "knn_shape", "local_density", "density_center"):
        assert callable(getattr(capi.Simulation, name))
    assert callable(capi.density_from_knn)
    sig = inspect.signature(capi.Simulation.knn)
    assert list(sig.parameters) == ["self", "points", "bodies", "k", "dist2"]
    assert sig.parameters["k"].default == 6 and sig.parameters["dist2"].default is True
    assert all(sig.parameters[p].kind is inspect.Parameter.KEYWORD_ONLY for p in ("bodies", "k", "dist2"))
    assert inspect.signature(capi.Simulation.local_density).parameters["k"].default == 6
    assert inspect.signature(capi.Simulation.density_center).parameters["k"].default == 6


def test_a_library_without_the_symbol_is_a_clear_error(monkeypatch):
    class Old:                                                          # a library of before round 13
        nb_neighbors = nb_neighbor_lists = object()

    monkeypatch.setattr(capi, "_lib", Old())
    with pytest.raises(capi.NBodyError) as e:
        capi._need("nb_knn", "knn()")
    assert e.value.code == 1 and "knn()" in str(e.value) and "no nb_knn" in str(e.value)
    with pytest.raises(capi.NBodyError):
        capi._knn_request(np.float32, np.zeros((1, 4)), None, 6, True)


def test_the_request_builder_checks_what_it_can_without_a_device():
    req, keep, index, d2 = capi._knn_request(np.float32, np.zeros((5, 3)), None, 7, True)
    assert (req.m, req.k, req.flags, req.reserved) == (5, 7, 0, 0) and req.struct_size == 48
    assert index.shape == (5, 7) and index.dtype == np.uint32 and d2.shape == (5, 7) and d2.dtype == np.float32
    assert keep[0].shape == (5, 4) and req.points and req.index and req.dist2
    req, keep, index, d2 = capi._knn_request(np.float64, None, (3, 9), 64, False)
    assert (req.m, req.first_body, req.flags) == (9, 3, capi.NB_NBR_AT_BODIES) and not req.points and d2 is None and not req.dist2
    assert index.shape == (9, 64)
    for k in (0, 65):                                                   # the engine's to refuse: passed on, the arrays stay small
        req, _, index, _ = capi._knn_request(np.float32, np.zeros((2, 4)), None, k, True)
        assert req.k == k and index.shape == (2, 1)
    with pytest.raises(ValueError):
        capi._knn_request(np.float32, np.zeros((2, 5)), None, 6, True)
    with pytest.raises(ValueError):
        capi._knn_request(np.float32, None, (-1, 2), 6, True)
    with pytest.raises(ValueError):
        capi._knn_request(np.float32, np.zeros((2, 4)), None, -1, True)


def test_reference_equals_a_plain_loop():
    rng = np.random.default_rng(60)
    for n in (1, 2, 5, 60):
        b = rng.integers(-3, 4, (n, 3))
        if n >= 8:
            b[7] = b[3]                                              # a duplicate: a neighbour at d2 = 0
        pts = rng.integers(-3, 4, (20, 3))
        for k in (1, 6, 64):                                         # k > n (and k > n - 1): padded rows
            for got, want in ((lattice_knn(b, b, k, skip0=0), naive_knn(b, b, k, skip0=0)),
                              (lattice_knn(b, pts, k), naive_knn(b, pts, k)),
                              (lattice_knn(b, b[n // 3:], k, skip0=n // 3), naive_knn(b, b[n // 3:], k, skip0=n // 3))):
                assert got[0].dtype == np.uint32 and got[0].shape == want[0].shape == (len(got[1]), k)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    index, d2 = lattice_knn(b, b, 64, skip0=0)
    assert index[3, 0] == 7 and index[7, 0] == 3 and d2[3, 0] == 0           # the duplicate is the nearest, both ways
    assert not any(r in index[r] for r in range(60))                          # never itself
    assert np.all(index[:, 59:] == NONE) and np.all(np.isinf(d2[:, 59:])) and np.all(index[:, :59] != NONE)
    assert np.all(np.diff(d2[:, :59], axis=1) >= 0)
    ties = np.diff(d2[:, :59], axis=1) == 0
    assert ties.any() and np.all(np.diff(index[:, :59].astype(np.int64), axis=1)[ties] > 0)      # equal distances: ascending j


def test_density_from_knn_is_the_casertano_hut_estimate():
    rng = np.random.default_rng(61)
    n, k = 200, 6
    b = np.concatenate([rng.normal(size=(n, 3)), rng.uniform(0.5, 2.0, (n, 1))], axis=1)
    x = b[:, :3]
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(d2, np.inf)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    rows = np.take_along_axis(d2, order, axis=1)
    want = np.array([b[order[i, :k - 1], 3].sum() / (4.0 * np.pi / 3.0 * np.sqrt(rows[i, k - 1]) ** 3) for i in range(n)])
    got = capi.density_from_knn(b, order.astype(np.uint32), rows)
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-13, atol=0)
    assert np.allclose(capi.density_from_knn(b[:, 3], order.astype(np.uint32), rows.astype(np.float32)), want, rtol=1e-6)
    # short rows: nan, and only there
    idx = order.astype(np.uint32)
    dd = rows.copy()
    idx[5, k - 1], dd[5, k - 1] = NONE, np.inf
    idx[9, 2:], dd[9, 2:] = NONE, np.inf
    got = capi.density_from_knn(b, idx, dd)
    assert np.isnan(got[[5, 9]]).all() and np.isfinite(np.delete(got, [5, 9])).all()
    with pytest.raises(ValueError):
        capi.density_from_knn(b, idx[:, :1], dd[:, :1])                  # k >= 2
    with pytest.raises(ValueError):
        capi.density_from_knn(b, idx, dd[:, :3])

    class Stub(capi.Simulation):
        def __init__(self):
            self.n = n

        def knn(self, points=None, *, bodies=None, k=6, dist2=True):
            assert points is None and bodies == (0, n) and k == 6
            return order.astype(np.uint32), rows

        def read(self, bodies=True, vel=True, accel=True):
            return b, None, None

        def __del__(self):
            pass

    assert np.allclose(Stub().local_density(), want, rtol=1e-13)
    assert np.allclose(Stub().density_center(), (want[:, None] * x).sum(0) / want.sum(), rtol=1e-12)


def knn_kernels():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    text = open(os.path.join(CSRC, "nb_engine.gfx950.s")).read()
    res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN2nb\d+nb_knn\w+):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M)}
    usage = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", res, re.S):
        if "nb_knn" in m.group(1) and "Function Name" not in m.group(2):
            usage[m.group(1)] = (int(m.group(3)), int(m.group(4)))
    return bodies, usage


def test_knn_kernels_use_no_scratch_and_no_atomics_and_the_f32_pass_is_packed():
    bodies, usage = knn_kernels()
    assert bodies and set(usage) == set(bodies), (sorted(bodies), sorted(usage))
    assert all(scratch == 0 for scratch, _ in usage.values()), usage
    for name in bodies:
        assert "scratch_" not in bodies[name] and "atomic" not in bodies[name], name
    f32 = [name for name in bodies if "nb_knn_pk" in name]
    assert len(f32) == 1, f32
    assert usage[f32[0]][1] == 4, usage                              # four waves per SIMD, as nb_nbl_pk
    assert "v_pk_fma_f32" in bodies[f32[0]] and "global_load_lds_dwordx4" in bodies[f32[0]] and "v_readlane_b32" in bodies[f32[0]]
    assert "v_rsq" not in bodies[f32[0]] and "v_sqrt" not in bodies[f32[0]]
    f64 = [name for name in bodies if "nb_knn64" in name]
    assert f64 and len([name for name in bodies if "nb_knn_merge" in name]) == 2
    for name in f64:
        assert re.search(r"v_fmac?_f64", bodies[name]), name
