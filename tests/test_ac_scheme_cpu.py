"""The Ahmad-Cohen neighbour scheme (nb_set_neighbor_scheme, added within ABI 2.4) without a device: the exports, the two structures,
the argument checks that come before any device call, the binding surface, the restatement's two limits and its order, the committed
record (tests/golden/ac_scheme.json) and the built code of the nb_ac_* kernels (no scratch)."""
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
import ac_ref as R
from block_ref import hermite_ref, norm_err

CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
ENTRY = ("nb_set_neighbor_scheme", "nb_neighbor_scheme_stats", "nb_download_neighbor_scheme")
CFG_FIELDS = ["struct_size", "substeps", "cap", "flags", "radius", "radii"]
STATS_FIELDS = ["struct_size", "enabled", "regular_steps", "substeps", "entries", "builds", "max_count", "overflowed"]


def test_library_exports_the_three_entry_points():
    L = capi.load_library()
    assert L.nb_abi_version() == 2 and L.nb_abi_minor() == 4          # an addition within 2.4: detected by the symbol
    text = open(HEADER).read()
    assert "2.4 (round 16)" in text
    for name in ENTRY:
        assert name in capi.SYMBOLS and name in text
        assert getattr(L, name) is not None


def test_structures_match_the_header(tmp_path):
    """sizeof and every field offset of the two structures as a C compiler lays the header's out."""
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbody3d_hip.h"\n'
                   'int main(void) { printf("%zu", sizeof(nb_neighbor_scheme));\n'
                   + "".join('printf(" %%zu", offsetof(nb_neighbor_scheme, %s));\n' % f for f in CFG_FIELDS)
                   + 'printf(" %zu", sizeof(struct nb_neighbor_scheme_stats));\n'
                   + "".join('printf(" %%zu", offsetof(struct nb_neighbor_scheme_stats, %s));\n' % f for f in STATS_FIELDS)
                   + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    Q, S = capi.nb_neighbor_scheme, capi.nb_neighbor_scheme_stats
    assert got == [C.sizeof(Q)] + [getattr(Q, f).offset for f, _ in Q._fields_] + [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_]
    assert [f for f, _ in Q._fields_] == CFG_FIELDS and [f for f, _ in S._fields_] == STATS_FIELDS
    assert (C.sizeof(Q), C.sizeof(S)) == (32, 48)


def test_null_arguments_are_invalid_without_a_device():
    L = capi.load_library()
    cfg = capi.nb_neighbor_scheme()
    cfg.struct_size, cfg.radius = C.sizeof(capi.nb_neighbor_scheme), 0.1
    assert L.nb_set_neighbor_scheme(None, C.byref(cfg)) == 1                        # NB_ERR_INVALID
    assert b"nb_set_neighbor_scheme" in L.nb_last_error(None)
    assert L.nb_set_neighbor_scheme(None, None) == 1
    st = capi.nb_neighbor_scheme_stats()
    st.struct_size = C.sizeof(capi.nb_neighbor_scheme_stats)
    assert L.nb_neighbor_scheme_stats(None, C.byref(st), 0) == 1
    assert b"nb_neighbor_scheme_stats" in L.nb_last_error(None)
    assert L.nb_download_neighbor_scheme(None, None, None, None, None, None, None) == 1
    assert b"nb_download_neighbor_scheme" in L.nb_last_error(None)


def test_binding_surface():
    S = capi.Simulation
    assert list(inspect.signature(S.neighbor_scheme_stats).parameters) == ["self", "reset"]
    assert list(inspect.signature(S.download_neighbor_scheme).parameters) == ["self", "cap"]
    assert callable(S.set_neighbor_scheme) and "radius=None, radii=None, substeps=None, cap=None" in S.set_neighbor_scheme.__doc__
    assert not hasattr(capi.MultiSimulation, "set_neighbor_scheme")                 # nb_multi has no counterpart


def test_a_library_without_the_symbol_is_a_clear_error(monkeypatch):
    class Old:                                                          # a library of before round 16
        nb_split_force = nb_list_force = nb_neighbor_lists = object()

    sim = object.__new__(capi.Simulation)
    sim._L, sim._h = Old(), None
    for call in (lambda: sim.set_neighbor_scheme(radius=0.1), lambda: sim.neighbor_scheme_stats(), lambda: sim.download_neighbor_scheme(8)):
        with pytest.raises(capi.NBodyError) as e:
            call()
        assert e.value.code == 1 and "no nb_set_neighbor_scheme" in str(e.value)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def small():
    b, v = R.fixture("plummer256")
    return b[:96].copy(), v[:96].copy()


def test_an_empty_radius_is_a_plain_hermite_step():
    b, v = small()
    o = R.ac_ref(b, v, 1.0, R.EPS2, R.DT, R.STEPS, substeps=4, cap=4, radius=1e-9)
    h = hermite_ref(b, v, 1.0, R.EPS2, R.DT, R.STEPS)
    assert int(o[7].max()) == 0 and o[8]["entries"] == 0 and o[8]["builds"] == R.STEPS + 1
    assert norm_err(o[0][:, :3], h[0][:, :3]) <= 1e-12 and norm_err(o[1][:, :3], h[1][:, :3]) <= 1e-12


def test_a_radius_that_covers_everything_steps_by_hs():
    b, v = small()
    o = R.ac_ref(b, v, 1.0, R.EPS2, R.DT, R.STEPS, substeps=4, cap=128, radius=100.0)
    assert int(o[7].min()) == len(b) - 1 and np.abs(o[4]).max() == 0.0 and np.abs(o[5]).max() == 0.0      # nothing is regular
    fine = hermite_ref(b, v, 1.0, R.EPS2, R.DT / 4, 4 * R.STEPS)
    finer = hermite_ref(b, v, 1.0, R.EPS2, R.DT / 32, 32 * R.STEPS)
    for q in (0, 1):
        assert norm_err(o[q][:, :3], fine[q][:, :3]) < norm_err(fine[q][:, :3], finer[q][:, :3])


def test_an_overflow_is_reported_with_the_numbers():
    b, v = small()
    with pytest.raises(R.Overflow) as e:
        R.ac_ref(b, v, 1.0, R.EPS2, R.DT, 1, substeps=2, cap=8, radius=100.0)
    assert "96 rows, largest count 95, cap 8" in str(e.value)


def test_rows_of_keeps_the_cap_smallest_in_ascending_order():
    inside = np.zeros((3, 6), bool)
    inside[0, [5, 1, 3]] = True
    inside[2, :] = True
    lst, cnt = R.rows_of(inside, 4)
    assert cnt.tolist() == [3, 0, 6]
    assert lst.tolist() == [[1, 3, 5, R.NONE], [R.NONE] * 4, [0, 1, 2, 3]]


# ---- the record ----------------------------------------------------------------------------------------------------------------
def test_the_record_holds_its_margins_counts_and_order():
    rec = R.record()
    assert rec["steps"] == R.STEPS and tuple(rec["substeps"]) == R.SUBSTEPS and sorted(rec["fixtures"]) == sorted(R.FIXTURES)
    for name, e in rec["fixtures"].items():
        assert e["margin"] >= 1e-3 and e["max_count"] <= e["cap"], name
        for ns in R.SUBSTEPS:
            run = e["runs"][str(ns)]
            assert run["margin"] >= 1e-3 and run["max_count"] <= e["cap"] and run["builds"] == R.STEPS + 1
            assert all(0 < run["f32_err"][q] < 1e-4 for q in R.QUANTITIES)
            assert os.path.exists(R.state_path(name, ns)) and R.recorded_state(name, ns)[0].shape == (e["n"], 3)
    assert rec["order"]["ratio"] >= 12                                  # the lower end of a 4th-order scheme


def test_the_record_is_current():
    """The smallest fixture is run again: the recorded state, stats, margin and binary32 error are what the restatement gives."""
    rec = R.record()
    e = rec["fixtures"]["plummer256"]
    b, v = R.fixture("plummer256")
    kw = R.radius_args(len(b), e["per_body"], e["radius"])
    for ns in (2,):
        run, m = e["runs"][str(ns)], []
        o = R.ac_ref(b, v, e["G"], R.EPS2, e["dt"], R.STEPS, substeps=ns, cap=e["cap"], margins=m, **kw)
        o32 = R.ac_ref(b, v, e["G"], R.EPS2, e["dt"], R.STEPS, substeps=ns, cap=e["cap"], margins=m, store=np.float32, **kw)
        for got, want in zip(R.totals(o), R.recorded_state("plummer256", ns)):
            assert norm_err(got, want) <= 1e-12
        assert (o[8]["entries"], o[8]["builds"], o[8]["max_count"]) == (run["entries"], run["builds"], run["last_max_count"])
        assert min(m) == pytest.approx(run["margin"], rel=1e-6)
        for i, q in enumerate(R.QUANTITIES):
            assert norm_err(R.totals(o32, np.float32)[i], R.totals(o)[i]) == pytest.approx(run["f32_err"][q], rel=1e-3)
    order = R.measure_order(e)
    assert order["ratio"] == pytest.approx(rec["order"]["ratio"], rel=1e-3) and order["ratio"] >= 12


# ---- the built kernels ---------------------------------------------------------------------------------------------------------
def ac_usage():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
    usage = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+)(.*?)LDS Size \[bytes/block\]: (\d+)", res, re.S):
        if re.match(r"_ZN2nb\d+nb_ac_(sub32|sub64|predict0|regular|start)I", m.group(1)) and "Function Name" not in m.group(2) + m.group(4):
            usage[m.group(1)] = (int(m.group(3)), int(m.group(5)))
    return usage


def test_the_scheme_kernels_use_no_scratch_and_no_lds():
    usage = ac_usage()
    assert len(usage) == 8, sorted(usage)                                # the two substep kernels + (f32, f64) x (predict0, regular, start)
    assert all(u == (0, 0) for u in usage.values()), usage
