"""The neighbour scheme with radii that follow a target count and its restore (nb_set_neighbor_adapt, nb_upload_neighbor_scheme; added
within ABI 2.4, round 18) without a device: the exports, the three structures, the argument checks that need no handle, the binding
surface, the restatement's limits, the committed record (tests/golden/ac_adapt.json) and the built code of the five new kernels."""
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
import ac_adapt_ref as A
import ac_ref as R
from block_ref import norm_err

CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
ENTRY = ("nb_set_neighbor_adapt", "nb_neighbor_adapt_stats", "nb_download_neighbor_radii", "nb_upload_neighbor_scheme")
FIELDS = {"nb_neighbor_adapt": ["struct_size", "target", "max_rebuilds", "flags", "grow_max", "radius_min", "radius_max"],
          "struct nb_neighbor_adapt_stats": ["struct_size", "enabled", "rebuilds", "rows_shrunk", "last_rebuilds", "reserved"],
          "nb_neighbor_checkpoint": ["struct_size", "reserved", "accel_irr", "jerk_irr", "accel_reg", "jerk_reg", "list", "count", "radii"]}


def test_library_exports_the_four_entry_points():
    L = capi.load_library()
    assert L.nb_abi_version() == 2 and L.nb_abi_minor() == 4          # an addition within 2.4: detected by the symbol
    text = open(HEADER).read()
    assert "2.4 (round 18)" in text
    for name in ENTRY:
        assert name in capi.SYMBOLS and name in text
        assert getattr(L, name) is not None


def test_structures_match_the_header(tmp_path):
    """sizeof and every field offset of the three structures as a C compiler lays the header's out: 40, 32 and 64 bytes (two words and
    seven pointers: the checkpoint as it is declared has no room for the 72 its proposal quoted)."""
    src = tmp_path / "size.c"
    body = ""
    for t, fields in FIELDS.items():
        body += 'printf(" %%zu", sizeof(%s));\n' % t + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (t, f) for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbody3d_hip.h"\nint main(void) {\n' + body + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = []
    for t, fields in FIELDS.items():
        S = getattr(capi, t.split()[-1])
        assert [f for f, _ in S._fields_] == fields
        want += [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert got == want
    assert [C.sizeof(capi.nb_neighbor_adapt), C.sizeof(capi.nb_neighbor_adapt_stats), C.sizeof(capi.nb_neighbor_checkpoint)] == [40, 32, 64]


def good_cfg(**kw):
    cfg = capi.nb_neighbor_adapt()
    cfg.struct_size, cfg.target = C.sizeof(capi.nb_neighbor_adapt), 6
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_invalid_arguments_without_a_device():
    """Every NB_ERR_INVALID that needs no handle's shape (2 target > cap and the contents of an upload need one: test_ac_adapt_gpu.py):
    the fields of a request are checked in front of the handle, so the message names the field whatever else is wrong."""
    L = capi.load_library()
    nan, inf = float("nan"), float("inf")
    for kw, field in ((dict(struct_size=32), "struct_size"), (dict(flags=1), "flags"), (dict(target=0), "target"), (dict(max_rebuilds=17), "max_rebuilds"),
                      (dict(grow_max=0.99), "grow_max"), (dict(grow_max=-2.0), "grow_max"), (dict(grow_max=nan), "grow_max"), (dict(grow_max=inf), "grow_max"),
                      (dict(radius_min=-1e-3), "radius_min"), (dict(radius_min=nan), "radius_min"), (dict(radius_max=-1.0), "radius_max"),
                      (dict(radius_max=nan), "radius_max"), (dict(radius_min=0.2, radius_max=0.1), "radius_min must not exceed radius_max"),
                      (dict(), "null handle"), (dict(grow_max=1.0, max_rebuilds=16, radius_min=0.1, radius_max=0.1), "null handle")):
        assert L.nb_set_neighbor_adapt(None, C.byref(good_cfg(**kw))) == 1, kw                # NB_ERR_INVALID
        msg = L.nb_last_error(None).decode()
        assert msg.startswith("nb_set_neighbor_adapt: ") and field in msg, (kw, msg)
    assert L.nb_set_neighbor_adapt(None, None) == 1 and b"null handle" in L.nb_last_error(None)
    st = capi.nb_neighbor_adapt_stats()
    st.struct_size = C.sizeof(capi.nb_neighbor_adapt_stats)
    assert L.nb_neighbor_adapt_stats(None, C.byref(st), 0) == 1 and b"nb_neighbor_adapt_stats" in L.nb_last_error(None)
    assert L.nb_download_neighbor_radii(None, None, None) == 1 and b"nb_download_neighbor_radii" in L.nb_last_error(None)
    ck = capi.nb_neighbor_checkpoint()
    for size, reserved, field in ((72, 0, "struct_size"), (64, 1, "reserved"), (64, 0, "accel_irr")):
        ck.struct_size, ck.reserved = size, reserved
        assert L.nb_upload_neighbor_scheme(None, C.byref(ck)) == 1
        msg = L.nb_last_error(None).decode()
        assert msg.startswith("nb_upload_neighbor_scheme: ") and field in msg, msg
    buf = np.zeros(8, np.float32)
    for k in FIELDS["nb_neighbor_checkpoint"][2:8]:
        setattr(ck, k, buf.ctypes.data)
    assert L.nb_upload_neighbor_scheme(None, C.byref(ck)) == 1 and b"null handle" in L.nb_last_error(None)
    assert L.nb_upload_neighbor_scheme(None, None) == 1 and b"nb_upload_neighbor_scheme" in L.nb_last_error(None)


def test_binding_surface():
    S = capi.Simulation
    assert "target, grow_max=None, max_rebuilds=None, radius_min=None, radius_max=None" in S.set_neighbor_adapt.__doc__
    assert list(inspect.signature(S.neighbor_adapt_stats).parameters) == ["self", "reset"]
    assert list(inspect.signature(S.download_neighbor_radii).parameters) == ["self"]
    assert list(inspect.signature(S.upload_neighbor_scheme).parameters) == ["self", "accel_irr", "jerk_irr", "accel_reg", "jerk_reg", "list", "count", "radii"]
    assert list(inspect.signature(S.neighbor_scheme_checkpoint).parameters) == ["self", "cap"]
    assert list(inspect.signature(S.restore_neighbor_scheme).parameters)[:2] == ["self", "ck"]
    assert not hasattr(capi.MultiSimulation, "set_neighbor_adapt")                  # nb_multi has no counterpart


def test_a_library_without_the_symbol_is_a_clear_error():
    class Old:                                                          # a library of before round 18
        nb_set_neighbor_scheme = nb_split_lists = object()

    sim = object.__new__(capi.Simulation)
    sim._L, sim._h = Old(), None
    for call in (lambda: sim.set_neighbor_adapt(6), lambda: sim.neighbor_adapt_stats(), lambda: sim.download_neighbor_radii(), lambda: sim.upload_neighbor_scheme()):
        with pytest.raises(capi.NBodyError) as e:
            call()
        assert e.value.code == 1 and "no nb_set_neighbor_adapt" in str(e.value)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def small():
    b, v = R.fixture("plummer256")
    return b[:96].copy(), v[:96].copy()


@pytest.mark.parametrize("store", [np.float64, np.float32])
def test_grow_max_one_without_an_overflow_is_ac_ref_exactly(store):
    b, v = small()
    radii = (0.5 * R.radii_pattern(len(b))).astype(np.float32)
    for kw in (dict(radius=0.4), dict(radii=radii)):
        o = A.ac_adapt_ref(b, v, 1.0, R.EPS2, R.DT, 3, 5, substeps=4, cap=40, grow_max=1.0, store=store, **kw)
        w = R.ac_ref(b, v, 1.0, R.EPS2, R.DT, 3, substeps=4, cap=40, store=store, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(o[:8], w[:8])) and 5 < int(w[7].max()) <= 40      # (counts on either side of the target)
        assert {k: o[8][k] for k in w[8]} == w[8] and (o[8]["rebuilds"], o[8]["rows_shrunk"]) == (0, 0)
        assert o[9].tobytes() == o[10].tobytes() == np.asarray(radii if "radii" in kw else np.full(len(b), 0.4), store).astype(np.float64).tobytes()


def test_the_rule_keeps_a_radius_of_zero_and_respects_its_clamps():
    h = np.array([0.0, 0.1, 0.1, 0.1, 0.1, 0.0])
    c = np.array([0, 0, 6, 600, 5, 3], np.uint32)
    for kw in (dict(), dict(radius_min=0.09, radius_max=0.11), dict(grow_max=1.0), dict(radius_min=0.5)):
        r = A.rule(h, c, 6, **kw)
        assert r[0] == 0.0 and r[5] == 0.0, kw                         # never lifted off 0, not even by radius_min
    r = A.rule(h, c, 6)
    g = A.GROW_DEFAULT
    assert r[1] == 0.1 * g and r[2] == 0.1 and r[3] == 0.1 * (1.0 / g) and 0.1 < r[4] < 0.1 * g
    r = A.rule(h, c, 6, radius_min=0.09, radius_max=0.11)
    assert r[1] == 0.11 and r[3] == 0.09 and r[2] == 0.1
    assert (A.rule(h, c, 6, grow_max=1.0) == h).all()
    assert A.rule(np.array([0.1]), np.array([0]), 6, store=np.float32)[0] == float(np.float32(0.1 * g))
    # the shrink touches the overflowed rows alone, and at 2 target <= cap < c it shrinks by more than cbrt(1/2)
    s = A.shrink(h, c, 24, 6)
    assert (s[[0, 1, 2, 4, 5]] == h[[0, 1, 2, 4, 5]]).all() and s[3] == 0.1 * np.cbrt(6.0 / 600.0) < 0.1 * 0.5 ** (1 / 3)


def test_a_recovery_shrinks_the_overflowed_rows_and_exhaustion_is_reported():
    b, v = small()
    o = A.ac_adapt_ref(b, v, 1.0, R.EPS2, R.DT, 0, 4, substeps=2, cap=8, radius=0.7)      # the start alone
    st = o[8]
    assert st["rebuilds"] >= 1 and st["rows_shrunk"] >= st["rebuilds"] and st["builds"] == 1 + st["rebuilds"] and st["overflowed"] == 0
    assert int(o[7].max()) <= 8 and (o[9] <= 0.7).all() and (o[9] < 0.7).any()
    with pytest.raises(A.Overflow) as e:                                # every row holds everybody at any radius one shrink reaches
        A.ac_adapt_ref(b, v, 1.0, R.EPS2, R.DT, 1, 4, substeps=2, cap=8, radius=100.0, max_rebuilds=1)
    assert "96 rows, largest count 95, cap 8" in str(e.value)


# ---- the record ----------------------------------------------------------------------------------------------------------------
def test_the_record_holds_its_margins_rebuilds_collapse_and_order():
    rec = A.record()
    assert rec["steps"] == A.STEPS and rec["substeps"] == A.SUBSTEPS and sorted(rec["cases"]) == sorted(A.CASES)
    for name, e in rec["cases"].items():
        cfg = A.CASES[name]
        assert all(e[k] == cfg[k] for k in ("fixture", "G", "dt", "target", "cap", "per_body", "f32")), name
        st = e["stats"]
        assert st["overflowed"] == 0 and st["max_count"] <= e["cap"] and st["regular_steps"] == A.STEPS and st["builds"] == A.STEPS + 1 + st["rebuilds"]
        assert 2 * e["target"] <= e["cap"]
        if name.startswith("recover"):
            assert st["rebuilds"] > 0 and st["rows_shrunk"] >= st["rebuilds"], name
        else:
            assert st["rebuilds"] == 0 and st["rows_shrunk"] == 0, name
        if e["f32"]:
            assert e["margin"] >= 32 * e["D"] > 0 and all(0 < e["f32_err"][q] < 1e-4 for q in A.QUANTITIES), name
            assert cfg["scan"][0] <= e["radius"] <= cfg["scan"][1] and e["radius"] == float(np.float32(e["radius"]))
        else:
            assert e["margin"] >= 1e-9, name
        state = A.recorded_state(name)
        assert state[0].shape == (e["n"], 3) and state[6].shape == (e["n"], e["cap"]) and int(state[7].max()) == st["max_count"]
        assert os.path.getsize(A.state_path(name)) < 1 << 20 and os.path.getsize(A.list_path(name)) < 1 << 20
    c = rec["collapse"]
    assert 40 <= c["K"] < 80 and c["steps"] == c["K"] + 8
    for key in ("f64", "f32"):
        assert c["stats_" + key]["regular_steps"] == c["steps"] and c["stats_" + key]["rebuilds"] >= 1 and c["stats_" + key]["overflowed"] == 0
        assert 0 < c["dE_" + key] < 1e-5
    assert sorted(c["dE_at"]) == sorted([str(c["K"]), str(c["deep"])])
    for at in c["dE_at"].values():                                      # whatever the rule trades away, it stays below the shared step at dt
        assert 0 < at["adaptive"] < at["hermite"] and 0 < at["fixed_cap255"] < at["hermite"]
    assert rec["order"]["ratio"] >= 12                                  # the scheme's own order gate


def test_the_record_is_current():
    """The two smallest cases are run again: the recorded state, radii, rows, stats, margin and binary32 error are what the
    restatement gives."""
    rec = A.record()
    for name in ("track256", "recover256"):
        e = rec["cases"][name]
        b, v, kw = A.case_args(e)
        m = []
        o = A.ac_adapt_ref(b, v, e["G"], R.EPS2, e["dt"], A.STEPS, margins=m, **kw)
        o32 = A.ac_adapt_ref(b, v, e["G"], R.EPS2, e["dt"], A.STEPS, margins=m, store=np.float32, **kw)
        want = A.recorded_state(name)
        for got, w in zip(A.totals(o), want[:4]):
            assert norm_err(got, w) <= 1e-12
        assert np.abs(o[10] - want[4]).max() <= 1e-15 and np.abs(o32[10] - want[5]).max() <= 1e-9
        assert o[6].tobytes() == want[6].tobytes() == o32[6].tobytes() and o[7].tobytes() == want[7].tobytes()
        assert o[8] == e["stats"] == o32[8]
        assert min(m) == pytest.approx(e["margin"], rel=1e-6)
        for i, q in enumerate(A.QUANTITIES):
            assert norm_err(A.totals(o32, np.float32)[i], A.totals(o)[i]) == pytest.approx(e["f32_err"][q], rel=1e-3)


# ---- the built kernels ---------------------------------------------------------------------------------------------------------
def usage():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+)(.*?)LDS Size \[bytes/block\]: (\d+)", res, re.S):
        if re.match(r"_ZN2nb\d+nb_ac_(check|shrink|regular_ad|start_ad|restore)I", m.group(1)) and "Function Name" not in m.group(2) + m.group(4):
            out[m.group(1)] = (int(m.group(3)), int(m.group(5)))
    return out


def test_the_new_kernels_use_no_scratch_and_no_lds():
    u = usage()
    assert len(u) == 9, sorted(u)                                       # nb_ac_check + (f32, f64) x (shrink, regular_ad, start_ad, restore)
    assert all(x == (0, 0) for x in u.values()), u
