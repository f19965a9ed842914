"""Block individual irregular steps inside the neighbour scheme (nb_set_neighbor_levels; added within ABI 2.4, round 19) without
a device: the exports, the two structures, the argument checks that need no handle, the binding surface, the restatement's two
limits and its accuracy against the shared scheme, the committed record (tests/golden/ac_levels.json) and the built code of the
new kernels."""
import ctypes as C
import functools
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

from nbody3d_amd import capi
import ac_levels_ref as LR
import ac_ref as R
from block_ref import norm_err

CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
ENTRY = ("nb_set_neighbor_levels", "nb_neighbor_level_stats", "nb_download_neighbor_levels", "nb_upload_neighbor_levels")
FIELDS = {"nb_neighbor_levels": ["struct_size", "min_level", "flags", "reserved", "eta"],
          "struct nb_neighbor_level_stats": ["struct_size", "enabled", "regular_steps", "ticks", "block_steps", "body_steps", "entries",
                                             "clamped", "finest_level", "reserved"]}


def test_library_exports_the_four_entry_points():
    L = capi.load_library()
    assert L.nb_abi_version() == 2 and L.nb_abi_minor() == 4          # an addition within 2.4: detected by the symbol
    text = open(HEADER).read()
    assert "2.4 (round 19)" in text and "#define NB_NLEV_FROZEN 1u" in text and capi.NLEV_FROZEN == 1
    for name in ENTRY:
        assert name in capi.SYMBOLS and name in text
        assert getattr(L, name) is not None


def test_structures_match_the_header(tmp_path):
    """sizeof and every field offset of the two structures as a C compiler lays the header's out: 24 and 64 bytes."""
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
    assert [C.sizeof(capi.nb_neighbor_levels), C.sizeof(capi.nb_neighbor_level_stats)] == [24, 64]


def good_cfg(**kw):
    cfg = capi.nb_neighbor_levels()
    cfg.struct_size = C.sizeof(capi.nb_neighbor_levels)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_invalid_arguments_without_a_device():
    """Every NB_ERR_INVALID that needs no handle (min_level > log2(substeps) and an uploaded level out of range need one:
    test_ac_levels_gpu.py): the fields are checked in front of the handle, so the message names the field whatever else is wrong."""
    L = capi.load_library()
    nan = float("nan")
    for kw, field in ((dict(struct_size=32), "struct_size"), (dict(struct_size=0), "struct_size"), (dict(flags=2), "flags"),
                      (dict(flags=0x80000001), "flags"), (dict(reserved=1), "reserved"), (dict(eta=-1e-3), "eta"), (dict(eta=nan), "eta"),
                      (dict(), "null handle"), (dict(flags=1, min_level=3, eta=0.01), "null handle")):
        assert L.nb_set_neighbor_levels(None, C.byref(good_cfg(**kw))) == 1, kw                # NB_ERR_INVALID
        msg = L.nb_last_error(None).decode()
        assert msg.startswith("nb_set_neighbor_levels: ") and field in msg, (kw, msg)
    assert L.nb_set_neighbor_levels(None, None) == 1 and b"null handle" in L.nb_last_error(None)
    st = capi.nb_neighbor_level_stats()
    st.struct_size = C.sizeof(capi.nb_neighbor_level_stats)
    assert L.nb_neighbor_level_stats(None, C.byref(st), 0) == 1 and b"nb_neighbor_level_stats" in L.nb_last_error(None)
    buf = np.zeros(8, np.uint8)
    for fn in ("nb_download_neighbor_levels", "nb_upload_neighbor_levels"):
        assert getattr(L, fn)(None, buf.ctypes.data) == 1 and fn.encode() in L.nb_last_error(None)
        assert getattr(L, fn)(None, None) == 1 and fn.encode() in L.nb_last_error(None)


def test_binding_surface():
    S = capi.Simulation
    assert "min_level=0, eta=None, frozen=False" in S.set_neighbor_levels.__doc__
    assert list(inspect.signature(S.neighbor_level_stats).parameters) == ["self", "reset"]
    assert list(inspect.signature(S.download_neighbor_levels).parameters) == ["self"]
    assert list(inspect.signature(S.upload_neighbor_levels).parameters) == ["self", "levels"]
    assert list(inspect.signature(S.restore_neighbor_scheme).parameters) == ["self", "ck", "scheme", "adapt", "levels"]
    assert not hasattr(capi.MultiSimulation, "set_neighbor_levels")                 # nb_multi has no counterpart


def test_a_library_without_the_symbol_is_a_clear_error():
    class Old:                                                          # a library of before round 19
        nb_set_neighbor_scheme = nb_split_lists = nb_set_neighbor_adapt = object()

    sim = object.__new__(capi.Simulation)
    sim._L, sim._h, sim.n = Old(), None, 4
    for call in (lambda: sim.set_neighbor_levels(min_level=1), lambda: sim.neighbor_level_stats(), lambda: sim.download_neighbor_levels(),
                 lambda: sim.upload_neighbor_levels(np.zeros(4, np.uint8))):
        with pytest.raises(capi.NBodyError) as e:
            call()
        assert e.value.code == 1 and "no nb_set_neighbor_levels" in str(e.value)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def args_of(name):
    e = R.record()["fixtures"][name]
    b, v = R.fixture(name)
    return b, v, e, R.radius_args(len(b), e["per_body"], e["radius"])


@functools.lru_cache(maxsize=None)
def shared(name, substeps):
    b, v, e, kw = args_of(name)
    return R.ac_ref(b, v, e["G"], R.EPS2, e["dt"], LR.STEPS_REC, substeps=substeps, cap=e["cap"], **kw)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_frozen_levels_are_the_shared_scheme_bit_for_bit(name):
    """Every level frozen at L: ac_ref(substeps = 2^L); frozen at 0: ac_ref(substeps = 1).  (Two regular steps at L = 6.)"""
    b, v, e, kw = args_of(name)
    for m, ns in ((6, 64), (0, 1)):
        w = R.ac_ref(b, v, e["G"], R.EPS2, e["dt"], 2, substeps=ns, cap=e["cap"], **kw)
        o = LR.ac_levels_ref(b, v, e["G"], R.EPS2, e["dt"], 2, L=6, cap=e["cap"], min_level=m, frozen=True, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(o[:8], w[:8])), (name, m)
        assert o[9] == dict(w[8], substeps=2 * 64) and (o[8] == m).all()      # (.substeps keeps counting 2^L per regular step)
        ls, n = o[10], len(b)
        assert (ls["ticks"], ls["block_steps"], ls["body_steps"]) == (128, 2 * ns, 2 * ns * n) and ls["finest_level"] == m
        assert ls["entries"] == ns * (w[8]["entries"] - int(np.minimum(w[7], e["cap"]).sum()))      # the rows of the first two builds, ns times each


@pytest.mark.parametrize("name", ["plummer256", "plummer1024"])
def test_levels_are_ten_times_closer_than_the_shared_scheme_at_their_floor(name):
    """Position error against the shared scheme at N_sub = 64: levels over [m, 6] against the shared scheme at N_sub = 2^m, for
    m = 1, 2, 3 (measured: 21x to 560x), with fewer body-steps than n 2^L."""
    b, v, e, kw = args_of(name)
    fine = shared(name, 64)[0][:, :3]
    for m in (1, 2, 3):
        o = LR.ac_levels_ref(b, v, e["G"], R.EPS2, e["dt"], LR.STEPS_REC, L=6, cap=e["cap"], min_level=m, eta=LR.ETA_REC, **kw)
        err, err_shared = norm_err(o[0][:, :3], fine), norm_err(shared(name, 2 ** m)[0][:, :3], fine)
        print("%s min_level %d: levels %.3g, shared N_sub = %d %.3g, ratio %.1f, body-steps %d of %d"
              % (name, m, err, 2 ** m, err_shared, err_shared / err, o[10]["body_steps"], LR.STEPS_REC * len(b) * 64))
        assert err * 10 <= err_shared, (name, m, err, err_shared)
        assert o[10]["body_steps"] < LR.STEPS_REC * len(b) * 64 and o[10]["block_steps"] <= o[10]["ticks"] == LR.STEPS_REC * 64
        assert int(o[8].min()) >= m and int(o[8].max()) <= 6


def test_uploaded_frozen_levels_step_every_body_by_its_own_level():
    b, v, e, kw = args_of("plummer256")
    lev = (np.arange(len(b)) % 4).astype(np.uint8)
    o = LR.ac_levels_ref(b, v, e["G"], R.EPS2, e["dt"], 2, L=3, cap=e["cap"], frozen=True, levels=lev, **kw)
    assert o[8].tobytes() == lev.tobytes()
    assert o[10]["body_steps"] == 2 * LR.body_steps_of(lev, 3) and o[10]["block_steps"] == 2 * 8 and o[10]["finest_level"] == 3


# ---- the record ----------------------------------------------------------------------------------------------------------------
def test_the_record_holds_its_conditions():
    rec = LR.record()
    assert (rec["L"], rec["eta"], rec["steps"]) == (LR.L_REC, LR.ETA_REC, LR.STEPS_REC)
    assert sorted(rec["runs"]) == sorted("%s_m%d" % (f, m) for f in R.FIXTURES for m in LR.MIN_LEVELS_REC)
    caps = {f: R.record()["fixtures"][f]["cap"] for f in R.FIXTURES}
    for key, e in rec["runs"].items():
        name = key.rsplit("_m", 1)[0]
        assert e["noise_flips"] == 0 and rec["noise"] == 1e-12 and len(rec["seeds"]) == 3, key      # no seed changes a level
        assert e["membership_margin"] >= 1e-3, key
        assert e["max_count"] <= caps[name] and e["scheme_stats"]["overflowed"] == 0, key
        assert e["decision_margin"] >= 1e-6, key                        # far above what an fp64 order of additions moves tau by
        ls = e["level_stats"]
        assert ls["ticks"] == LR.STEPS_REC * 64 and 0 < ls["block_steps"] <= ls["ticks"] and ls["body_steps"] < LR.STEPS_REC * e["n"] * 64, key
        assert len(e["levels"]) == e["n"] and min(e["levels"]) >= e["min_level"] and max(e["levels"]) <= 6, key
        assert LR.recorded_state(name, e["min_level"])[0].shape == (e["n"], 3)
        assert os.path.getsize(LR.state_path(name, e["min_level"])) < 1 << 20
    # empty ticks are part of the recorded runs
    assert rec["runs"]["plummer256_m0"]["level_stats"]["block_steps"] < 256 and rec["runs"]["plummer1024_m0"]["level_stats"]["block_steps"] < 256


def test_the_record_is_current():
    """The smallest case is run again: the recorded levels, stats and state are what the restatement gives."""
    rec = LR.record()
    b, v, e, kw = args_of("plummer256")
    for m in LR.MIN_LEVELS_REC:
        ent = rec["runs"]["plummer256_m%d" % m]
        o = LR.ac_levels_ref(b, v, e["G"], R.EPS2, e["dt"], LR.STEPS_REC, L=LR.L_REC, cap=e["cap"], min_level=m, eta=LR.ETA_REC, **kw)
        assert [int(z) for z in o[8]] == ent["levels"] and o[10] == ent["level_stats"] and o[9] == ent["scheme_stats"]
        for got, w in zip(R.totals(o), LR.recorded_state("plummer256", m)):
            assert norm_err(got, w) <= 1e-12


# ---- the built kernels ---------------------------------------------------------------------------------------------------------
def usage():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
    out = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+)(.*?)LDS Size \[bytes/block\]: (\d+)", res, re.S):
        if re.match(r"_ZN2nb\d+nb_ac_lv_(start|begin|sub32|sub64)I", m.group(1)) and "Function Name" not in m.group(2) + m.group(4):
            out[m.group(1)] = (int(m.group(3)), int(m.group(5)))
    return out


def test_the_new_kernels_use_no_scratch_and_no_lds():
    u = usage()
    assert len(u) == 6, sorted(u)                                       # nb_ac_lv_sub32, nb_ac_lv_sub64 + (f32, f64) x (start, begin)
    assert all(x == (0, 0) for x in u.values()), u
