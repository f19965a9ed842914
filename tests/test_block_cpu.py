"""Block individual time steps of the Hermite integrator (nb_set_block_steps) without a device: the exports and the layout of the
two structures, the rejections that come before any device call, the binding surface, the built code of the nb_blk_* kernels, and
the fp64 restatement of the scheme (tests/block_ref.py) against the shared-step restatement and on an eccentric Kepler orbit."""
import ctypes as C
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

from nbody3d_amd import capi, ic

import block_ref as R

CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
NAMES = ("nb_set_block_steps", "nb_block_stats", "nb_download_levels", "nb_upload_levels")


def test_library_exports_the_block_step_entry_points():
    L = capi.load_library()
    for name in NAMES:
        assert name in capi.SYMBOLS
        assert getattr(L, name) is not None
    text = open(HEADER).read()
    assert re.search(r"#define\s+NB_BLOCK_FROZEN\s+1u", text) and capi.NB_BLOCK_FROZEN == 1
    assert capi.ABI_MINOR == 3 and capi.abi_minor() == 4          # additions within 2.4: detected by the symbol


def test_structure_layouts_match_the_header(tmp_path):
    steps = ("struct_size", "max_level", "min_level", "flags", "eta")
    stats = ("struct_size", "enabled", "outer_steps", "block_steps", "body_steps", "clamped", "finest_level", "reserved")
    fmt = " ".join(["%zu"] * (2 + len(steps) + len(stats)))
    args = ["sizeof(nb_block_steps)"] + ["offsetof(nb_block_steps, %s)" % f for f in steps]
    args += ["sizeof(struct nb_block_stats)"] + ["offsetof(struct nb_block_stats, %s)" % f for f in stats]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbody3d_hip.h"\n'
                   'int main(void) { printf("%s\\n", %s); return 0; }\n' % (fmt, ", ".join(args)))
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(capi.nb_block_steps)] + [getattr(capi.nb_block_steps, f).offset for f in steps]
    want += [C.sizeof(capi.nb_block_stats)] + [getattr(capi.nb_block_stats, f).offset for f in stats]
    assert got == want
    assert got[0] == 24 and got[len(steps) + 1] == 48


def test_null_handle_rejections_name_the_function():
    L = capi.load_library()
    cfg = capi.nb_block_steps()
    cfg.struct_size = C.sizeof(cfg)
    st = capi.nb_block_stats()
    st.struct_size = C.sizeof(st)
    buf = (C.c_uint8 * 4)()
    for name, call in (("nb_set_block_steps", lambda: L.nb_set_block_steps(None, C.byref(cfg))),
                       ("nb_block_stats", lambda: L.nb_block_stats(None, C.byref(st), 0)),
                       ("nb_download_levels", lambda: L.nb_download_levels(None, buf)),
                       ("nb_upload_levels", lambda: L.nb_upload_levels(None, buf))):
        assert call() == 1, name
        assert name.encode() in L.nb_last_error(None), name


def test_binding_surface():
    S = capi.Simulation
    for m in ("set_block_steps", "block_stats", "read_levels", "upload_levels"):
        assert callable(getattr(S, m)), m
    assert "reset" in inspect.signature(S.block_stats).parameters
    doc = S.set_block_steps.__doc__
    assert all(k in doc for k in ("eta", "max_level", "min_level", "frozen"))


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_block_surface_cpu():
    js = os.path.join(ROOT, "nbody3d-webgpu_amd", "js")
    addon, src = os.path.join(js, "addon", "nb_napi.node"), os.path.join(js, "addon", "nb_napi.c")
    if not os.path.exists(addon) or os.path.getmtime(addon) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", js, "-s"])
    p = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "node_block_tests.js"), "cpu"],
                       capture_output=True, text=True, timeout=300)
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert line, "node produced no result: rc=%d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(line[-1])
    assert res["ok"] and p.returncode == 0, {k: v for k, v in res["results"].items() if not v["pass"]}
    for k in ("addon_exports_setBlockSteps", "addon_exports_blockStats", "addon_exports_downloadLevels", "addon_exports_uploadLevels",
              "wrapper_has_setBlockSteps", "wrapper_has_blockStats", "wrapper_has_readLevels", "wrapper_has_uploadLevels"):
        assert res["results"][k]["pass"], k


# ---- the built code --------------------------------------------------------------------------------------------------------
def block_kernels():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    text = open(os.path.join(CSRC, "nb_engine.gfx950.s")).read()
    res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN2nb\d+nb_blk_\w+):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M)}
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+)", res, re.S):
        if re.match(r"_ZN2nb\d+nb_blk_", m.group(1)) and "Function Name" not in m.group(2):
            scratch[m.group(1)] = int(m.group(3))
    return bodies, scratch


def test_block_kernels_use_no_scratch():
    bodies, scratch = block_kernels()
    assert bodies and set(scratch) == set(bodies), (sorted(bodies), sorted(scratch))
    assert all(v == 0 for v in scratch.values()), scratch
    for want in ("nb_blk_start", "nb_blk_sched", "nb_blk_predict", "nb_blk_fj_pkILi2E", "nb_blk_fj_pkILi1E", "nb_blk_fj64", "nb_blk_correct"):
        assert any(want in k for k in bodies), want
    for k, v in bodies.items():
        assert "scratch_" not in v, k
        if "nb_blk_fj_pk" in k:
            assert "v_pk_fma_f32" in v and "v_rsq_f32" in v and "global_load_lds_dwordx4" in v, k
        if "nb_blk_fj64" in k:
            assert "v_rsq_f64" in v and "v_fma_f64" in v, k


def test_gathered_f32_force_jerk_loop_is_the_pair_arithmetic():
    """The innermost loop of nb_blk_fj_pk<2> and <1>: at most 26 packed instructions per two v_rsq_f32, nothing that touches global
    memory or scratch (the gather is in the prologue, the compact store in the epilogue)."""
    bodies, _ = block_kernels()
    found = 0
    for name, body in bodies.items():
        if "nb_blk_fj_pk" not in name:
            continue
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
        assert plain, (name, [len(lp) for lp in inner])
        for lp in plain:
            ops = [l.split()[0] for l in lp if not l.endswith(":")]
            rsq = sum(o.startswith("v_rsq_f32") for o in ops)
            pk = sum(o.startswith("v_pk_") for o in ops)
            print("%s inner loop: %d instructions, %d v_pk_*, %d v_rsq_f32" % (name, len(ops), pk, rsq))
            assert rsq >= 8 and rsq % 2 == 0 and 0 < pk <= 26 * (rsq // 2), (name, rsq, pk)
            assert not any(o.startswith("scratch_") or o.startswith("global_") for o in ops), name
        found += 1
    assert found == 2, sorted(bodies)


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", [0, 3])
def test_pinned_levels_in_the_restatement_are_shared_steps(l):
    b, v = R.tight_pair(*ic.plummer(40, seed=21))
    dt = 2.0 ** -4
    got = R.block_ref(b, v, 1.0, R.EPS2, dt, 2, max_level=l, min_level=l)
    ref = R.hermite_ref(b, v, 1.0, R.EPS2, dt / 2 ** l, 2 * 2 ** l)
    errs = [R.norm_err(got[k][:, :3], ref[k][:, :3]) for k in range(4)]
    print("pinned level %d against the shared-step restatement: x %.3g v %.3g a %.3g j %.3g" % ((l,) + tuple(errs)))
    assert max(errs) <= 1e-13, errs
    assert got[5]["block_steps"] == 2 * 2 ** l and got[5]["body_steps"] == 40 * 2 * 2 ** l and (got[4] == l).all()


def test_kepler_orbit_in_the_restatement():
    """e = 0.9, one period in 16 outer steps: |dE/E| <= 1e-5 in at most 1/8 of the 8,192 body-steps the pinned level-8 run needs."""
    b0, v0, out, de = R.kepler_ref()
    st = out[5]
    print("Kepler e=0.9 restatement: |dE/E| %.3g, %d body-steps in %d block steps, finest level %d"
          % (de, st["body_steps"], st["block_steps"], st["finest_level"]))
    assert de <= 1e-5, de
    assert st["body_steps"] <= 8192 // 8, st
    assert st["clamped"] == 0
