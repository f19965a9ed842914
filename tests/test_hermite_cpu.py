"""The Hermite integrator (nb_config.integrator = NB_INT_HERMITE4) without a device: the exports, the layout of nb_config, the
rejections that come before any device call, the built code of the nb_fj* / nb_hermite* kernels and the binding surface."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

from nbody3d_amd import capi

CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")


def test_library_exports_the_hermite_entry_points():
    L = capi.load_library()
    for name in ("nb_download_jerk", "nb_upload_derivs"):
        assert name in capi.SYMBOLS
        assert getattr(L, name) is not None
    text = open(HEADER).read()
    assert re.search(r"NB_INT_LEAPFROG\s*=\s*0\s*,\s*NB_INT_HERMITE4\s*=\s*1\b", text)
    assert re.search(r"NB_JERK\s*=\s*3\b", text)
    assert capi.NB_INT_HERMITE4 == 1 and capi.NB_INT_LEAPFROG == 0


def test_config_layout_is_unchanged_and_integrator_sits_at_72(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbody3d_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(nb_config), offsetof(nb_config, integrator), '
                   'offsetof(nb_config, reserved), sizeof(((nb_config *)0)->reserved)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [88, 72, 76, 12]
    K = capi.nb_config
    assert [C.sizeof(K), K.integrator.offset, K.reserved.offset, K.reserved.size] == got


def _cfg(n=64, integrator=1):
    cfg = capi.nb_config()
    cfg.struct_size = C.sizeof(capi.nb_config)
    cfg.n = n
    cfg.device = -1
    cfg.integrator = integrator
    return cfg


def _create(cfg):
    L = capi.load_library()
    h = C.c_void_p()
    rc = L.nb_create(C.byref(cfg), C.byref(h))
    assert not h.value
    return rc, L.nb_last_error(None)


def test_rejections_come_before_any_device_call():
    """NB_ERR_INVALID (1), never NB_ERR_NO_DEVICE (2), with a message that names the field."""
    L = capi.load_library()
    rc, msg = _create(_cfg(integrator=2))
    assert rc == 1 and b"integrator" in msg
    cfg = _cfg()
    cfg.shard_begin, cfg.shard_count = 0, 32
    rc, msg = _create(cfg)
    assert rc == 1 and b"shard_count" in msg
    cfg = _cfg()
    cfg.ext_bodies = 0x1000
    rc, msg = _create(cfg)
    assert rc == 1 and b"ext_bodies" in msg
    cfg = _cfg()
    cfg.force_variant = 201011
    rc, msg = _create(cfg)
    assert rc == 1 and b"force_variant" in msg
    cfg = _cfg()
    cfg.jsplit = 2
    rc, msg = _create(cfg)
    assert rc == 1 and b"jsplit" in msg
    m = C.c_void_p()
    cfg = _cfg(n=4096)
    assert L.nb_multi_create(C.byref(cfg), 2, None, C.byref(m)) == 1 and not m.value
    assert b"integrator" in L.nb_multi_last_error(None)
    info = capi.nb_plan_info()
    info.struct_size = C.sizeof(capi.nb_plan_info)
    assert L.nb_plan_query(C.byref(cfg), 256, 2.4e9, C.byref(info), None, 0) == 1
    assert b"integrator" in L.nb_last_error(None)
    buf = (C.c_float * 4)()
    assert L.nb_download_jerk(None, buf) == 1 and b"nb_download_jerk" in L.nb_last_error(None)
    assert L.nb_upload_derivs(None, buf, buf) == 1 and b"nb_upload_derivs" in L.nb_last_error(None)


def test_a_struct_that_ends_in_front_of_the_field_reads_it_as_leapfrog():
    """struct_size = offsetof(integrator) is still accepted and the (garbage) tail is not read: the config passes every check and
    fails only where a leapfrog config fails on this host (no device), or creates a handle where there is one."""
    L = capi.load_library()
    cfg = _cfg(integrator=7)
    cfg.struct_size = capi.nb_config.integrator.offset
    h = C.c_void_p()
    rc = L.nb_create(C.byref(cfg), C.byref(h))
    assert rc in (0, 2), (rc, L.nb_last_error(None))
    if h.value:
        assert not L.nb_variant_name(h).startswith(b"hermite4_")
        L.nb_destroy(h)


def hermite_kernels():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    text = open(os.path.join(CSRC, "nb_engine.gfx950.s")).read()
    res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN2nb\d+nb_(?:fj|hermite)\w+):.*?$(.*?)^\.Lfunc_end", text, re.S | re.M)}
    scratch = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+)", res, re.S):
        if re.match(r"_ZN2nb\d+nb_(fj|hermite)", m.group(1)) and "Function Name" not in m.group(2):
            scratch[m.group(1)] = int(m.group(3))
    return bodies, scratch


def test_hermite_kernels_use_no_scratch():
    bodies, scratch = hermite_kernels()
    assert bodies and set(scratch) == set(bodies), (sorted(bodies), sorted(scratch))
    assert all(v == 0 for v in scratch.values()), scratch
    for want in ("nb_fj_pk", "nb_fj64", "nb_fj_reduce", "nb_hermite_predict", "nb_hermite_correct"):
        assert any(want in k for k in bodies), want
    for k, v in bodies.items():
        assert "scratch_" not in v, k
        if "nb_fj_pk" in k:
            assert "v_pk_fma_f32" in v and "v_rsq_f32" in v and "global_load_lds_dwordx4" in v, k
        if "nb_fj64" in k:
            assert "v_rsq_f64" in v and "v_fma_f64" in v, k


def test_f32_force_jerk_loop_is_the_pair_arithmetic():
    """The innermost loop of nb_fj_pk: per two v_rsq_f32 (one packed group against one j-body) at most 26 packed instructions, at
    most one more VALU instruction in fourteen around them, and nothing that touches global memory or scratch."""
    bodies, _ = hermite_kernels()
    body = [v for k, v in bodies.items() if "nb_fj_pk" in k][0]
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
        print("nb_fj_pk inner loop: %d instructions, %d VALU, %d v_pk_*, %d v_rsq_f32" % (len(ops), len(valu), pk, rsq))
        assert rsq >= 8 and rsq % 2 == 0 and 0 < pk <= 26 * (rsq // 2), (rsq, pk)
        assert len(valu) - pk - rsq <= (pk + rsq) // 14, (len(valu), pk, rsq)
        assert not any(o.startswith("scratch_") or o.startswith("global_") for o in ops)


def test_binding_surface():
    assert callable(capi.Simulation.read_jerk) and callable(capi.Simulation.upload_derivs)
    assert "integrator" in inspect.signature(capi.Simulation.__init__).parameters
    assert "integrator" not in inspect.signature(capi.MultiSimulation.__init__).parameters
    with pytest.raises(ValueError):
        capi.Simulation(16, integrator="rk4")          # refused by the binding, before nb_create
    assert capi.ABI_MINOR == 3 and capi.abi_minor() == 4
