"""nb_split_force (added within ABI 2.4) without a device: the exports, the request structure, the argument checks that come before any
device call, the binding surface, the reference against census_ref's full sums, the census record (tolerances measured from a
binary32 restatement, never from a device; one boundary pair on the wrong side breaks them) and the built code of the nb_split*
kernels (no scratch)."""
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
import census_ref
import split_force_ref as R

CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(ROOT, "include", "nbody3d_hip.h")
FIELDS = ["struct_size", "m", "flags", "first_body", "points", "point_vel", "radii", "radius", "accel_irr", "accel_reg", "jerk_irr", "jerk_reg"]
ENTRY = ("nb_split_force", "nb_multi_split_force", "nb_split_force_shape")


def test_library_exports_the_split_force_entry_points():
    L = capi.load_library()
    assert L.nb_abi_version() == 2 and L.nb_abi_minor() == 4          # an addition within 2.4: detected by the symbol
    for name in ENTRY:
        assert name in capi.SYMBOLS
        assert getattr(L, name) is not None
    text = open(HEADER).read()
    assert re.search(r"#define NB_ABI_MINOR 4u", text) and "2.4 (round 15)" in text
    for name in ENTRY + ("nb_split_force_request",):
        assert name in text
    assert re.search(r"#define NB_SPLIT_AT_BODIES 1u", text) and re.search(r"#define NB_SPLIT_DEVICE +4u", text)
    assert (capi.NB_SPLIT_AT_BODIES, capi.NB_SPLIT_DEVICE) == (1, 4)


def test_request_structure_matches_the_header(tmp_path):
    """sizeof and every field offset of nb_split_force_request as a C compiler lays the header's structure out."""
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nbody3d_hip.h"\n'
                   'int main(void) { printf("%zu", sizeof(nb_split_force_request));\n'
                   + "".join('printf(" %%zu", offsetof(nb_split_force_request, %s));\n' % f for f in FIELDS)
                   + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    Q = capi.nb_split_force_request
    assert got == [C.sizeof(Q)] + [getattr(Q, f).offset for f, _ in Q._fields_]
    assert [f for f, _ in Q._fields_] == FIELDS
    assert C.sizeof(Q) == 80


def test_null_handle_and_null_request_are_invalid_without_a_device():
    L = capi.load_library()
    req = capi.nb_split_force_request()
    req.struct_size = C.sizeof(capi.nb_split_force_request)
    req.m, req.radius = 1, 1.0
    assert L.nb_split_force(None, C.byref(req)) == 1                   # NB_ERR_INVALID
    assert b"nb_split_force" in L.nb_last_error(None)
    assert L.nb_split_force(None, None) == 1
    assert L.nb_multi_split_force(None, C.byref(req)) == 1
    assert b"nb_multi_split_force" in L.nb_multi_last_error(None)
    assert L.nb_multi_split_force(None, None) == 1
    assert L.nb_split_force_shape(None, 1, None, None, None, None) == 1
    assert b"nb_split_force_shape" in L.nb_last_error(None)


def test_binding_surface():
    for cls in (capi.Simulation, capi.MultiSimulation):
        sig = inspect.signature(cls.split_force)
        assert list(sig.parameters) == ["self", "points", "bodies", "point_vel", "radius", "radii", "jerk"]
        assert all(sig.parameters[p].kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters)[2:])
    assert inspect.signature(capi.Simulation.split_force).parameters["jerk"].default is None
    for name in ("split_force_device", "split_force_shape", "irregular_force"):
        assert callable(getattr(capi.Simulation, name))


def test_a_library_without_the_symbol_is_a_clear_error(monkeypatch):
    class Old:                                                          # a library of before round 15
        nb_neighbors = nb_neighbor_lists = nb_knn = nb_list_force = object()

    monkeypatch.setattr(capi, "_lib", Old())
    with pytest.raises(capi.NBodyError) as e:
        capi._need("nb_split_force", "split_force()")
    assert e.value.code == 1 and "split_force()" in str(e.value) and "no nb_split_force" in str(e.value)


def test_the_request_builder_checks_what_it_can_without_a_device():
    req, keep, out = capi._split_force_request(np.float32, None, (3, 5), None, 0.5, None, True)
    assert (req.m, req.flags, req.first_body, req.radius) == (5, capi.NB_SPLIT_AT_BODIES, 3, 0.5) and req.struct_size == 80
    assert list(out) == list(R.OUTPUTS) and all(a.shape == (5, 4) and a.dtype == np.float32 for a in out.values())
    assert req.accel_irr and req.accel_reg and req.jerk_irr and req.jerk_reg and not req.points and not req.point_vel and not req.radii
    req, keep, out = capi._split_force_request(np.float64, np.zeros((5, 3)), None, None, None, np.arange(5), False)
    assert req.flags == 0 and req.points and req.radii and req.radius == 0.0 and not req.jerk_irr and not req.jerk_reg
    assert list(out) == ["accel_irr", "accel_reg"] and keep[2].dtype == np.float64 and keep[0].shape == (5, 4)
    for bad in (dict(), dict(bodies=(-1, 5)), dict(points=np.zeros((5, 5))), dict(points=np.zeros((5, 3)), point_vel=np.zeros((4, 3))),
                dict(bodies=(0, 5), radii=np.zeros(4))):
        kw = dict(points=None, bodies=None, point_vel=None, radii=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            capi._split_force_request(np.float32, kw["points"], kw["bodies"], kw["point_vel"], 1.0, kw["radii"], False)
    with pytest.raises(ValueError) as e:                                # the message names the function that was called
        capi._split_force_request(np.float32, np.zeros((3, 5)), None, None, 1.0, None, False)
    assert "split_force()" in str(e.value)


def test_the_two_sums_add_up_to_the_census_full_row_sums():
    """irr + reg of split_ref equals census_ref.row_ref's sums over all rows to 1e-13 (of the row's scale), at the bodies and at points;
    a radius of 0 leaves every irregular sum empty, one past the system every regular sum."""
    n = 300
    b, v = R.bodies(n, 9), R.velocities(n, 9)
    rows = np.arange(n)
    full = census_ref.row_ref(b, rows, vel=v)
    ref = R.split_ref(b, v, radius=2.0 * R.SPACING)
    assert 0 < ref["member"].sum() < n * n and ref["member"][rows, rows].all()
    for kind, key, scale in (("accel", "a", "scale"), ("jerk", "j", "j_scale")):
        d = np.abs(ref[kind + "_irr"] + ref[kind + "_reg"] - full[key]).max(1)
        assert (d <= 1e-13 * full[scale]).all(), kind
        assert np.allclose(ref[kind + "_irr_scale"] + ref[kind + "_reg_scale"], full[scale], rtol=1e-13)
    pts = R.points(n, 40, 9)
    pfull = census_ref.row_ref(b, None, targets=pts)
    pref = R.split_ref(b, None, radius=2.0 * R.SPACING, pts=pts)
    assert (np.abs(pref["accel_irr"] + pref["accel_reg"] - pfull["a"]).max(1) <= 1e-13 * pfull["scale"]).all()
    none = R.split_ref(b, v, radii=np.zeros(n))
    assert not none["member"].any() and not none["accel_irr"].any() and not none["jerk_irr"].any() and not none["accel_irr_scale"].any()
    every = R.split_ref(b, v, radius=100.0)
    assert every["member"].all() and not every["accel_reg"].any() and not every["jerk_reg"].any()
    f32 = R.split_f32(b, v, member=none["member"])
    assert not f32["accel_irr"].any() and not f32["jerk_irr"].any()
    with pytest.raises(AssertionError):                                  # a pair within 1e-6 of its radius is refused
        x = b[:, :3].astype(np.float64)
        R.split_ref(b, v, radius=float(np.sqrt(((x[1] - x[0]) ** 2).sum())) * (1 + 1e-8), dtype=np.float64)


def test_census_record_is_current_and_the_restatement_is_inside_its_tolerances():
    """The committed tolerances equal a fresh measurement; the restatement is inside each of them; every input keeps boundary_share >= 8
    tol for all four outputs, at the bodies and at the points."""
    rec = R.record()
    fresh = [R.measure(n, sp) for n in R.SIZES for sp in R.SPACINGS]
    assert rec["G"] == R.G == 0.37 and rec["eps2"] == R.EPS2 == 1e-4 and rec["tol_f64"] == 1e-12 and rec["near"] == 8
    assert [(e["n"], e["spacings"]) for e in rec["inputs"]] == [(n, sp) for n in (77, 1025, 4099) for sp in (1.6, 2.4)]
    for e, f in zip(rec["inputs"], fresh):
        assert set(e) == set(f)
        assert e["factor"] == R.TOL_FACTOR == 8.0 and e["points"] == 300
        for k in e:
            if isinstance(e[k], float):
                assert e[k] == pytest.approx(f[k], rel=1e-6), (e["n"], e["spacings"], k)
            else:
                assert e[k] == f[k], (e["n"], e["spacings"], k)
        for pre in ("", "pt_"):
            for out in R.OUTPUTS:
                tol, err, share = e[pre + out + "_tol"], e[pre + out + "_ref_f32_err"], e[pre + out + "_boundary_share"]
                assert tol == pytest.approx(8.0 * err, rel=1e-12) and 0 < err < tol and err < 3e-6
                assert share >= 8.0 * tol, (e["n"], e["spacings"], pre + out, share / tol)
    c = rec["cancellation"]
    assert c["n"] == 4096 and c["seed"] == 7 and 31.5 < c["mean_count"] < 32.5
    for kind in ("accel", "jerk"):                                       # recorded, not asserted as a ratio
        for how in ("subtract", "split"):
            assert 0 < c[kind][how]["median"] <= c[kind][how]["worst"]


@pytest.mark.parametrize("n,spacings", [(77, 1.6), (1025, 2.4)])
def test_one_boundary_pair_on_the_wrong_side_breaks_both_sums(n, spacings):
    """Moving any single boundary pair (the 8 nearest the radius on either side of every row) to the other sum in the reference moves
    both sums it touches by more than their tolerance."""
    c = R.census_input(n, spacings)
    e = R.entry(n, spacings)
    for pre, ref, xt in (("", c["ref"], c["b"]), ("pt_", c["pref"], c["pts"])):
        xt = np.asarray(xt, np.float64)[:, :3]
        _, pick = R.boundary_share(c["b"], ref, xt, R.radii_of(c["radius"], None, len(xt), np.float32))
        k, j = np.nonzero(pick)
        assert len(k) >= 8 * len(xt)
        for kind, t in (("accel", ref["tn"]), ("jerk", ref["tjn"])):
            for side in ("_irr", "_reg"):
                scale = ref[kind + side + "_scale"][k]
                moved = t[k, j][scale > 0] / scale[scale > 0]            # the row error the move makes in this sum (an empty sum: != 0)
                assert (moved > e[pre + kind + side + "_tol"]).all(), (pre, kind, side)


def split_usage():
    if shutil.which("/opt/rocm/bin/hipcc") is None and shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", CSRC, "-s", "asm"])
    res = open(os.path.join(CSRC, "nb_engine.resources.txt")).read()
    usage = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)ScratchSize \[bytes/lane\]: (\d+)", res, re.S):
        if re.match(r"_ZN2nb\d+nb_split(_pk|64|_reduce)I", m.group(1)) and "Function Name" not in m.group(2):
            usage[m.group(1)] = int(m.group(3))
    return usage


def test_split_force_kernels_use_no_scratch():
    usage = split_usage()
    assert len(usage) == 6, sorted(usage)                                # (f32, f64) x (with, without the jerk) + two reduces
    assert all(scratch == 0 for scratch in usage.values()), usage
