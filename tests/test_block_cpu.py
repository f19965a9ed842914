"""Block individual time steps of the Hermite integrator (nb_set_block_steps) without a device: the exports and the layout of the
two structures, the rejections that come before any device call, the binding surface, the built code of the nb_blk_* kernels, and
the fp64 restatement of the scheme (tests/block_ref.py) against the shared-step restatement and on an eccentric Kepler orbit, its
decision log, and the inputs and the record of the decision audit (tests/test_block_decisions_gpu.py)."""
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


# ---- the decision log, decide() and correct() ------------------------------------------------------------------------------
_twelve = {}


def twelve():
    """The N = 12 system of the exact GPU test, two outer steps, with its log and its margins: computed once, shared."""
    if not _twelve:
        b0, v0 = R.tight_pair(*ic.plummer(12, seed=3))
        margins, log = [], []
        out = R.block_ref(b0, v0, 1.0, R.EPS2, 2.0 ** -3, 2, eta=0.02, max_level=12, margins=margins, log=log)
        _twelve["x"] = (b0, v0, out, margins, log)
    return _twelve["x"]


def test_replaying_the_log_alone_gives_the_levels_and_the_stats():
    b0, v0, out, margins, log = twelve()
    lev, st = R.replay_log(log, 12, 12, check=True)
    assert np.array_equal(lev, out[4]) and st == out[5], (lev, out[4], st, out[5])
    assert st["block_steps"] == len(R.log_active_sizes(log)) and st["body_steps"] == R.log_active_sizes(log).sum()
    kinds = R.log_kinds(log)
    assert sum(kinds[k] for k in ("deepened_one", "deepened_more", "coarsened", "kept")) + kinds["coarsen_unaligned"] == st["body_steps"], kinds
    assert R.log_min_margins(log, 12).min() == min(margins)
    assert R.first_divergence(log, out[4]) is None
    wrong = out[4].copy()
    wrong[5] += 1
    assert "body 5" in R.first_divergence(log, wrong)
    # a system that starts from uploaded levels and continues: the same, from those levels
    log2 = []
    out2 = R.block_ref(out[0], out[1], 1.0, R.EPS2, 2.0 ** -3, 1, eta=0.02, max_level=12, levels=out[4], aj=out[2:4], log=log2)
    lev, st = R.replay_log(log2, 12, 12, levels=out[4], check=True)
    assert np.array_equal(lev, out2[4]) and st == out2[5]


def test_margins_are_what_the_scalar_rule_collects():
    """margins= before the log existed: level_for's own collection, decision by decision in the order taken (the start rule, then
    every block step's active bodies in ascending order), decisions with an infinite tau left out."""
    b0, v0, out, margins, log = twelve()
    old, stats = [], {"clamped": 0}
    for e in log:
        for tau in e["tau"]:
            R.level_for(tau, 2.0 ** -3, 0, 12, stats, old)
    assert len(margins) == 436 and margins == old
    assert float(min(margins)) == 0.002277026047941999 and float(sum(margins)) == pytest.approx(88.30180751464374, rel=1e-12)


def test_decide_and_correct_reproduce_the_restatement_bit_for_bit():
    """The N = 12 run again, its schedule taken from the log, every step by correct() and decide() alone."""
    b0, v0, out, margins, log = twelve()
    dt, L = 2.0 ** -3, 12
    tick = dt / 2.0 ** L
    b, v = np.array(b0, np.float64), np.array(v0, np.float64)
    a, j = R.fj_ref(b, v, 1.0, R.EPS2)
    lev, t = log[0]["after"].copy(), np.zeros(12, np.int64)
    for e in log[1:]:
        act, t_next = e["act"], e["t_next"]
        h = ((t_next - t) * tick)[:, None]
        bp, vp = b.copy(), v.copy()
        bp[:, :3] = b[:, :3] + h * (v[:, :3] + h / 2 * (a + h / 3 * j))
        vp[:, :3] = v[:, :3] + h * (a + h / 2 * j)
        a1, j1 = R.fj_ref(bp, vp, 1.0, R.EPS2, act)
        hs = 2.0 ** (L - lev[act]) * tick
        x1, v1 = R.correct(b[act], v[act], a[act], j[act], a1, j1, hs)
        d = R.decide(a[act], j[act], a1, j1, hs, lev[act], t_next, dt, 0.02, 0, L)
        assert all(d[k].tobytes() == e[k].tobytes() for k in ("tau", "want", "after", "aligned", "clamped", "margin")), t_next
        b[act, :3], v[act, :3], a[act], j[act], lev[act], t[act] = x1, v1, a1, j1, d["after"], t_next
        if t_next == 2 ** L:
            t[:] = 0
    for got, want in zip((b, v, a, j, lev.astype(np.uint8)), out[:5]):
        assert got.tobytes() == want.tobytes()


def test_the_torch_direct_sum_is_the_numpy_one():
    b, v = R.tight_pair(*ic.plummer(1026, seed=22))
    rows = np.array([0, 1, 5, 300, 301, 1025])
    for r in (None, rows):
        for got, want in zip(R.fj_torch(b, v, 1.0, R.EPS2, r), R.fj_ref(b, v, 1.0, R.EPS2, r)):
            assert R.norm_err(got, want) <= 1e-13


# ---- the decision audit: its inputs and its record ---------------------------------------------------------------------------
def close(fresh, rec):
    """A fresh measurement against the record: counts and parameters equal; the margins |tau / step - 1| to the record's exclusion
    margin -- another machine may add the direct sums in another order, which moves tau by no more than its evaluation spread."""
    for k, val in fresh.items():
        if isinstance(val, float):
            assert val == pytest.approx(rec[k], rel=1e-6, abs=R.decisions_record()["exclusion_margin"]), (k, val, rec[k])
        else:
            assert val == rec[k], (k, val, rec[k])


@pytest.mark.parametrize("n", sorted(R.SCHEDULES))
def test_schedule_inputs_meet_their_conditions_and_the_record_is_a_fresh_measurement(n):
    """Part A's conditions on the restatement alone (at least five levels of 16 bodies, active sets in every bucket, every kind of
    decision, nothing clamped, the smallest margin at least 8 flip-safe margins), the record against a fresh measurement, and the
    stored sizes' fixtures regenerated.  The noise runs cost three more restatements each: they are repeated at N = 1026 only, the
    other sizes keep the recorded ones (never above the record's own bound)."""
    rec = next(e for e in R.decisions_record()["schedules"] if e["n"] == n)
    R.schedule_conditions(rec)
    noisy = n == 1026
    fresh, lev, state = R.measure_schedule(n, R.NOISE_SEEDS if noisy else ())
    print("N=%d: %s, levels %s, |A| %s, kinds %s, smallest margin %.3g" % (n, fresh["stats"], fresh["levels"], fresh["active_sizes"],
                                                                          fresh["kinds"], fresh["min_margin"]))
    dev = fresh.pop("noise_position_dev")
    if noisy:
        assert dev <= R.FACTOR * rec["noise_position_dev"], (dev, rec["noise_position_dev"])      # rounding noise: within the factor it is used with
    else:
        for k in ("noise_seeds", "noise_flipped", "flip_safe_margin"):
            fresh.pop(k)
    close(fresh, rec)
    assert rec["noise"] == 1e-12 and len(rec["noise_seeds"]) >= 3
    if n in R.STORED:
        slev, sstate = [np.load(p) for p in R.fixture_paths(n)]
        assert np.array_equal(slev, lev) and sstate.shape == state.shape and len(state) <= 256
        assert np.array_equal(sstate[:, 0], state[:, 0])
        for c in range(1, 13, 3):
            assert R.norm_err(sstate[:, c:c + 3], state[:, c:c + 3]) <= 1e-13
        assert all(os.path.getsize(p) < 64 * 1024 for p in R.fixture_paths(n))


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", R.STEP_SIZES)
def test_step_inputs_stay_under_the_cap_and_the_record_is_a_fresh_measurement(n, prec):
    """Part B on the reference alone: the decisions of the emulated block steps inside the exclusion margin are at most 0.5 % per
    run (the start rule's too), and the margin is 8 x the largest recorded spread, which a fresh measurement stays inside."""
    whole = R.decisions_record()
    rec = next(e for e in whole["steps"] if e["n"] == n and e["precision"] == prec)
    margin = whole["exclusion_margin"]
    assert margin == R.exclusion_margin(whole["steps"]) and whole["excluded_cap"] == R.EXCLUDED_CAP == 0.005 and whole["factor"] == R.FACTOR == 8
    fresh = R.measure_step(n, prec)
    assert fresh["start_tau_spread"] <= margin
    for f, r in zip(fresh["steps"], rec["steps"]):
        assert f.pop("tau_spread") <= margin, (f, margin)       # cancellation noise: held to the bound it sets, not to its own digits
        close(f, r)
    a0, j0 = R.step_inputs(n, prec)[2:]
    assert not j0[list(R.ZERO_JERK)].any() and np.count_nonzero((j0[:, :3] == 0).all(1)) == len(R.ZERO_JERK)
    runs = []
    for l2, L, lmin in R.START_RUNS:
        stats, log = {"clamped": 0}, []
        lev = R.start_levels(a0[:, :3], j0[:, :3], 2.0 ** l2, R.ETA, lmin, L, stats, log=log)
        runs.append(("start 2^%d L %d lmin %d" % (l2, L, lmin), log[0]["margin"], stats["clamped"]))
        assert lev.min() == lmin and (lev[list(R.ZERO_JERK)] == lmin).all()
    assert runs[-1][2] > 0                                      # the run that is there for clamped decisions has them
    for l2, L in R.STEP_RUNS:
        d = R.decide(*R.emulate_step(n, prec, 2.0 ** l2), 2.0 ** l2, 0, 2 ** L, 2.0 ** l2, R.ETA, 0, L)
        runs.append(("step 2^%d L %d" % (l2, L), d["margin"], int(d["clamped"].sum())))
        assert L == 12 or runs[-1][2] > 0
        assert L != 12 or len(np.unique(d["after"])) >= 5       # deepening from level 0 by many different depths
    for name, m, clamped in runs:
        share = float((m < margin).mean())
        print("N=%d %s %s: %d clamped, smallest margin %.3g, %.3g %% inside the exclusion margin %.3g" % (n, prec, name, clamped, m.min(), 100 * share, margin))
        assert share <= R.EXCLUDED_CAP, (name, share)


@pytest.mark.parametrize("L,lmin", R.FREE_RUNS)
def test_free_motion_schedule_is_integer_logic(L, lmin):
    """G = 0 with zero derivatives: every tau is inf, every want is min_level, and the schedule from mixed levels has all three
    outcomes of a wish to coarsen -- not aligned, one level, and one level where `want` is several below."""
    n, log = 1025, []
    out = R.free_schedule(n, "f32", L, lmin, log)
    lev0 = R.free_levels(n, L, lmin)
    assert all(np.isinf(e["tau"]).all() and (e["want"] == lmin).all() for e in log)
    kinds = R.log_kinds(log)
    several = sum(int(((e["before"] - e["want"] >= 2) & e["aligned"]).sum()) for e in log)
    print("L %d min_level %d: %s, %s, %d coarsened with want two or more below" % (L, lmin, out[5], kinds, several))
    assert kinds["coarsened"] > 0 and kinds["coarsen_unaligned"] > 0 and several > 0 and kinds["deepened_one"] == kinds["deepened_more"] == 0
    assert (out[4] == lmin).all() and out[5]["block_steps"] == L - lmin + 2 ** lmin and out[5]["clamped"] == 0      # then 2^lmin - 1 steps at min_level
    assert out[5]["body_steps"] == int((lev0.astype(np.int64) - lmin + 2 ** lmin).sum()) and out[5]["finest_level"] == L
    lev, st = R.replay_log(log, n, L, levels=lev0, check=True)
    assert np.array_equal(lev, out[4]) and st == out[5]
    assert not out[2].any() and not out[3].any()
