"""GPU tests of the native collective path (nb_rccl_attach) with 2 to 4 ranks on the one GPU of a test box.

RCCL refuses two ranks on one device, so the engine is pointed (NB_RCCL_LIB) at the stand-in library of tests/rccl_shim: all
ranks are threads of one child process (tests/rccl_shim/rccl_ranks_worker.py), the collectives are event-ordered copies and one
fixed-order sum kernel.  What runs is the PRODUCT's code against real foreign rows: rccl_exchange_begin / rccl_reduce_scatter_A /
rccl_exchange_wait of csrc/nb_comm.hip and the sym_rank and gather_pending branches of nb_step -- the send pointer base + row * sb,
the receive offset A + 4 * esz * sb, the wait for ev_done in front of a sweep that reads foreign rows, finish_gather in front of
a download or a query, the rebuild of the G*m stream at G != 1, the collective counters of nb_step_times2.  What it cannot show:
RCCL itself, xGMI, real process boundaries, nb_multi's RCCL mode with more than one shard.

NB_SHIM_LATE_US makes every collective land late (a host function sleeps on the collective's stream before the copies), so that a
forgotten wait reads stale rows instead of getting lucky.  Measured on an MI355X with nb_step_times2 (force pass + nb_sym_reduce,
the slowest rank of the plain run, averaged over its six steps with the first, cold one among them): 0.85 to 1.20 ms for the
five rank-form shapes (g ranks share the one GPU), 0.007 to 0.14 ms for the ordered-pair i-shards.  The late runs use
LATE_US = 12,000 us, ten times the slowest of these; every test that relies on the delay asserts LATE_US >= 5 x the force pass
its own worker measured.

One child process per (g, precision), five in all, each with a time limit of 120 s; a worker takes 3 to 6 s.

Engines with one thing changed fail here (once each, on an MI355X): rccl_exchange_wait without its stream wait -- the overlapped runs
of every rank-form shape and of the g = 2 i-shards, all G = 0.37 cases, all reads behind a late gather; receive pointer A -- every
rank-form test but the counters; send pointer base -- everything but the counters and the error cases; nb_download without
finish_gather -- every overlapped run and all reads behind a late gather.  (The overlapped i-shard run with g = 4 did not catch the
missing stream wait, though its reads behind the gather did: presumably its eight streams share the process's few hardware queues,
which can put an engine stream behind a late collective by accident.  g = 2 and 3 are where a missing wait shows.)
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rccl_shim_build
from conftest import ROOT, rel_pos_err
from oracle import oracle
from test_field_gpu import errors as field_errors, ref_field

pytestmark = pytest.mark.gpu

LATE_US = 12000
STEPS, DT = 6, 1e-3
WORKER = os.path.join(ROOT, "tests", "rccl_shim", "rccl_ranks_worker.py")
RANK_SHAPES = [("f32", 2), ("f32", 3), ("f32", 4), ("f64", 2), ("f64", 4)]
ISHARD_SHAPES = [("f32", 2), ("f32", 4), ("f64", 2)]
ISHARD_SPLIT = {("f32", 2), ("f64", 2)}          # the rows of the table whose own-row splits are asserted
G037 = [("rank", "f32", 3), ("rank", "f64", 2), ("ishard", "f32", 2), ("ishard", "f64", 2)]
COMBOS = ("o0l0", "o1l0", "o0l1", "o1l1")
_runs = {}


def worker(precision, g):
    """(arrays, meta) of one worker run; run once per (g, precision), failures remembered too."""
    key = (precision, g)
    if key not in _runs:
        try:
            import tempfile
            out = os.path.join(tempfile.mkdtemp(prefix="rccl_ranks_"), "g%d_%s.npz" % (g, precision))
            env = dict(os.environ, NB_RCCL_LIB=rccl_shim_build.build())
            p = subprocess.run([sys.executable, WORKER, out, str(g), precision, str(LATE_US)], capture_output=True, text=True, timeout=120, env=env)
            assert p.returncode == 0, "worker g=%d %s exited %d\n%s" % (g, precision, p.returncode, (p.stdout + p.stderr)[-4000:])
            with np.load(out) as f:
                z = {k: f[k] for k in f.files}
            _runs[key] = (z, json.loads(str(z.pop("meta"))))
        except BaseException as e:          # a second test of the same run does not start it again
            _runs[key] = e
    if isinstance(_runs[key], BaseException):
        raise _runs[key]
    return _runs[key]


@functools.lru_cache(maxsize=None)
def oracle_run(mode, precision, g, G):
    z, _ = worker(precision, g)
    key = mode.split("_")[0]
    b, v = z[key + "/b0"], z[key + "/v0"]
    run = oracle.run_f64 if precision == "f64" else oracle.run_f32
    return run(b, v, None, DT, G, STEPS)[0], oracle.accel_f64(b.astype(np.float64), G)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_late_enough(meta, key):
    force = max(t["force_ms"] + t["sym_reduce_ms"] for t in meta[key + "/o0l0"]["times"])
    print("%s: force pass %.4f ms on the slowest rank, delay %d us" % (key, force, LATE_US))
    assert force > 0 and LATE_US >= 5 * 1000 * force, (force, LATE_US)


def assert_identity(z, meta, key, g, combos):
    """the bytes of bodies, vel and accel are the same in every combination of overlap and delay, and on every rank"""
    for c in combos:
        for r in range(g):
            assert meta["%s/%s" % (key, c)]["info"][r] == [g, r, rccl_shim_build.VERSION], (c, r)
            assert same(z["%s/%s/bodies%d" % (key, c, r)], z["%s/%s/bodies0" % (key, combos[0])]), "%s: bodies of rank %d in %s" % (key, r, c)
        for what in ("vel", "acc"):
            assert same(z["%s/%s/%s" % (key, c, what)], z["%s/%s/%s" % (key, combos[0], what)]), "%s: %s in %s" % (key, what, c)


def assert_oracle(z, mode, precision, g, G, combo):
    n = len(z[mode.split("_")[0] + "/b0"])
    ref_b, ref_a = oracle_run(mode, precision, g, G)
    err = rel_pos_err(z["%s/%s/bodies0" % (mode, combo)][:n], ref_b, 1.0)
    a1 = z["%s/%s/accel1" % (mode, combo)][:n, :3].astype(np.float64)
    aerr = np.abs(a1 - ref_a[:, :3]).max() / np.abs(ref_a[:, :3]).max()
    print("%s %s g=%d G=%g: rel_pos_err %.3g, first-step accelerations %.3g" % (mode, precision, g, G, err, aerr))
    assert err < (1e-12 if precision == "f64" else 1e-6), err
    assert aerr < 2e-5, aerr


# ---- the rank form of the symmetric pass --------------------------------------------------------

@pytest.mark.parametrize("precision,g", RANK_SHAPES)
def test_rank_form_runs_both_collectives_every_step(precision, g):
    """A timed, non-overlapped run: the handle is in the rank form, one reduce-scatter and one all-gather per step, through the
    stand-in library (its version code, not RCCL's)."""
    z, meta = worker(precision, g)
    m = meta["rank/o0l0"]
    for r in range(g):
        t = m["times"][r]
        assert "symwrank" in m["variant"][r], m["variant"]
        assert t["launches"] == STEPS and t["reduce_scatters"] == STEPS and t["allgathers"] == STEPS, t
        assert t["sym_reduce_ms"] > 0 and t["force_ms"] > 0 and t["reduce_scatter_ms"] > 0 and t["allgather_ms"] > 0, t
        assert m["info"][r] == [g, r, rccl_shim_build.VERSION] and rccl_shim_build.VERSION < 20000
        assert m["info_detached"][r] == [0, 0, 0]
    assert_late_enough(meta, "rank")


@pytest.mark.parametrize("precision,g", RANK_SHAPES)
def test_rank_form_same_bytes_with_and_without_overlap_and_delay(precision, g):
    """Overlap off/on x delay 0/late: the same bytes of bodies on every rank (replica agreement) and of every rank's own rows of
    vel and accel.  A send pointer that is not base + row * sb, a receive offset that is not A + 4 * esz * sb or a missing
    wait for ev_done all end here."""
    z, meta = worker(precision, g)
    assert_late_enough(meta, "rank")
    assert_identity(z, meta, "rank", g, COMBOS)


@pytest.mark.parametrize("precision,g", RANK_SHAPES)
def test_rank_form_equals_the_multi_handle_in_peer_mode(precision, g):
    """nb_multi's virtual shards run the same kernels and sum the shards' partial accelerations in the same order (ascending,
    from +0): the same bytes on the caller's n rows.  (The multi handle gets the padded rows too: asked for 6,000 rows over 3
    shards it sees 2,000 rows per shard, below the 2,048 from which it takes the rank form, and only then rounds up to 2,048.)"""
    z, meta = worker(precision, g)
    n = meta["rank"]["n"]
    assert "symwrank" in meta["rank"]["multi_variant"], meta["rank"]
    for what, mine in (("bodies", "bodies0"), ("vel", "vel"), ("acc", "acc")):
        assert same(z["rank/o0l0/" + mine][:n], z["rank/multi/" + what][:n]), what


@pytest.mark.parametrize("precision,g", RANK_SHAPES)
def test_rank_form_against_the_oracle(precision, g):
    z, _ = worker(precision, g)
    assert_oracle(z, "rank", precision, g, 1.0, "o0l0")


# ---- ordered-pair i-shards -----------------------------------------------------------------------

@pytest.mark.parametrize("precision,g", ISHARD_SHAPES)
def test_ishard_same_bytes_with_and_without_overlap_and_delay(precision, g):
    """No SYM_SHARD: the all-gather alone, and with overlap the split launch (own-row partitions before the wait)."""
    z, meta = worker(precision, g)
    shapes = meta["ishard/o1l1"]["shape"]
    if (precision, g) in ISHARD_SPLIT:
        assert all(s["own_splits"] > 0 for s in shapes), shapes
    t = meta["ishard/o0l0"]["times"]
    assert all(x["launches"] == STEPS and x["allgathers"] == STEPS and x["reduce_scatters"] == 0 for x in t), t
    assert_late_enough(meta, "ishard")
    assert_identity(z, meta, "ishard", g, COMBOS)


@pytest.mark.parametrize("precision,g", ISHARD_SHAPES)
def test_ishard_equals_a_whole_system_handle(precision, g):
    """The same kernel with the same j-partitions on one unsharded handle: the same bytes, as test_rccl_attach_single_rank
    asserts for one rank; and both within the bounds of the oracle."""
    z, meta = worker(precision, g)
    m = meta["ishard"]
    assert m["twin_variant"] == meta["ishard/o0l0"]["variant"][0], m
    assert m["twin_shape"]["j_per_split"] == meta["ishard/o0l0"]["shape"][0]["j_per_split"], m
    for what, mine in (("bodies", "bodies0"), ("vel", "vel"), ("acc", "acc")):
        assert same(z["ishard/o0l0/" + mine], z["ishard/whole/" + what]), what
    assert_oracle(z, "ishard", precision, g, 1.0, "o0l0")


# ---- G != 1: the other ranks' rows of the j-stream copy are rebuilt from the gathered positions ----

@pytest.mark.parametrize("mode,precision,g", G037)
def test_g_037_rebuilds_the_j_stream_behind_the_gather(mode, precision, g):
    """Every collective late, overlap off and on: identical bytes, on every rank, within the bounds of the oracle at that G."""
    z, meta = worker(precision, g)
    assert_late_enough(meta, mode)
    key = mode + "_g037"
    assert_identity(z, meta, key, g, ("o0l1", "o1l1"))
    assert not same(z[key + "/o0l1/bodies0"], z[mode + "/o0l0/bodies0"])          # G did change the run
    if mode == "ishard":
        for what, mine in (("bodies", "bodies0"), ("vel", "vel"), ("acc", "acc")):
            assert same(z[key + "/o0l1/" + mine], z[key + "/whole/" + what]), what
    assert_oracle(z, key, precision, g, 0.37, "o0l1")


# ---- reads behind a late gather --------------------------------------------------------------------

@pytest.mark.parametrize("mode,precision,g", [("rank",) + s for s in RANK_SHAPES] + [("ishard",) + s for s in ISHARD_SHAPES])
def test_reads_behind_a_late_gather(mode, precision, g):
    """Overlap on, every collective late; straight behind its last nb_step, with no nb_sync, each rank downloads, asks for the
    nearest neighbour of every row and for the field at 64 points -- three runs, each call once in first place, where it meets
    the pending gather itself.  The download is the plain run's final state; index and dist2 are exactly those of a fresh
    whole-system handle loaded with that state; the field is within tests/test_field_gpu.py's bounds of the host fp64 sum."""
    z, meta = worker(precision, g)
    assert_late_enough(meta, mode)
    truth = z[mode + "/o0l0/bodies0"]
    rows = meta[mode]["rows"]
    ra, rf = ref_field(truth, z[mode + "/pts"])
    tol = 1e-12 if precision == "f64" else 2e-5
    for first in ("read", "nbr", "field"):
        k = "%s/reads_%s/" % (mode, first)
        for r in range(g):
            assert same(z[k + "bodies%d" % r], truth), (first, r)
            for what in ("vel", "acc"):
                own = slice(r * rows, (r + 1) * rows)
                assert same(z[k + "%s%d" % (what, r)][own], z["%s/o0l0/%s" % (mode, what)][own]), (first, what, r)
            assert same(z[k + "idx%d" % r], z[mode + "/fresh/idx"]), (first, r)
            assert same(z[k + "d2%d" % r], z[mode + "/fresh/d2"]), (first, r)
            ea, ef = field_errors(z[k + "fa%d" % r], z[k + "fphi%d" % r], ra, rf)
            assert ea <= tol and ef <= tol, (first, r, ea, ef)
            for what in ("fa", "fphi"):
                assert same(z[k + "%s%d" % (what, r)], z[k + what + "0"]), (first, what, r)          # rank 0 and every other rank: the same bytes


# ---- what nb_rccl_attach refuses with two ranks ----------------------------------------------------

def test_partition_errors_with_two_ranks():
    _, meta = worker("f32", 2)
    p = meta["partition"]
    assert "NB_ERR_INVALID" in p["quarter_as_rank0_of_2"], p          # shard=(256, 256) of 1024 is no half
    assert "NB_ERR_INVALID" in p["first_block_as_rank1"], p           # rank 1 owns the second block
    for r in (0, 1):
        assert p["ranks"][r]["info"] == [2, r, rccl_shim_build.VERSION], p
        assert p["ranks"][r]["still"] == [2, r, rccl_shim_build.VERSION], p
        assert p["ranks"][r]["detached"] == [0, 0, 0], p
    assert "NB_ERR_STATE" in p["ranks"][1]["second"], p               # a second attach


def test_an_aborted_group_fails_the_step_on_every_rank():
    """The stand-in library's abort flag (what a timed-out barrier or a HIP error inside it sets), raised between two steps of two
    attached ranks: nb_step returns NB_ERR_COMM on both and the worker ends by itself."""
    _, meta = worker("f32", 2)
    assert all("NB_ERR_COMM" in e for e in meta["abort"]), meta["abort"]
