"""Child process of tests/test_rccl_ranks_gpu.py: the engine's native collective path (nb_rccl_attach) with g ranks on ONE GPU.

Started with NB_RCCL_LIB pointing at the stand-in library of tests/rccl_shim (the engine reads the variable once per process, so
it cannot be set inside pytest's own).  One Python thread per rank (ctypes releases the GIL), each with its own shard handle,
attached to one communicator; every thread uploads the same padded arrays and steps as nb_step(1), nb_step(1), nb_step(4).
One run covers one (g, precision) pair and every mode the test asks of it; the reference results -- nb_multi in peer mode, plain
whole-system handles -- are computed in the same process.  Everything goes, unjudged, into the .npz named by argv[1].

    rccl_ranks_worker.py OUT.npz G PRECISION LATE_US
"""
import ctypes
import json
import os
import sys
import threading
import traceback

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "nbody3d-webgpu_amd"))

from nbody3d_amd import MultiSimulation, Simulation, capi, ic  # noqa: E402

DT = 1e-3
STEPS = (1, 1, 4)
# (precision, g) -> n of the rank-form shape (nb_multi pads to whole super-blocks per shard: 6000 -> 3 x 2048)
RANK_FORM = {("f32", 2): 4096, ("f32", 3): 6000, ("f32", 4): 8192, ("f64", 2): 4096, ("f64", 4): 8192}
# (precision, g) -> (n, configuration) of the ordered-pair i-shard shape
ISHARD = {("f32", 2): (4096, dict(force_variant=28, jsplit=4)), ("f32", 4): (8192, dict(flags=capi.NB_FLAG_NO_SYM)), ("f64", 2): (2048, dict(jsplit=4))}
G037_RANK = {("f32", 3), ("f64", 2)}
G037_ISHARD = {("f32", 2), ("f64", 2)}
SEED = {"f32": 61, "f64": 62}


def padded(a, n_pad):
    out = np.zeros((n_pad, 4), a.dtype)          # zero-mass rows at the origin, zero velocity: as nb_multi_upload pads
    out[:len(a)] = a
    return out


def field_points(b, m=64):
    rng = np.random.default_rng(7)
    lo, hi = b[:, :3].min(0), b[:, :3].max(0)
    near = b[rng.integers(0, len(b), m // 2), :3] + rng.normal(0, 0.02, (m // 2, 3))
    box = lo + (hi - lo) * rng.random((m - m // 2, 3))
    return np.concatenate([near, box]).astype(b.dtype)


class Ranks:
    """g rank threads over one communicator."""

    def __init__(self, shim, g, precision, n_pad, b, v, kw):
        self.shim, self.g, self.precision, self.n_pad, self.b, self.v, self.kw = shim, g, precision, n_pad, b, v, kw
        self.rows = n_pad // g
        self.create = threading.Lock()
        self.errors = []

    def run(self, *, overlap, late_us, G=1.0, timing=False, first_accel=False, after=None):
        os.environ["NB_SHIM_LATE_US"] = str(int(late_us))          # read by the library when a communicator is created
        uid = capi.rccl_unique_id()
        out = [None] * self.g
        threads = [threading.Thread(target=self._rank, args=(r, uid, out, overlap, G, timing, first_accel, after)) for r in range(self.g)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if self.errors:
            raise RuntimeError("rank thread failed:\n" + "\n".join(self.errors))
        return out

    def _rank(self, r, uid, out, overlap, G, timing, first_accel, after):
        sim = None
        try:
            with self.create:
                sim = Simulation(self.n_pad, precision=self.precision, shard=(r * self.rows, self.rows), **self.kw)
            res = {"variant": sim.variant, "shape": sim.shape_info()}
            sim.rccl_attach(uid, self.g, r, overlap=overlap)
            res["info"] = sim.rccl_info()
            sim.init(self.b, self.v)
            sim.set_params(DT, G)
            sim.enable_timing(timing)
            for k, steps in enumerate(STEPS):
                sim.simulate(steps)
                if k == 0 and first_accel:
                    res["accel1"] = sim.read(bodies=False, vel=False)[2]
            if after is not None:
                res["after"] = after(sim, r)          # straight behind the last nb_step: no nb_sync first
            if timing:
                res["times"] = sim.step_breakdown()
            res["bodies"], res["vel"], res["acc"] = sim.read()
            sim.rccl_detach()
            res["info_detached"] = sim.rccl_info()
            out[r] = res
        except Exception:
            self.errors.append("rank %d: %s" % (r, traceback.format_exc()))
            self.shim.nb_shim_abort_all()             # nobody may wait for this rank
        finally:
            if sim is not None:
                sim.close()


def store(z, key, out, rows):
    """bodies of every rank; vel, accel (and the first step's accel) merged from every rank's own rows"""
    g = len(out)
    for r, res in enumerate(out):
        z["%s/bodies%d" % (key, r)] = res["bodies"]
    for what in ("vel", "acc", "accel1"):
        if what in out[0]:
            z["%s/%s" % (key, what)] = np.concatenate([out[r][what][r * rows:(r + 1) * rows] for r in range(g)])


def combos(z, meta, ranks, key, G, late_us, which):
    for overlap, late in which:
        tag = "%s/o%dl%d" % (key, overlap, int(late > 0))
        # the plain run also carries the timing; without overlap a download after the first step changes nothing that follows
        out = ranks.run(overlap=bool(overlap), late_us=late, G=G, timing=(overlap, late) == (0, 0), first_accel=not overlap)
        store(z, tag, out, ranks.rows)
        meta[tag] = {"variant": [o["variant"] for o in out], "shape": [o["shape"] for o in out], "info": [o["info"] for o in out],
                     "info_detached": [o["info_detached"] for o in out], "times": [o.get("times") for o in out]}


def reads_behind(z, meta, ranks, key, late_us, pts):
    """Overlap on, every collective late; each rank asks straight behind its last nb_step -- once with each kind of call first, so
    that each of them meets the pending gather itself."""
    n_pad = ranks.n_pad

    def make(order):
        def after(sim, r):
            got = {}
            for what in order:
                if what == "read":
                    got["bodies"], got["vel"], got["acc"] = sim.read()
                elif what == "nbr":
                    got["idx"], got["d2"], _ = sim.neighbors(bodies=(0, n_pad))
                else:
                    got["fa"], got["fphi"] = sim.field(pts)
            return got
        return after

    for order in (("read", "nbr", "field"), ("nbr", "field", "read"), ("field", "read", "nbr")):
        out = ranks.run(overlap=True, late_us=late_us, after=make(order))
        for r, res in enumerate(out):
            for k, a in res["after"].items():
                z["%s/reads_%s/%s%d" % (key, order[0], k, r)] = a
    meta[key + "/reads"] = True


def partition_errors(shim):
    """What nb_rccl_attach refuses with two ranks, before any collective starts."""
    got = {}
    uid = capi.rccl_unique_id()

    def code(fn):
        try:
            fn()
            return "no error"
        except capi.NBodyError as e:
            return str(e)

    with Simulation(1024, shard=(256, 256)) as s:
        got["quarter_as_rank0_of_2"] = code(lambda: s.rccl_attach(uid, 2, 0))
    with Simulation(1024, shard=(0, 512)) as s:
        got["first_block_as_rank1"] = code(lambda: s.rccl_attach(uid, 2, 1))
    res, errors = [None, None], []

    def rank(r):
        try:
            with Simulation(1024, shard=(r * 512, 512)) as s:
                s.rccl_attach(uid, 2, r)
                a = s.rccl_info()
                second = code(lambda: s.rccl_attach(uid, 2, r)) if r == 1 else None
                still = s.rccl_info()
                s.rccl_detach()
                res[r] = {"info": a, "second": second, "still": still, "detached": s.rccl_info()}
        except Exception:
            errors.append(traceback.format_exc())
            shim.nb_shim_abort_all()

    th = [threading.Thread(target=rank, args=(r,)) for r in (0, 1)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errors:
        raise RuntimeError("\n".join(errors))
    got["ranks"] = res
    return got


def abort_ends_a_step(shim):
    """The library's abort flag, set while two ranks are attached: nb_step fails with NB_ERR_COMM on both, nobody waits."""
    uid = capi.rccl_unique_id()
    b, v = ic.plummer(1024, seed=63)
    res, errors = [None, None], []
    attached = threading.Barrier(2, timeout=60)

    def rank(r):
        try:
            with Simulation(1024, shard=(r * 512, 512)) as s:
                s.rccl_attach(uid, 2, r)
                s.init(b, v)
                s.set_params(DT, 1.0)
                s.simulate(1)
                attached.wait()
                if r == 1:
                    shim.nb_shim_abort_all()
                attached.wait()
                try:
                    s.simulate(1)
                    res[r] = "no error"
                except capi.NBodyError as e:
                    res[r] = str(e)
        except Exception:
            errors.append(traceback.format_exc())
            shim.nb_shim_abort_all()
            attached.abort()

    th = [threading.Thread(target=rank, args=(r,)) for r in (0, 1)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    if errors:
        raise RuntimeError("\n".join(errors))
    return res


def twin_config(n, precision, rows, kw):
    """The whole-system handle that runs the i-shard handles' kernel with their j-partitions (no fused step)."""
    q = capi.plan_query(n, precision=precision, shard=(0, rows), n_cu=0, clock_hz=0, **kw)
    code = q["kind"] * 100000 + q["ipl"] * 1000 + q["ls"] * 10 + q["x"]
    return dict(force_variant=code, jsplit=q["jsplit"], flags=kw.get("flags", 0) | capi.NB_FLAG_NO_FUSE)


def stepped(sim, b, v, G):
    sim.init(b, v)
    sim.set_params(DT, G)
    for steps in STEPS:
        sim.simulate(steps)
    return sim.read()


def main():
    out_path, g, precision, late_us = sys.argv[1], int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
    shim = ctypes.CDLL(os.environ["NB_RCCL_LIB"])       # the same mapping the engine opens
    dtype = np.float64 if precision == "f64" else np.float32
    z, meta = {}, {"g": g, "precision": precision, "late_us": late_us}
    four = ((0, 0), (1, 0), (0, late_us), (1, late_us))

    if (precision, g) in RANK_FORM:
        n = RANK_FORM[(precision, g)]
        align = 512 if precision == "f64" else 1024
        rows = (n + g - 1) // g
        rows = (rows + align - 1) // align * align          # whole super-blocks per rank, as nb_multi_create lays them out
        n_pad = rows * g
        b, v = (a.astype(dtype) for a in ic.plummer(n, seed=SEED[precision]))
        bp, vp = padded(b, n_pad), padded(v, n_pad)
        meta["rank"] = {"n": n, "n_pad": n_pad, "rows": rows}
        z["rank/b0"], z["rank/v0"] = b, v
        ranks = Ranks(shim, g, precision, n_pad, bp, vp, dict(flags=capi.NB_FLAG_SYM_SHARD))
        combos(z, meta, ranks, "rank", 1.0, late_us, four)
        # The multi handle is given the padded rows: nb_multi_create takes the rank form from 2,048 rows per shard BEFORE it rounds
        # the shards up to whole super-blocks, so 6,000 rows over 3 shards (2,000 each) would run the ordered-pair kernels.
        with MultiSimulation(n_pad, g, precision=precision) as ms:
            meta["rank"]["multi_variant"] = ms.variant
            z["rank/multi/bodies"], z["rank/multi/vel"], z["rank/multi/acc"] = stepped(ms, bp, vp, 1.0)
        pts = field_points(b)
        z["rank/pts"] = pts
        reads_behind(z, meta, ranks, "rank", late_us, pts)
        with Simulation(n_pad, precision=precision) as fresh:      # a whole system loaded with the final state of the plain run
            fresh.init(z["rank/o0l0/bodies0"], z["rank/o0l0/vel"])
            fresh.set_params(DT, 1.0)
            z["rank/fresh/idx"], z["rank/fresh/d2"], _ = fresh.neighbors(bodies=(0, n_pad))
        if (precision, g) in G037_RANK:
            combos(z, meta, ranks, "rank_g037", 0.37, late_us, ((0, late_us), (1, late_us)))

    if (precision, g) in ISHARD:
        n, kw = ISHARD[(precision, g)]
        rows = n // g
        b, v = (a.astype(dtype) for a in ic.plummer(n, seed=SEED[precision] + 10))
        meta["ishard"] = {"n": n, "n_pad": n, "rows": rows}
        z["ishard/b0"], z["ishard/v0"] = b, v
        ranks = Ranks(shim, g, precision, n, b, v, kw)
        combos(z, meta, ranks, "ishard", 1.0, late_us, four)
        twin = twin_config(n, precision, rows, kw)
        meta["ishard"]["twin"] = twin
        with Simulation(n, precision=precision, **twin) as one:
            meta["ishard"]["twin_variant"], meta["ishard"]["twin_shape"] = one.variant, one.shape_info()
            z["ishard/whole/bodies"], z["ishard/whole/vel"], z["ishard/whole/acc"] = stepped(one, b, v, 1.0)
        pts = field_points(b)
        z["ishard/pts"] = pts
        reads_behind(z, meta, ranks, "ishard", late_us, pts)
        with Simulation(n, precision=precision) as fresh:
            fresh.init(z["ishard/o0l0/bodies0"], z["ishard/o0l0/vel"])
            fresh.set_params(DT, 1.0)
            z["ishard/fresh/idx"], z["ishard/fresh/d2"], _ = fresh.neighbors(bodies=(0, n))
        if (precision, g) in G037_ISHARD:
            combos(z, meta, ranks, "ishard_g037", 0.37, late_us, ((0, late_us), (1, late_us)))
            with Simulation(n, precision=precision, **twin) as one:
                z["ishard_g037/whole/bodies"], z["ishard_g037/whole/vel"], z["ishard_g037/whole/acc"] = stepped(one, b, v, 0.37)

    if (precision, g) == ("f32", 2):
        meta["partition"] = partition_errors(shim)
        meta["abort"] = abort_ends_a_step(shim)

    z["meta"] = np.array(json.dumps(meta))
    np.savez(out_path, **z)
    print("worker ok: g=%d %s, %d arrays" % (g, precision, len(z)))


if __name__ == "__main__":
    main()
