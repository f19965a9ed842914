"""Every query on handles that have STEPPED, against a fresh twin (tests/query_state.py has the request set and the comparison).

Per case: upload ic.plummer(n, seed=21), set (dt = 1e-2, G), then per checkpoint simulate(k) and -- nothing in between, no sync, no
read: either would wait for the stream and finish a pending gather -- every query; only then read() the state, load it into the
twin (a plain handle of the same n and precision that never steps; a fresh Hermite handle for the Hermite kinds) and ask the twin.
Neighbours, lists, k nearest and list forces must equal the twin's bit for bit, the frame the downloaded bodies; field and
diagnostics lie within 2e-5 (f32) / 1e-12 (f64, NB_FIELD_F64) of the host fp64 sums over the downloaded state and, between two
whole-system handles of one n and precision, equal the twin's in bits.  Multi handles are held to the tolerance alone there: shard 0
answers with the padded row count, which changes field_shape, and the diagnostics are summed shard by shard.

The control, at the first checkpoint of every case: the twin loaded with the state one step earlier (the uploaded one) must FAIL
every category (query_state.stale_must_fail; tests/test_query_state_cpu.py derives the row counts this relies on)."""
import numpy as np
import pytest

from conftest import torch
from nbody3d_amd import MultiSimulation, Simulation
from query_state import answers, changed_rows, compare, is_exact, load_twin, make_twin, requests, stale_must_fail
from test_eqm_gpu import hip_runtime

pytestmark = pytest.mark.gpu

DT, SEED = 1e-2, 21

# id: (n, precision, how the handle is made, family its variant must name, G, checkpoints)
CASES = {
    "fused_regs": (1000, "f32", {}, "fused_regs", 1.0, (1, 2, 17, 3)),
    "fused_lds": (2002, "f32", dict(force_variant=402644), "fused_lds", 1.0, (1, 2, 17, 3)),
    "jpacked_js0": (2002, "f32", dict(force_variant=601014, jsplit=0), "fused_jpairs", 0.37, (1, 2, 17)),
    "jpacked_js3": (2002, "f32", dict(force_variant=601014, jsplit=3), "fused_jpairs", 0.37, (1, 2, 17)),
    "two_kernel_lds": (1001, "f32", dict(force_variant=22, jsplit=2), "f32pk_lds256", 1.0, (1, 2, 17)),
    "two_kernel_sgpr": (1001, "f32", dict(force_variant=304014), "f32pk_sgpr", 0.37, (1, 17)),
    "symmetric": (2002, "f32", dict(force_variant=704013), "f32pk_symw_", 1.0, (1, 2, 33)),
    "symmetric_eqm": (2048, "f32", dict(force_variant=708013), "f32pk_symw_", 1.0, (1, 17)),
    "f64_ordered": (1000, "f64", {}, "f64_lds", 1.0, (1, 2, 17)),
    "f64_symmetric": (2002, "f64", dict(force_variant=708013), "f64_symw_", 1.0, (1, 2)),
    "hermite_f32": (1000, "f32", dict(integrator="hermite4"), "hermite4_f32", 1.0, (1, 2, 4)),
    "hermite_f64": (1000, "f64", dict(integrator="hermite4"), "hermite4_f64", 1.0, (1, 2, 4)),
    "block_f32": (1000, "f32", dict(integrator="hermite4", block=True), "hermite4_f32", 1.0, (1, 2)),
    "block_f64": (1000, "f64", dict(integrator="hermite4", block=True), "hermite4_f64", 1.0, (1, 2)),
    "multi_ordered_padded": (1000, "f32", dict(multi=3), "f32", 1.0, (1, 2, 17)),
    "multi_rank_overlap_f32": (4100, "f32", dict(multi=2, collective="peer_overlap"), "symwrank", 1.0, (1, 2, 5)),
    "multi_rank_overlap_f64": (4100, "f64", dict(multi=2, collective="peer_overlap"), "symwrank", 1.0, (1, 2, 5)),
}

_requests = {}


def request_set(n, precision, hermite):
    """One request set per (n, precision, hermite), shared and read-only."""
    key = (n, precision, hermite)
    if key not in _requests:
        _requests[key] = requests(n, np.float64 if precision == "f64" else np.float32, SEED, hermite)
    return _requests[key]


def make(case):
    n, precision, how, family, G, _ = CASES[case]
    how = dict(how)
    block = how.pop("block", False)
    if "multi" in how:
        sim = MultiSimulation(n, how.pop("multi"), precision=precision, **how)
    else:
        sim = Simulation(n, precision=precision, **how)
    try:
        assert family in sim.variant, (case, sim.variant)
        if case == "multi_ordered_padded":
            assert "sym" not in sim.variant, sim.variant
        if block:
            sim.set_block_steps()
            assert sim.block_stats()["enabled"] == 1
    except BaseException:
        sim.close()
        raise
    return sim


class Walk:
    """One handle and its twin: checkpoint() is the protocol of the module docstring."""

    def __init__(self, kind, sim, twin, req, precision, G):
        self.kind, self.sim, self.twin, self.req, self.precision, self.G = kind, sim, twin, req, precision, G
        self.multi = isinstance(sim, MultiSimulation)
        self.steps, self.worst, self.last = 0, {}, None
        sim.init(req["bodies"], req["vel"])
        sim.set_params(DT, G)
        self.state = (req["bodies"], req["vel"], np.zeros_like(req["bodies"]))

    def where(self, what):
        return "%s (%s), %s after %d steps" % (self.kind, self.sim.variant, what, self.steps)

    def ask(self, what, control=False):
        """Every query on the handle as it stands, then the read, then the twin."""
        older = self.state
        got = answers(self.sim, self.req)                                   # nothing between the step and the queries
        self.state = self.sim.read()
        want = answers(load_twin(self.twin, self.state, DT, self.G), self.req)
        fig = compare(got, want, self.state, self.req, self.precision, not self.multi, G=self.G,
                      steps=None if self.multi else self.steps, where=self.where(what))
        for k, (e, _) in fig.items():
            self.worst[k] = max(self.worst.get(k, 0.0), e)
        if control:
            stale = answers(load_twin(self.twin, older, DT, self.G), self.req)
            stale_must_fail(got, stale, older, self.req, self.precision, G=self.G, where=self.where(what))
        self.last = got
        return got

    def checkpoint(self, k, control=False):
        self.sim.simulate(k)
        self.steps += k
        return self.ask("simulate(%d)" % k, control)

    def change_G(self, G):
        """A later nb_set_params is followed without a step: field, list forces and diagnostics scale, the neighbours stay."""
        before = self.last
        self.G = G
        self.sim.set_params(DT, G)
        got = self.ask("set_params(G = %g)" % G)
        for name in got:
            geometry = is_exact(name) and not name.startswith("lf_")
            same = len(changed_rows(got[name], before[name])) == 0
            if geometry or name.startswith("frame"):
                assert same, self.where("set_params") + ": %s changed with G" % name
            else:
                assert not same, self.where("set_params") + ": %s did not follow G" % name


@pytest.mark.parametrize("case", list(CASES))
def test_queries_answer_on_the_stepped_state(case):
    n, precision, how, _, G, checkpoints = CASES[case]
    hermite = how.get("integrator") == "hermite4"
    req = request_set(n, precision, hermite)
    with make(case) as sim, make_twin(n, precision, hermite) as twin:
        w = Walk(case, sim, twin, req, precision, G)
        if case == "symmetric_eqm":
            assert sim.eqm_form == 2, sim.eqm_form                       # equal masses, G m a power of two
        if "collective" in how:
            assert sim.collective_info()["mode"] == how["collective"]
        for i, k in enumerate(checkpoints):
            w.checkpoint(k, control=(i == 0))
        w.change_G(2.5)
        print("%s: worst %s" % (case, ", ".join("%s %.2e" % kv for kv in sorted(w.worst.items()))))


def fused_lds_at_odd_parity():
    n, precision, how, family, G, _ = CASES["fused_lds"]
    req = request_set(n, precision, False)
    sim, twin = make("fused_lds"), make_twin(n, precision)
    w = Walk("fused_lds", sim, twin, req, precision, G)
    w.checkpoint(3)                                                      # an odd number of ping-pong steps
    return sim, twin, w, req


def test_restore_at_odd_parity():
    sim, twin, w, req = fused_lds_at_odd_parity()
    with sim, twin:
        b = req["bodies"].copy()
        b[:, :3] *= np.float32(1.25)
        sim.init(b, req["vel"])
        w.ask("init() of another state")
        assert w.state[0].tobytes() == b.tobytes()
        w.checkpoint(1)
        w.checkpoint(2)


def test_positions_written_through_the_device_pointer():
    sim, twin, w, req = fused_lds_at_odd_parity()
    with sim, twin:
        b = req["bodies"].copy()
        b[:, :3] = b[::-1, :3] * np.float32(0.8)                          # other positions, the masses as they are
        sim.sync()
        p = sim.device_ptr("bodies")
        assert hip_runtime().hipMemcpy(p, b.ctypes.data, b.nbytes, 1) == 0
        w.ask("a write through nb_device_ptr(NB_BODIES)")
        assert w.state[0].tobytes() == b.tobytes()
        w.checkpoint(1)


@pytest.mark.parametrize("case", ["symmetric", "f64_ordered"])
def test_device_pointer_forms_back_to_back_behind_the_steps(case):
    """simulate(17) and the five device-pointer forms enqueued on one torch stream with no host sync in between: the outputs equal
    the host forms called afterwards, bit for bit (one handle, one m: the launch shapes of the field are the same)."""
    assert torch is not None
    n, precision, how, family, G, _ = CASES[case]
    req = request_set(n, precision, False)
    stream = torch.cuda.Stream()
    ft = torch.float64 if precision == "f64" else torch.float32
    m, (first, count), cap, k = len(req["points"]), req["range"], req["cap"], req["k"]
    lrows, lcap = req["lists"].shape
    with Simulation(n, precision=precision, stream=stream.cuda_stream, **how) as sim:
        assert family in sim.variant, sim.variant
        sim.init(req["bodies"], req["vel"])
        sim.set_params(DT, G)
        with torch.cuda.stream(stream):
            dev = lambda a: torch.from_numpy(np.array(a)).to("cuda")          # (a copy: the request set is read-only)
            new = lambda shape, t: torch.full(shape, 7, device="cuda", dtype=t)
            pts, radii = dev(req["points"]), dev(req["radii"])
            lists, cnt = dev(req["lists"].view(np.int32)), dev(req["count"].view(np.int32))
            out = {"nbr_pts.index": new((m,), torch.int32), "nbr_pts.dist2": new((m,), ft), "nbr_pts.count": new((m,), torch.int32),
                   "knn_pts.index": new((m, k), torch.int32), "knn_pts.dist2": new((m, k), ft),
                   "nbl_bod.list": new((count, cap), torch.int32), "nbl_bod.count": new((count,), torch.int32),
                   "nbl_bod.index": new((count,), torch.int32), "nbl_bod.dist2": new((count,), ft),
                   "lf_bod.accel": new((count, 4), ft), "lf_bod.phi": new((count,), ft),
                   "lf_pts.accel": new((m, 4), ft), "lf_pts.phi": new((m,), ft),
                   "field_pts.accel": new((m, 4), ft), "field_pts.phi": new((m,), ft),
                   "field_bod.accel": new((count, 4), ft), "field_bod.phi": new((count,), ft)}
            ptr = {key: t.data_ptr() for key, t in out.items()}
        stream.synchronize()                                             # the uploads; from here on nothing waits
        sim.simulate(17)
        sim.neighbors_device(pts.data_ptr(), m, ptr["nbr_pts.index"], ptr["nbr_pts.dist2"], ptr["nbr_pts.count"], radii_ptr=radii.data_ptr())
        sim.knn_device(pts.data_ptr(), m, k, ptr["knn_pts.index"], ptr["knn_pts.dist2"])
        sim.neighbor_lists_device(None, 0, ptr["nbl_bod.list"], cap, ptr["nbl_bod.count"], ptr["nbl_bod.index"], ptr["nbl_bod.dist2"],
                                  bodies=(first, count), radius=req["radius"])
        sim.list_force_device(lists.data_ptr(), 0, lcap, bodies=(first, count), count_ptr=cnt.data_ptr(), accel_ptr=ptr["lf_bod.accel"],
                              phi_ptr=ptr["lf_bod.phi"])
        sim.list_force_device(lists.data_ptr(), m, lcap, points_ptr=pts.data_ptr(), count_ptr=cnt.data_ptr(), accel_ptr=ptr["lf_pts.accel"],
                              phi_ptr=ptr["lf_pts.phi"])
        sim.field_device(pts.data_ptr(), m, ptr["field_pts.accel"], ptr["field_pts.phi"])
        sim.field_device(None, 0, ptr["field_bod.accel"], ptr["field_bod.phi"], bodies=(first, count))
        stream.synchronize()
        host = answers(sim, req)
        bad = []
        for key, t in out.items():
            got = t.cpu().numpy()
            got = got.view(np.uint32) if got.dtype == np.int32 else got
            r = changed_rows(got, host[key])
            if len(r):
                bad.append("%s: %d rows differ from the host form, first rows %s" % (key, len(r), r[:5].tolist()))
        assert not bad, "%s (%s), device-pointer forms behind simulate(17):\n  %s" % (case, sim.variant, "\n  ".join(bad))
        # ... and the host forms themselves are right on this state
        state = sim.read()
        with make_twin(n, precision) as twin:
            want = answers(load_twin(twin, state, DT, G), req)
        compare(host, want, state, req, precision, True, G=G, steps=17, where="%s (%s) on a torch stream, after simulate(17)" % (case, sim.variant))


def test_shard_handle_with_a_gather_in_flight():
    """Two shard handles on one GPU with the two-phase exchange hook (the set-up of test_parity_gpu.py's overlapped exchange): after
    a step the gather of the other rank's rows is pending.  The first query finishes it -- wait() is called once, by the query and
    not by a read -- and the answers are those of the twin on all rows after that step; the next step does not wait again."""
    assert torch is not None
    n, g, steps, G = 4096, 2, 2, 1.0
    per = n // g
    req = request_set(n, "f32", False)
    kw = dict(force_variant=22, jsplit=8)                                # j_per_split = 512 divides the shard rows
    stream = torch.cuda.current_stream().cuda_stream
    bufs = [torch.empty((n, 4), device="cuda", dtype=torch.float32) for _ in range(g)]
    sims = [Simulation(n, shard=(r * per, per), stream=stream, ext_bodies=bufs[r].data_ptr(), **kw) for r in range(g)]
    twin = make_twin(n, "f32")
    snap, waits = {}, [0] * g
    try:
        for r, s in enumerate(sims):
            assert "f32pk_lds256" in s.variant and s.shape_info()["own_splits"] > 0, (s.variant, s.shape_info())
            s.init(req["bodies"], req["vel"])
            s.set_params(DT, G)

            def wait(st, r=r):
                waits[r] += 1
                for q in range(g):
                    if q != r:
                        bufs[r][q * per:(q + 1) * per].copy_(snap[q])
                return 0

            s.set_exchange_overlapped(lambda *a: 0, wait)
        for k in range(steps):
            before = list(waits)
            sims[0].step()
            assert waits[0] == before[0], "rank 0's step waited again for the gather a query had finished"
            sims[1].step()
            assert waits[1] == before[1] + (1 if k else 0)                # rank 1's gather of step k - 1 was still pending
            snap = {q: bufs[q][q * per:(q + 1) * per].clone() for q in range(g)}      # every rank's rows after step k
            w0 = waits[0]
            got = answers(sims[0], req)                                  # gather_pending is set: the first query finishes it
            assert waits[0] == w0 + 1, "the queries called wait() %d times for the pending gather" % (waits[0] - w0)
            state = sims[0].read()
            assert waits[0] == w0 + 1
            rows = np.concatenate([bufs[q][q * per:(q + 1) * per].cpu().numpy() for q in range(g)])
            assert state[0].tobytes() == rows.tobytes(), "rank 0 does not hold every rank's rows after step %d" % (k + 1)
            want = answers(load_twin(twin, state, DT, G), req)
            compare(got, want, state, req, "f32", False, G=G, shard=(0, per),
                    where="shard handle 0 of %d (%s), gather in flight after step %d" % (g, sims[0].variant, k + 1))
        for s in sims:
            s.sync()
    finally:
        for s in sims:
            s.close()
        twin.close()
