"""What the six queries (nb_field_eval, nb_neighbors, nb_neighbor_lists, nb_knn, nb_list_force, nb_split_force), their five *_shape
getters and the six nb_multi_* wrappers did BEFORE they were given one prologue, one staging path and one batch rule -- as data:
tests/golden/measure_query_parent.py records it from a build of that commit, tests/test_query_parent_gpu.py holds every later build
to it.  Three parts:

  * shapes: every *_shape getter on whole-system handles (the getters launch nothing; the rule depends on the device's compute-unit
    count, which is recorded with them);
  * messages: one request per distinct failure of the queries, the getters and the wrappers, each with exactly one fault: the return
    code and the full text of nb_last_error / nb_multi_last_error;
  * bits: SHA-256 of every array query_state.answers() returns for query_state.requests(771, ...) on fresh handles (init and
    set_params, no step), and of split_force at points and at bodies.  At n = 771 the field pass has four j-chunks: a changed cut or
    a wrong batch offset moves float bits that the tolerances of the other tests would let pass."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

from nbody3d_amd import MultiSimulation, Simulation, capi, ic

JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "query_parent.json")

# ---- shapes --------------------------------------------------------------------------------------------------------------------------

SHAPE_N = (300, 4099, 6144, 262144)                 # the first three: what the queries' own tests use
SHAPE_M = (1, 2, 257, 5000, 65536 + 300, 262144 + 300, 300000, 1 << 22)
SHAPE_CAP = (1, 64, 4096)
SHAPE_K = (1, 6, 64)
SHAPE_HANDLES = [(n, p, False) for n in SHAPE_N for p in ("f32", "f64")] + [(4099, "f32", True)]      # (n, precision, Hermite)


def handle_id(n, precision, hermite):
    return "%d_%s%s" % (n, precision, "_hermite" if hermite else "")


def make(n, precision, hermite=False):
    return Simulation(n, precision=precision, integrator="hermite4") if hermite else Simulation(n, precision=precision)


def compute_units():
    import torch
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def shapes_of(sim):
    """{getter(arguments): the dict it returns} for every (m, cap | k) of the lists above."""
    out = {}
    for m in SHAPE_M:
        out["neighbors(%d)" % m] = sim.neighbors_shape(m)
        out["split_force(%d)" % m] = sim.split_force_shape(m)
        for cap in SHAPE_CAP:
            out["neighbor_lists(%d, %d)" % (m, cap)] = sim.neighbor_lists_shape(m, cap)
            out["list_force(%d, %d)" % (m, cap)] = sim.list_force_shape(m, cap)
        for k in SHAPE_K:
            out["knn(%d, %d)" % (m, k)] = sim.knn_shape(m, k)
    return out


def all_shapes():
    out = {}
    for n, precision, hermite in SHAPE_HANDLES:
        with make(n, precision, hermite) as sim:
            out[handle_id(n, precision, hermite)] = shapes_of(sim)
    return out


# ---- messages ------------------------------------------------------------------------------------------------------------------------

MSG_N, MSG_M = 64, 8                                 # bodies of the handles, points of the requests
QUERIES = ("field_eval", "neighbors", "neighbor_lists", "knn", "list_force", "split_force")
GETTERS = ("neighbors", "neighbor_lists", "knn", "list_force", "split_force")
REQUEST = {"field_eval": capi.nb_field_request, "neighbors": capi.nb_neighbor_request, "neighbor_lists": capi.nb_neighbor_list_request,
           "knn": capi.nb_knn_request, "list_force": capi.nb_list_force_request, "split_force": capi.nb_split_force_request}


def valid_request(q, keep):
    """A host-pointer request of query q that an f32 handle of MSG_N bodies accepts; `keep` holds the arrays it points to."""
    m = MSG_M

    def ptr(shape, dtype=np.float32, fill=0):
        keep.append(np.full(shape, fill, dtype))
        return keep[-1].ctypes.data_as(C.c_void_p)

    def uptr(shape):
        return ptr(shape, np.uint32)

    r = REQUEST[q]()
    r.struct_size, r.m, r.points = C.sizeof(r), m, ptr((m, 4))
    if q == "field_eval":
        r.accel, r.phi = ptr((m, 4)), ptr(m)
    elif q == "neighbors":
        r.radius, r.index, r.dist2, r.count = 0.5, uptr(m), ptr(m), uptr(m)
    elif q == "neighbor_lists":
        r.radius, r.cap, r.list, r.count = 0.5, 4, uptr((m, 4)), uptr(m)
    elif q == "knn":
        r.k, r.index, r.dist2 = 2, uptr((m, 2)), ptr((m, 2))
    elif q == "list_force":
        r.cap, r.list, r.accel = 4, uptr((m, 4)), ptr((m, 4))
    else:
        r.radius, r.accel_irr, r.accel_reg = 0.5, ptr((m, 4)), ptr((m, 4))
    return r


def _at_bodies(r, first=0):
    r.flags |= 1
    r.points = None
    r.first_body = first


def _set(**kw):
    def f(r, keep):
        for k, v in kw.items():
            setattr(r, k, v)
    return f


def _with_vel(*outputs):
    """Asks for the jerk outputs named, with the point velocities they need."""
    def f(r, keep):
        for k in outputs + ("point_vel",):
            keep.append(np.zeros((MSG_M, 4), np.float32))
            setattr(r, k, keep[-1].ctypes.data_as(C.c_void_p))
    return f


def _vel_at_bodies(r, keep):
    _at_bodies(r)
    _with_vel()(r, keep)


def _vel_without_jerk(r, keep):
    _with_vel()(r, keep)


# the faults every request can have: {name: what it does to a valid request}
HEAD_FAULTS = {
    "struct_size": lambda r, keep: setattr(r, "struct_size", r.struct_size - 4),
    "flags": lambda r, keep: setattr(r, "flags", r.flags | 8),
    "points_with_at_bodies": lambda r, keep: setattr(r, "flags", r.flags | 1),
    "no_points": _set(points=None),
    "m_0": _set(m=0),
    "past_n": lambda r, keep: (_at_bodies(r, MSG_N - MSG_M + 1)),
}
# and those of the fields only one query has
OWN_FAULTS = {
    "field_eval": {"no_output": _set(accel=None, phi=None)},
    "neighbors": {"no_output": _set(index=None, dist2=None, count=None), "radius_negative": _set(radius=-1.0),
                  "count_without_radius": _set(radius=0.0)},
    "neighbor_lists": {"no_list": _set(list=None), "cap_0": _set(cap=0), "cap_4097": _set(cap=4097), "reserved": _set(reserved=1),
                       "radius_negative": _set(radius=-1.0), "no_radius": _set(radius=0.0)},
    "knn": {"k_0": _set(k=0), "k_65": _set(k=65), "reserved": _set(reserved=1), "no_output": _set(index=None, dist2=None)},
    "list_force": {"no_list": _set(list=None), "cap_0": _set(cap=0), "cap_4097": _set(cap=4097), "reserved": _set(reserved=1),
                   "no_output": _set(accel=None), "vel_at_bodies": _vel_at_bodies, "vel_without_jerk": _vel_without_jerk},
    "split_force": {"no_output": _set(accel_irr=None, accel_reg=None), "vel_at_bodies": _vel_at_bodies, "vel_without_jerk": _vel_without_jerk,
                    "radius_negative": _set(radius=-1.0), "no_radius": _set(radius=0.0)},
}
# a jerk without the point velocities: on the Hermite handle (a leapfrog handle has no jerk to give: its own case below)
JERK = {"list_force": ("jerk",), "split_force": ("jerk_irr", "jerk_reg")}
NEEDS_G = ("field_eval", "list_force", "split_force")


def _jerk_without_vel(q):
    def f(r, keep):
        _with_vel(*JERK[q])(r, keep)
        r.point_vel = None
    return f


def message_cases():
    """[(id, handle, function, query | None, fault)]: handle names one of message_handles(); fault(request, keep) or, for a getter,
    its arguments after the handle."""
    cases = []
    for q in QUERIES:
        fn = "nb_" + q
        cases.append((fn + ":null_handle", "none", fn, q, None))
        cases.append((fn + ":null_request", "ready", fn, None, None))
        for name, fault in list(HEAD_FAULTS.items()) + list(OWN_FAULTS[q].items()):
            cases.append(("%s:%s" % (fn, name), "ready", fn, q, fault))
        cases.append((fn + ":nothing_uploaded", "created", fn, q, None))
        if q in NEEDS_G:
            cases.append((fn + ":no_params", "uploaded", fn, q, None))
        if q in JERK:
            cases.append((fn + ":jerk_without_vel", "hermite", fn, q, _jerk_without_vel(q)))
            cases.append((fn + ":jerk_on_leapfrog", "ready", fn, q, _with_vel(*JERK[q])))
        mf = "nb_multi_" + q
        cases.append((mf + ":null_handle", "none", mf, q, None))
        cases.append((mf + ":null_request", "multi", mf, None, None))
        cases.append((mf + ":m_0", "multi", mf, q, HEAD_FAULTS["m_0"]))           # the shard's text, under the wrapper's name
        cases.append((mf + ":past_n", "multi", mf, q, HEAD_FAULTS["past_n"]))     # against the caller's n, not the padded one
        if q in JERK:
            cases.append((mf + ":jerk", "multi", mf, q, _with_vel(*JERK[q])))
    for g in GETTERS:
        fn = "nb_%s_shape" % g
        extra = {"neighbors": (), "split_force": (), "knn": (2,)}.get(g, (4,))
        cases.append((fn + ":null_handle", "none", fn, None, (1,) + extra))
        cases.append((fn + ":m_0", "ready", fn, None, (0,) + extra))
        for bad in {"knn": (0, 65)}.get(g, (0, 4097) if extra else ()):
            cases.append(("%s:%d" % (fn, bad), "ready", fn, None, (1, bad)))
    return cases


class message_handles:
    """The handles the cases name: `created` (nothing uploaded), `uploaded` (no nb_set_params), `ready`, `hermite` and `multi` (ready)."""

    def __enter__(self):
        b, v = ic.plummer(MSG_N, seed=5)
        self.sims = {"created": Simulation(MSG_N), "uploaded": Simulation(MSG_N).init(b, v), "ready": Simulation(MSG_N).init(b, v),
                     "hermite": Simulation(MSG_N, integrator="hermite4").init(b, v), "multi": MultiSimulation(MSG_N, 2)}
        self.sims["multi"].init(b, v)
        for k in ("ready", "hermite", "multi"):
            self.sims[k].set_params(1e-2, 1.0)
        return self

    def __exit__(self, *a):
        for s in self.sims.values():
            s.close()

    def handle(self, name):
        return None if name == "none" else self.sims[name]._h


def message_of(handles, case):
    """(return code, text) of one case."""
    _, hname, fn, q, fault = case
    L = capi.load_library()
    h = handles.handle(hname)
    if fn.endswith("_shape"):
        outs = len(getattr(L, fn).argtypes) - 1 - len(fault)
        rc = getattr(L, fn)(h, *fault, *[None] * outs)
    elif q is None:
        rc = getattr(L, fn)(h, None)
    else:
        keep = []
        r = valid_request(q, keep)
        if fault:
            fault(r, keep)
        rc = getattr(L, fn)(h, C.byref(r))
    last = L.nb_multi_last_error if fn.startswith("nb_multi_") else L.nb_last_error
    return int(rc), last(h).decode()


def all_messages():
    with message_handles() as handles:
        return {case[0]: list(message_of(handles, case)) for case in message_cases()}


# ---- bits ----------------------------------------------------------------------------------------------------------------------------

BITS_N, BITS_SEED, BITS_DT, BITS_G = 771, 21, 1e-2, 1.0
BITS_HANDLES = (("f32", False), ("f64", False), ("f32", True))


def sha(a):
    a = np.ascontiguousarray(a)
    return "%s%s:%s" % (a.dtype.str, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest())


def bits_of(precision, hermite):
    """{output: digest} of a fresh handle's answers."""
    import query_state as Q
    req = Q.requests(BITS_N, np.float64 if precision == "f64" else np.float32, BITS_SEED, hermite)
    with make(BITS_N, precision, hermite) as sim:
        sim.init(req["bodies"], req["vel"])
        sim.set_params(BITS_DT, BITS_G)
        got = Q.answers(sim, req)
        for name, out in (("split_pts", sim.split_force(req["points"], point_vel=req["point_vel"] if hermite else None, radii=req["radii"])),
                          ("split_bod", sim.split_force(bodies=req["range"], radius=req["radius"]))):
            for k, a in out.items():
                got[name + "." + k] = a
    return {k: sha(a) for k, a in sorted(got.items())}


def all_bits():
    return {handle_id(BITS_N, p, h): bits_of(p, h) for p, h in BITS_HANDLES}


def load():
    with open(JSON_PATH) as f:
        return json.load(f)
