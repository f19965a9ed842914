"""One request set and one comparison for "what do the queries answer on a handle that has stepped" (tests/test_query_state_gpu.py,
tests/test_query_state_cpu.py and the queries of tests/api_sequence.py).

The header promises that nb_field_eval, nb_neighbors, nb_neighbor_lists, nb_knn, nb_list_force, nb_diagnostics and the frame feed read
"the positions as they stand behind every step enqueued so far", on every handle kind.  The check: run every query on the stepped
handle, THEN download its state, load that state into a fresh handle that never steps (the twin) and ask the twin the same.

  * neighbours, lists, k nearest, list forces: bit for bit (their answers depend on the point, the row's entries and the bodies only);
  * the frame's bodies: the downloaded bodies rounded to binary32, bit for bit;
  * field and diagnostics: within the bounds of tests/test_field_gpu.py (2e-5 f32, 1e-12 f64 and NB_FIELD_F64) of a host fp64 sum over
    the DOWNLOADED state, and -- `same_shape`: two whole-system handles of one n and precision, whose launch shapes are then the same
    (field_shape and diag_chunk of nb_engine.hip depend on n, the precision and the device only) -- bit for bit with the twin.

`stale_must_fail` is the control: the same answers against a state one step older must fail every one of those checks."""
import numpy as np

from nbody3d_amd import ic
from test_field_gpu import EPS2, TOL32, TOL64, points_for, ref_field

NONE = 0xffffffff
POINTS = 256
RADIUS = 0.3
CAP = 16
K = 7
LF_ROWS, LF_CAP = 300, 24
MIN_ROWS = 10            # rows of every group of integer outputs (INT_GROUPS) that one step must change (stale_must_fail)


def requests(n, dtype, seed, hermite):
    """The fixed request set of an n-body Plummer sphere (ic.plummer(n, seed), N-body units); req["bodies"] / req["vel"] are the system."""
    dtype = np.dtype(dtype).type
    b, v = ic.plummer(n, seed=seed)
    rng = np.random.default_rng(seed + 77)
    pts = points_for(b, POINTS, seed)                     # half near bodies, half in the bounding box
    pts[::10] = b[rng.integers(0, n, len(pts[::10])), :3]  # every 10th: exactly on a body
    first = n // 3
    lists = rng.integers(0, n, (LF_ROWS, LF_CAP)).astype(np.uint32)
    lists[rng.random(lists.shape) < 0.1] = NONE           # padding wherever it stands
    for k, bad in enumerate((n, n + 1, n + 1000, 1 << 31, NONE - 1)):      # past the rows: adds nothing
        lists[(37 * k + 5) % LF_ROWS, (5 * k + 1) % LF_CAP] = bad
    pvel = np.zeros((POINTS, 4), dtype)
    pvel[:, :3] = rng.normal(0.0, 0.5, (POINTS, 3))
    req = {"n": n, "dtype": dtype, "seed": seed, "hermite": bool(hermite), "bodies": b.astype(dtype), "vel": v.astype(dtype),
           "points": np.ascontiguousarray(np.concatenate([pts, np.zeros((POINTS, 1), np.float32)], axis=1).astype(dtype)),
           "radii": rng.uniform(0.15, 0.45, POINTS).astype(dtype), "radius": RADIUS, "range": (first, min(300, n - first)),
           "cap": CAP, "k": K, "lists": lists, "count": rng.integers(0, LF_CAP + 8, LF_ROWS).astype(np.uint32), "point_vel": pvel}
    for a in req.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return req


def whole_system(sim):
    """A Simulation that holds every row itself (not a shard handle, not a multi handle): the kinds with a frame feed."""
    return hasattr(sim, "request_frame") and getattr(sim, "shard_count", None) == sim.n


def answers(sim, req):
    """Every query through the Python wrapper: {name: ndarray}.  Nothing but queries is called (no sync, no read)."""
    multi = not hasattr(sim, "request_frame")
    jerk = req["hermite"] and not multi
    pts, rng = req["points"], req["range"]
    out = {}

    def put(name, keys, vals):
        for k, x in zip(keys, vals):
            if x is not None:
                out[name + "." + k] = np.array(x)

    put("nbr_pts", ("index", "dist2", "count"), sim.neighbors(pts, radii=req["radii"]))
    put("nbr_bod", ("index", "dist2", "count"), sim.neighbors(bodies=rng, radius=req["radius"]))
    put("nbl_bod", ("list", "count", "index", "dist2"), sim.neighbor_lists(bodies=rng, radius=req["radius"], cap=req["cap"], nearest=True))
    put("nbl_pts", ("list", "count", "index", "dist2"), sim.neighbor_lists(pts, radii=req["radii"], cap=req["cap"], nearest=True))
    put("knn_pts", ("index", "dist2"), sim.knn(pts, k=req["k"]))
    put("knn_bod", ("index", "dist2"), sim.knn(bodies=rng, k=req["k"]))
    m = len(pts)
    put("lf_pts", ("accel", "jerk", "phi"), sim.list_force(req["lists"][:m], points=pts, point_vel=req["point_vel"] if jerk else None,
                                                        count=req["count"][:m], jerk=jerk, phi=True))
    put("lf_bod", ("accel", "jerk", "phi"), sim.list_force(req["lists"][:rng[1]], bodies=rng, count=req["count"][:rng[1]], jerk=jerk, phi=True))
    put("field_pts", ("accel", "phi"), sim.field(pts))
    put("field_bod", ("accel", "phi"), sim.field(bodies=rng))
    if sim.dtype == np.float32:
        put("field64_pts", ("accel", "phi"), sim.field(pts, f64=True))
    ke, pe, mom = sim.diagnostics()
    out["diag"] = np.array([ke, pe, mom[0], mom[1], mom[2]], np.float64)
    if whole_system(sim):
        sim.request_frame()
        fb, _, step = sim.frame()
        out["frame.bodies"] = np.array(fb)
        out["frame.step"] = np.array([step], np.uint64)
    return out


def make_twin(n, precision, hermite=False):
    """The handle that never steps: the plainest kernel, or a fresh Hermite handle for the Hermite kinds."""
    from nbody3d_amd import Simulation
    return Simulation(n, precision=precision, integrator="hermite4") if hermite else Simulation(n, precision=precision, force_variant=1, jsplit=1)


def load_twin(twin, state, dt, G):
    twin.init(*state)
    twin.set_params(dt, G)
    return twin


# ---- the comparison ------------------------------------------------------------------------------------------------------------------

# The integer outputs, in the groups the control counts changed rows over.  A query's nearest index is taken over its point rows and its
# body rows together: the points stand still, half of them in the thin outskirts of the bounding box, so one step changes the
# nearest body of only a handful of them (3 to 6 of 256 in tests/test_query_state_cpu.py); every other output is held on its own.
INT_GROUPS = {"nearest index (neighbors)": ("nbr_pts.index", "nbr_bod.index"), "nearest index (neighbor_lists)": ("nbl_pts.index", "nbl_bod.index"),
              "count (neighbors, points)": ("nbr_pts.count",), "count (neighbors, bodies)": ("nbr_bod.count",),
              "count (neighbor_lists, points)": ("nbl_pts.count",), "count (neighbor_lists, bodies)": ("nbl_bod.count",),
              "list rows (points)": ("nbl_pts.list",), "list rows (bodies)": ("nbl_bod.list",),
              "knn rows (points)": ("knn_pts.index",), "knn rows (bodies)": ("knn_bod.index",)}
TOLERANCE = ("field_pts", "field_bod", "field64_pts")       # (+ "diag"): held to the fp64 sum; to the twin's bits only with same_shape


def is_exact(name):
    return name.split(".")[0] in ("nbr_pts", "nbr_bod", "nbl_pts", "nbl_bod", "knn_pts", "knn_bod", "lf_pts", "lf_bod")


def changed_rows(x, y):
    """The rows in which two arrays differ in bits."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.shape == y.shape and x.dtype == y.dtype, (x.shape, y.shape, x.dtype, y.dtype)
    if x.size == 0:
        return np.zeros(0, np.int64)
    rows = x.shape[0] if x.ndim else 1
    u = x.reshape(rows, -1).view(np.uint8).reshape(rows, -1) != y.reshape(rows, -1).view(np.uint8).reshape(rows, -1)
    return np.nonzero(u.any(1))[0]


def ref_energy(state, G, eps2=EPS2, shard=None):
    """What nb_diagnostics promises, in fp64 on the host: the kinetic energy and momentum of the handle's rows and its share of the
    potential energy (every pair i < j whose lower index is one of its rows); plus sum m |v|, the scale of the momentum."""
    b, v = np.asarray(state[0], np.float64), np.asarray(state[1], np.float64)
    n = len(b)
    sb, sc = (0, n) if shard is None else shard
    x, m = b[:, :3], b[:, 3]
    pe = 0.0
    j = np.arange(n)
    for i0 in range(sb, sb + sc, 512):
        i = np.arange(i0, min(i0 + 512, sb + sc))
        d = x[None, :, :] - x[i, None, :]
        y = 1.0 / np.sqrt((d * d).sum(2) + eps2)
        pe -= G * float((m[i, None] * m[None, :] * y * (j[None, :] > i[:, None])).sum())
    rows = slice(sb, sb + sc)
    mv = m[rows, None] * v[rows, :3]
    ke = 0.5 * float((m[rows] * (v[rows, :3] ** 2).sum(1)).sum())
    return np.array([ke, pe, mv[:, 0].sum(), mv[:, 1].sum(), mv[:, 2].sum()]), float(np.sqrt((mv * mv).sum(1)).sum())


def tolerance_errors(got, state, req, precision, G=1.0, eps2=EPS2, shard=None):
    """{output: (error, bound)} of field and diagnostics against the host fp64 sums over `state` (the metric of test_field_gpu.py)."""
    b = state[0]
    first, count = req["range"]
    rows = np.arange(first, first + count)
    refs = {"field_pts": ref_field(b, req["points"], G=G, eps2=eps2), "field_bod": ref_field(b, np.asarray(b)[rows], G=G, eps2=eps2, skip=rows)}
    refs["field64_pts"] = refs["field_pts"]
    out = {}
    for q, (ra, rf) in refs.items():
        if q + ".accel" not in got:
            continue
        tol = TOL64 if (precision == "f64" or q == "field64_pts") else TOL32
        a, f = got[q + ".accel"], got[q + ".phi"]
        out[q + ".accel"] = (float((np.abs(a[:, :3].astype(np.float64) - ra).max(1) / np.abs(ra).max(1)).max()), tol)
        out[q + ".phi"] = (float((np.abs(f.astype(np.float64) - rf) / np.abs(rf)).max()), tol)
        assert np.all(a[:, 3] == 0), q + ".accel: a w lane is not 0"
    tol = TOL64 if precision == "f64" else TOL32
    want, pscale = ref_energy(state, G, eps2, shard)
    d = got["diag"]
    out["diag.ke"] = (abs(d[0] - want[0]) / abs(want[0]), tol)
    out["diag.pe"] = (abs(d[1] - want[1]) / abs(want[1]), tol)
    out["diag.momentum"] = (float(np.abs(d[2:] - want[2:]).max()) / pscale, tol)
    return out


def failures(got, want, state, req, precision, same_shape, G=1.0, eps2=EPS2, shard=None, steps=None):
    """Every check of the module docstring that `got` misses, as {output: message}, and the tolerance figures found."""
    bad = {}
    extra = set(got) ^ set(want)           # a multi or shard handle has no frame feed; its twin, a whole-system handle, has
    assert extra <= (set(want) - set(got)) & {"frame.bodies", "frame.step"}, "the two handles answered different sets of outputs: %s" % sorted(extra)
    for name in sorted(got):
        exact = is_exact(name) or (same_shape and (name == "diag" or name.split(".")[0] in TOLERANCE))
        if exact:
            r = changed_rows(got[name], want[name])
            if len(r):
                k = int(r[0])
                bad[name] = "%d of %d rows differ from the twin's in bits, first rows %s: row %d is %s, the twin's %s" % (
                    len(r), len(np.atleast_1d(got[name])), r[:5].tolist(), k, np.atleast_1d(got[name])[k], np.atleast_1d(want[name])[k])
    if "frame.bodies" in got:
        r = changed_rows(got["frame.bodies"], np.asarray(state[0]).astype(np.float32))
        if len(r):
            bad["frame.bodies"] = "%d rows differ from the downloaded bodies, first rows %s" % (len(r), r[:5].tolist())
        if steps is not None and int(got["frame.step"][0]) != steps:
            bad["frame.step"] = "the frame carries step index %d after %d steps" % (int(got["frame.step"][0]), steps)
    figures = tolerance_errors(got, state, req, precision, G, eps2, shard)
    for name, (err, tol) in figures.items():
        if not err <= tol:
            bad[name + " (fp64)"] = "%.3g off the host fp64 sum over the downloaded state (bound %.0e)" % (err, tol)
    return bad, figures


def compare(got, want, state, req, precision, same_shape, G=1.0, eps2=EPS2, shard=None, steps=None, where=""):
    """Asserts every check; `where` names the handle kind and the checkpoint.  Returns the tolerance figures {output: (error, bound)}."""
    bad, figures = failures(got, want, state, req, precision, same_shape, G, eps2, shard, steps)
    print("%s: %s" % (where, ", ".join("%s %.2e" % (k, e) for k, (e, _) in sorted(figures.items()))))
    assert not bad, "%s:\n  %s" % (where, "\n  ".join("%s: %s" % kv for kv in sorted(bad.items())))
    return figures


def stale_must_fail(got, stale, stale_state, req, precision, G=1.0, eps2=EPS2, shard=None, where=""):
    """The control: `stale` are a twin's answers on the state one step before the one `got` was asked on.  Every category of compare()
    must fail on it: every float output differs in bits, field misses its fp64 bound over the stale state, every integer output
    differs in at least MIN_ROWS rows.  Returns {group: changed rows} of the integer outputs (INT_GROUPS)."""
    bad, figures = failures(got, stale, stale_state, req, precision, True, G, eps2, shard)
    missed, rows = [], {}
    for name in sorted(got):
        if name == "frame.step":
            continue
        if name not in bad:          # (same_shape above: every output was held to bits, the frame to the older bodies)
            missed.append("%s equals the answer on the older state in bits" % name)
    for name, (err, tol) in figures.items():
        if name.startswith("field") and err <= tol:
            missed.append("%s is within %.0e of the fp64 sum over the older state (%.3g)" % (name, tol, err))
    for kind, names in INT_GROUPS.items():
        rows[kind] = sum(len(changed_rows(got[name], stale[name])) for name in names)
        if rows[kind] < MIN_ROWS:
            missed.append("%s: only %d rows differ from the answer on the older state" % (kind, rows[kind]))
    print("%s: one step changes %s" % (where, ", ".join("%s %d" % kv for kv in sorted(rows.items()))))
    assert not missed, "%s: the comparison would not notice a state one step old:\n  %s" % (where, "\n  ".join(missed))
    return rows
