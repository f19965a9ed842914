"""What nb_step did on Hermite handles BEFORE orders 4 and 6 were given one host path (one pass launcher, one predictor/corrector
launcher, one hermite_step, one block_step) -- as data: tests/golden/measure_hermite_parent.py records it from a build of that
commit through the public Python API, tests/test_hermite_parent_gpu.py holds every later build to it.  Two parts:

  * bits: per case a list of segments, each {arrays: SHA-256 of every downloaded array (bodies, vel, accel, jerk; snap and crackle
    at order 6; levels with block steps), stats: block_stats(), variant, shape: shape_info()}.  The launch rule of the full and of
    the gathered pass depends on the device's compute-unit count, which is recorded with them;
  * messages: the return code and the full nb_last_error text of nb_step without nb_set_params on the four step paths.

The cases (seeded ic.plummer, G = 1 unless stated):
  plain    orders 4 and 6 x f32 and f64, three steps, at N = 771 (one j-chunk, ragged last tile, one partly filled workgroup) and
           N = 4099 (two j-chunks of 2,304 and 1,795 bodies);
  restart  N = 771 f64: two steps | set_params with G = 0.5, one step (the start and the snap start run again) |
           set_hermite_order(6), one step | set_hermite_order(4), one step;
  block    N = 771 and 4099, max_level = 6, simulate(2) (the schedule-ahead between outer steps): order 4 dynamic f32 and f64,
           order 6 dynamic f64, order 6 frozen f32 with uploaded levels spread over four levels.  At these sizes the f32 launches
           always halve the rows (NG = 1).  One of them again as two calls of simulate(1);
  ng2      f32, N = 24,577, orders 4 and 6, frozen with min_level = max_level = 1, one outer step: every block step has all bodies
           active, ceil(24577/1024) * ceil(24577/256) = 2,425 >= 8 x 256, the smallest shape at which the 1,024-row gathered
           kernels are launched on 256 compute units."""
import hashlib
import json
import os

import numpy as np

from nbody3d_amd import Simulation, capi, ic

JSON_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hermite_parent.json")

SEED = 21
DT_PLAIN, DT_BLOCK = 2.0 ** -7, 2.0 ** -4
SIZES = (771, 4099)
NG2_N = 24577
MAX_LEVEL = 6

PLAIN = [("plain", order, prec, n) for n in SIZES for order in (4, 6) for prec in ("f32", "f64")]
RESTART = [("restart", 4, "f64", 771)]
# (kind, order, precision, n, frozen, calls of simulate)
BLOCK = [("block", order, prec, n, frozen, (2,)) for n in SIZES
         for order, prec, frozen in ((4, "f32", False), (4, "f64", False), (6, "f64", False), (6, "f32", True))]
SPLIT_OF = ("block", 6, "f64", 771, False, (2,))
SPLIT = ("block", 6, "f64", 771, False, (1, 1))
NG2 = [("ng2", order, "f32", NG2_N) for order in (4, 6)]
CASES = PLAIN + RESTART + BLOCK + [SPLIT] + NG2


def case_id(case):
    kind, order, prec, n = case[:4]
    tail = ""
    if kind == "block":
        tail = ("_frozen" if case[4] else "_dynamic") + "_" + "+".join(str(k) for k in case[5])
    return "%s_o%d_%s_%d%s" % (kind, order, prec, n, tail)


def compute_units():
    import torch
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def sha(a):
    a = np.ascontiguousarray(a)
    return "%s%s:%s" % (a.dtype.str, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest())


def segment(sim, order, block):
    """What one segment of a case records."""
    b, v, a = sim.read()
    arrays = {"bodies": b, "vel": v, "accel": a, "jerk": sim.read_jerk()}
    if order == 6:
        arrays["snap"], arrays["crackle"] = sim.read_snap()
    if block:
        arrays["levels"] = sim.read_levels()
    return {"arrays": {k: sha(x) for k, x in sorted(arrays.items())}, "stats": sim.block_stats(), "variant": sim.variant,
            "shape": sim.shape_info()}


def spread_levels(n):
    """Levels 0..3, scattered over the rows (a multiplicative hash of the row number: no generator whose stream could change)."""
    return ((np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)) >> 30).astype(np.uint8)


def set_block(sim, order, **kw):
    (sim.set_block_steps6 if order == 6 else sim.set_block_steps)(**kw)


def run(case):
    """[segment, ...] of one case."""
    kind, order, prec, n = case[:4]
    b0, v0 = ic.plummer(n, seed=SEED)
    out = []
    with Simulation(n, precision=prec, integrator="hermite4") as sim:
        if order == 6:
            sim.set_hermite_order(6)
        sim.init(b0, v0)
        if kind == "plain":
            sim.set_params(DT_PLAIN, 1.0)
            sim.simulate(3)
            out.append(segment(sim, order, False))
        elif kind == "restart":
            sim.set_params(DT_PLAIN, 1.0)
            sim.simulate(2)
            out.append(segment(sim, 4, False))
            sim.set_params(DT_PLAIN, 0.5)
            sim.simulate(1)
            out.append(segment(sim, 4, False))
            sim.set_hermite_order(6)
            sim.simulate(1)
            out.append(segment(sim, 6, False))
            sim.set_hermite_order(4)
            sim.simulate(1)
            out.append(segment(sim, 4, False))
        elif kind == "block":
            frozen, calls = case[4], case[5]
            sim.set_params(DT_BLOCK, 1.0)
            set_block(sim, order, max_level=MAX_LEVEL, frozen=frozen)
            if frozen:
                sim.upload_levels(spread_levels(n))
            for k in calls:
                sim.simulate(k)
            out.append(segment(sim, order, True))
        else:
            sim.set_params(DT_BLOCK, 1.0)
            set_block(sim, order, max_level=1, min_level=1, frozen=True)
            sim.simulate(1)
            out.append(segment(sim, order, True))
    return out


def all_bits():
    return {case_id(c): run(c) for c in CASES}


# ---- messages ------------------------------------------------------------------------------------------------------------------------
MSG_N = 64
MSG_PATHS = [(block, order) for block in (False, True) for order in (4, 6)]


def message_id(block, order):
    return "nb_step:no_params:%s_o%d" % ("block" if block else "plain", order)


def message_of(block, order):
    """(return code, text) of nb_step on an uploaded handle whose nb_set_params has not been called."""
    b0, v0 = ic.plummer(MSG_N, seed=5)
    L = capi.load_library()
    with Simulation(MSG_N, precision="f64", integrator="hermite4") as sim:
        if order == 6:
            sim.set_hermite_order(6)
        sim.init(b0, v0)
        if block:
            set_block(sim, order, max_level=2)
        rc = L.nb_step(sim._h, 1)
        return int(rc), L.nb_last_error(sim._h).decode()


def all_messages():
    return {message_id(b, o): list(message_of(b, o)) for b, o in MSG_PATHS}


def load():
    with open(JSON_PATH) as f:
        return json.load(f)
