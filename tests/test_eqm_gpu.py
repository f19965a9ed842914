"""The equal-mass kernels of the symmetric force pass (nb_force_symw_eqm, nb_force_symw_pairs_eqm) against the general ones.

On a system whose bodies all have the same mass the two G*m products of a pair are one product, and the rotating mass lane carries a
constant: the equal-mass kernels take one product and rotate no mass.  Every per-pair product and every addition is the general
kernel's, so the yardstick is BYTES: a handle that runs them (Simulation.eqm) and a handle with NB_FLAG_NO_EQM leave the same bodies,
velocities and accelerations.  The shapes are the smallest at which each loop form runs on a plan without padding rows:
  N =  8,192, force_variant 716013 / 708013 (16 / 8 residents per lane): wave ranges cut inside sweeps -- the single forms;
  N = 12,288 and 20,480 with NB_FLAG_WHOLE_SWEEPS: the paired loop (checked on the plan, walked as the kernel walks it);
  N = 65,536: the default plan;  N = 262,144: the headline (the queue of pieces is on).
A handle is NOT eligible -- Simulation.eqm is false, bytes still those of NB_FLAG_NO_EQM -- with unequal masses (one ulp is enough),
padding rows (a ragged N), a nonzero vel.w or accel.w (leapfrog would move the mass lane); whatever writes the state from outside the
step (a new upload, a device pointer handed out) makes the engine look again before the next step.
"""
import ctypes as C

import numpy as np
import pytest

from nbody3d_amd import Simulation, capi, ic

pytestmark = pytest.mark.gpu

WHOLE, NO_EQM = capi.NB_FLAG_WHOLE_SWEEPS, capi.NB_FLAG_NO_EQM
# (n, force_variant, flags, some sweeps must pair)
SHAPES = [(8192, 716013, 0, False), (8192, 708013, 0, False),
          (12288, 716013, WHOLE, True), (12288, 708013, WHOLE, True),
          (20480, 716013, WHOLE, True), (20480, 708013, WHOLE, True),
          (65536, 0, 0, True)]
SMALL = (12288, 716013, WHOLE)        # the shape of the eligibility and invalidation cases: paired and single loops both run

_systems = {}


def plummer(n):
    """ic.plummer(n) once per size; the tests copy what they change."""
    if n not in _systems:
        _systems[n] = ic.plummer(n, seed=5)
    return _systems[n]


def paired_sweeps(n, variant, flags):
    """How many chunk-sweeps of the plan run two at a time (kernels/symmetric.hip.h `pair`; tools/paired_share.py), and the plan."""
    q = capi.plan_query(n, force_variant=variant, flags=flags, n_cu=0, clock_hz=0)
    assert q["symw"] and q["x"] == 3, q["variant"]
    pl, ups, cps = q["plan"], q["ups"], q["ipl"]
    nsb, th, tl, n_hi, zc = pl["nsb"], pl["total_hi"], pl["total_lo"], pl["n_hi"], pl["zc"]
    first_lo = n_hi * th
    first_z = first_lo + (nsb - n_hi) * tl
    ranges = [(int(a), int(b)) for a, b, _, _ in q["waves"]] + [(int(u), int(u) + (int(l) >> 16)) for u, l in q.get("pieces", [])]
    paired = 0
    for u, uend in ranges:
        while u < uend:
            p = u // ups
            if p < first_lo:
                g = p // th; k = p - g * th; total = th
            elif p < first_z:
                r = p - first_lo; g = n_hi + r // tl; k = r - (g - n_hi) * tl; total = tl
            else:
                g = nsb; k = p - first_z; total = zc
            both_end = total - cps if g < nsb else 0
            ug_end = min((p - k + total) * ups, uend)
            while u < ug_end:
                q0 = u % ups
                if q0 == 0 and ug_end - u >= 2 * ups and k + 1 < both_end:
                    paired += 2; u += 2 * ups; k += 2
                    continue
                u += min(ups - q0, ug_end - u)
                if u % ups == 0:
                    k += 1
    return paired, q


def state(sim):
    return tuple(x.tobytes() for x in sim.read())


def run(n, variant, flags, b, v, a=None, G=1.0, steps=(1, 20)):
    """[(eqm, state) after each entry of `steps`]: 1 step is a plain launch, 20 go through the captured graph."""
    out = []
    with Simulation(n, force_variant=variant, flags=flags) as sim:
        sim.init(b, v, a)
        sim.set_params(1e-3, G)
        for k in steps:
            eqm = sim.eqm
            sim.simulate(k)
            out.append((eqm, state(sim)))
        out.append((sim.eqm, sim.variant))
    return out


def both_arms(n, variant, flags, b, v, a=None, G=1.0, steps=(1, 20), eligible=True):
    got = run(n, variant, flags, b, v, a, G, steps)
    want = run(n, variant, flags | NO_EQM, b, v, a, G, steps)
    assert got[-1][1] == want[-1][1]                        # the same plan, the same variant string
    assert all(e is eligible for e, _ in got), (n, variant, [e for e, _ in got])
    assert not any(e for e, _ in want)
    for k, (g, w) in enumerate(zip(got[:-1], want[:-1])):
        for name, x, y in zip(("bodies", "vel", "accel"), g[1], w[1]):
            assert x == y, (n, variant, flags, "after %d steps" % sum(steps[:k + 1]), name)


@pytest.mark.parametrize("n,variant,flags,pairs", SHAPES)
def test_equal_mass_plummer_is_byte_identical_to_the_general_kernels(n, variant, flags, pairs):
    paired, q = paired_sweeps(n, variant, flags)
    assert q["plan"]["np"] == n and q["plan"]["zc"] == 0            # no padding rows
    assert (paired > 0) == pairs, (n, variant, flags, paired)
    b, v = plummer(n)
    assert np.unique(np.ascontiguousarray(b[:, 3]).view(np.uint32)).size == 1
    both_arms(n, variant, flags, b, v)


@pytest.mark.parametrize("n,variant,flags,pairs", SHAPES)
def test_equal_mass_with_g_folded_into_the_j_stream(n, variant, flags, pairs):
    b, v = plummer(n)
    both_arms(n, variant, flags, b, v, G=0.37)


def one_ulp(b):
    b = b.copy()
    b[len(b) // 3, 3] = np.nextafter(b[len(b) // 3, 3], np.float32(1))
    return b


def test_unequal_masses_keep_the_general_kernels():
    n, variant, flags = SMALL
    b, v = ic.uniform_cube(n)
    both_arms(n, variant, flags, b, v, eligible=False)
    b, v = plummer(n)
    both_arms(n, variant, flags, one_ulp(b), v, eligible=False)


def test_a_plan_with_padding_rows_keeps_the_general_kernels():
    n = 12289
    b, v = plummer(n)
    both_arms(n, SMALL[1], SMALL[2], b, v, eligible=False)


def test_nonzero_w_lanes_keep_the_general_kernels():
    n, variant, flags = SMALL
    b, v = plummer(n)
    v1 = v.copy()
    v1[7, 3] = 1e-3
    both_arms(n, variant, flags, b, v1, eligible=False)
    a = np.zeros_like(b)
    both_arms(n, variant, flags, b, v, a)                 # an uploaded all-zero accel: still eligible
    a[n - 1, 3] = 0.5
    both_arms(n, variant, flags, b, v, a, eligible=False)


def hip_runtime():
    """The HIP runtime the process already has (conftest loads torch's copy first; a second copy would see no device)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            L = C.CDLL(line.split()[-1])
            L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            return L
    raise RuntimeError("no HIP runtime loaded")


def poke(sim, which, row, value):
    """Writes one w lane through the device pointer the engine hands out."""
    sim.sync()
    p = sim.device_ptr(which)
    x = np.array([value], np.float32)
    assert hip_runtime().hipMemcpy(p + 16 * row + 12, x.ctypes.data, 4, 1) == 0


def sequence(flags, change):
    """Step once on the equal-mass system, change it from outside the step, step again (1, then 20: the graph)."""
    n, variant, fl = SMALL
    b, v = plummer(n)
    with Simulation(n, force_variant=variant, flags=fl | flags) as sim:
        sim.init(b, v)
        sim.set_params(1e-3, 1.0)
        first = sim.eqm
        sim.simulate(1)
        change(sim)
        after = sim.eqm
        sim.simulate(1)
        s1 = state(sim)
        sim.simulate(20)
        return first, after, sim.eqm, s1, state(sim)


def reupload_one_mass(sim):
    b, v, a = sim.read()
    sim.restore(one_ulp(b), v, a)


CHANGES = {
    "upload": (reupload_one_mass, False),
    "bodies_ptr": (lambda sim: poke(sim, "bodies", 100, 3e-4), False),
    "vel_ptr": (lambda sim: poke(sim, "vel", 5, 0.25), False),
    "accel_ptr": (lambda sim: poke(sim, "accel", 12287, -1.0), False),
    # handed out but not written: the engine looks again and finds the system still eligible
    "bodies_ptr_untouched": (lambda sim: sim.device_ptr("bodies"), True),
    "same_upload": (lambda sim: sim.restore(*sim.read()), True),
}


@pytest.mark.parametrize("how", sorted(CHANGES))
def test_a_write_from_outside_the_step_is_looked_at_before_the_next_step(how):
    change, still = CHANGES[how]
    first, after, last, s1, s21 = sequence(0, change)
    assert first is True and after is still and last is still, (how, first, after, last)
    ref = sequence(NO_EQM, change)
    assert ref[:3] == (False, False, False)
    assert s1 == ref[3] and s21 == ref[4], how


def test_headline_size_one_step_with_the_queue_on():
    n = 262144
    paired, q = paired_sweeps(n, 0, 0)
    assert len(q["pieces"]) > 0 and paired > 0 and q["plan"]["np"] == n
    b, v = plummer(n)
    both_arms(n, 0, 0, b, v, steps=(1,))
