"""The equal-mass kernels with unit mass product (nb_force_symw_unit, nb_force_symw_pairs_unit: the engine's form 2) against the general ones.

Where the one G*m of an equal-mass system is a power of two the product commutes with every rounding, so the kernels keep their sums
unscaled and multiply each row once where it is stored -- the same BYTES as the equal-mass kernels (form 1), which tests/test_eqm_gpu.py
holds to the bytes of the general ones (form 0).  The yardstick here is the same: bodies, velocities and accelerations of a handle
against a handle with NB_FLAG_NO_EQM, after 1 step (a plain launch) and 20 more (the captured graph), and Simulation.eqm_form asked
before every call.  The shapes are the smallest at which each loop form runs on a plan without padding rows, masses a power of two:
  N =  8,192, force_variant 716013 / 708013 on ic.plummer (m = 2^-13): wave ranges cut inside sweeps -- the single forms;
  N = 12,288 and 20,480 with NB_FLAG_WHOLE_SWEEPS, the mass lane overwritten with 2^-14: the paired loop (checked on the plan);
  N = 65,536: the default plan.
The form follows the scalar the kernels stream -- m when G = 1, else (float)G * m: a positive normal power of two with an exponent in
[-32, 32] gives form 2, anything else form 1 -- and the G of the last set_params: a captured graph belongs to the form it was captured
in.  NB_FLAG_NO_EQM_POW2 keeps form 1, NB_FLAG_NO_EQM form 0; a system that is not eligible for the equal-mass kernels stays at form 0.
"""
import numpy as np
import pytest

from nbody3d_amd import Simulation, capi, ic
from test_eqm_gpu import paired_sweeps, poke

pytestmark = pytest.mark.gpu

WHOLE, NO_EQM, NO_POW2 = capi.NB_FLAG_WHOLE_SWEEPS, capi.NB_FLAG_NO_EQM, capi.NB_FLAG_NO_EQM_POW2
SMALL = (12288, 716013, WHOLE)        # the shape of the invalidation cases: paired and single loops both run

_systems = {}
_reference = {}


def plummer(n, mass=None):
    """ic.plummer(n) once per size and mass (None: as generated, 1 / n); the tests copy what they change."""
    if (n, None) not in _systems:
        _systems[(n, None)] = ic.plummer(n, seed=5)
    if (n, mass) not in _systems:
        b, v = _systems[(n, None)]
        b = b.copy()
        b[:, 3] = np.float32(mass)
        _systems[(n, mass)] = (b, v)
    b, v = _systems[(n, mass)]
    return b, v


def state(sim):
    return tuple(x.tobytes() for x in sim.read())


def run(n, variant, flags, b, v, gs=(1.0,), steps=(1, 20), dt=1e-3):
    """[(form, state)] after each entry of `steps`, for each G of `gs` in turn on ONE handle; then the form at the end."""
    out = []
    with Simulation(n, force_variant=variant, flags=flags) as sim:
        sim.init(b, v)
        for G in gs:
            sim.set_params(dt, G)
            for k in steps:
                form = sim.eqm_form
                assert sim.eqm is (form != 0)               # nb_eqm_info answers 1 for both equal-mass forms
                sim.simulate(k)
                out.append((form, state(sim)))
        out.append((sim.eqm_form, sim.variant))
    return out


def reference(key, n, variant, flags, b, v, gs, dt):
    """The NB_FLAG_NO_EQM handle driven the same way: once per system."""
    if key not in _reference:
        _reference[key] = run(n, variant, flags | NO_EQM, b, v, gs, dt=dt)
        assert all(f == 0 for f, _ in _reference[key])
    return _reference[key]


def both_arms(n, variant, flags, mass, forms, gs=(1.0,), system=None, dt=1e-3):
    """`forms`: the form expected at each G of `gs`."""
    b, v = system if system is not None else plummer(n, mass)
    got = run(n, variant, flags, b, v, gs, dt=dt)
    want = reference((n, variant, flags & ~NO_POW2, mass, gs, dt) if system is None else object(), n, variant, flags & ~NO_POW2, b, v, gs, dt)
    assert got[-1][1] == want[-1][1]                        # the same plan, the same variant string
    expect = [f for f in forms for _ in (1, 20)]
    assert [f for f, _ in got[:-1]] == expect and got[-1][0] == forms[-1], (n, variant, mass, gs, [f for f, _ in got])
    for k, (g, w) in enumerate(zip(got[:-1], want[:-1])):
        for name, x, y in zip(("bodies", "vel", "accel"), g[1], w[1]):
            assert x == y, (n, variant, flags, mass, gs, "call %d" % k, name)


def test_plummer_masses_are_a_power_of_two():
    b, _ = plummer(8192)
    assert np.all(b[:, 3] == np.float32(2.0 ** -13))


@pytest.mark.parametrize("variant", [716013, 708013])
def test_single_forms_at_8192(variant):
    paired, q = paired_sweeps(8192, variant, 0)
    assert q["plan"]["np"] == 8192 and q["plan"]["zc"] == 0
    both_arms(8192, variant, 0, None, [2])


@pytest.mark.parametrize("n", [12288, 20480])
@pytest.mark.parametrize("variant", [716013, 708013])
def test_paired_form_with_whole_sweeps(n, variant):
    paired, q = paired_sweeps(n, variant, WHOLE)
    assert q["plan"]["np"] == n and q["plan"]["zc"] == 0 and paired > 0, (n, variant, paired)
    both_arms(n, variant, WHOLE, 2.0 ** -14, [2])


def test_default_plan_at_65536():
    paired, q = paired_sweeps(65536, 0, 0)
    assert q["plan"]["np"] == 65536 and paired > 0
    b, _ = plummer(65536)
    assert np.all(b[:, 3] == np.float32(2.0 ** -16))
    both_arms(65536, 0, 0, None, [2])


@pytest.mark.parametrize("G,mass,form", [(2.0, None, 2), (0.25, None, 2), (0.37, None, 1), (1.0, 3 * 2.0 ** -15, 1)])
def test_g_folded_into_the_j_stream(G, mass, form):
    both_arms(8192, 716013, 0, mass, [form], gs=(G,))


def test_one_handle_through_three_values_of_g():
    # 2, 1, 2: the graph slots are keyed on the form (and on G)
    both_arms(8192, 716013, 0, None, [2, 1, 2], gs=(1.0, 0.37, 0.5))


@pytest.mark.parametrize("mass,form", [(2.0 ** -32, 2), (2.0 ** -33, 1)])
def test_the_exponent_window(mass, form):
    both_arms(8192, 716013, 0, mass, [form])


@pytest.mark.parametrize("G,form", [(2.0 ** 45, 2), (2.0 ** 46, 1), (-1.0, 1)])
def test_the_upper_edge_of_the_window_and_a_negative_g(G, form):
    # m = 2^-13: G*m = 2^32 is the last exponent of the window, 2^33 the first outside it; a negative G*m keeps form 1 (the sign bit).
    # dt = 2^-40: accelerations of order |G| move nothing far in 21 steps, so every distance stays what the other cases see
    both_arms(8192, 716013, 0, None, [form], gs=(G,), dt=2.0 ** -40)


def test_flags_keep_the_other_forms():
    both_arms(8192, 716013, NO_POW2, None, [1])
    b, v = plummer(8192)
    assert all(f == 0 for f, _ in run(8192, 716013, NO_EQM, b, v))


def sequence(flags, change):
    """Step once on the power-of-two system, change it from outside the step, step again (1, then 20: the graph)."""
    n, variant, fl = SMALL
    b, v = plummer(n, 2.0 ** -14)
    with Simulation(n, force_variant=variant, flags=fl | flags) as sim:
        sim.init(b, v)
        sim.set_params(1e-3, 1.0)
        first = sim.eqm_form
        sim.simulate(1)
        change(sim)
        after = sim.eqm_form
        sim.simulate(1)
        s1 = state(sim)
        sim.simulate(20)
        return first, after, sim.eqm_form, s1, state(sim)


def reupload_other_mass(sim):
    b, v, a = sim.read()
    b = b.copy()
    b[:, 3] = np.float32(3 * 2.0 ** -16)
    sim.restore(b, v, a)


CHANGES = {
    "upload_not_a_power_of_two": (reupload_other_mass, 1),
    "one_mass_through_the_pointer": (lambda sim: poke(sim, "bodies", 100, 3e-4), 0),
    "pointer_untouched": (lambda sim: sim.device_ptr("bodies"), 2),
}


@pytest.mark.parametrize("how", sorted(CHANGES))
def test_a_write_from_outside_the_step_changes_the_form(how):
    change, then = CHANGES[how]
    first, after, last, s1, s21 = sequence(0, change)
    assert (first, after, last) == (2, then, then), (how, first, after, last)
    ref = sequence(NO_EQM, change)
    assert ref[:3] == (0, 0, 0)
    assert s1 == ref[3] and s21 == ref[4], how


def test_ineligible_systems_stay_at_form_0():
    n, variant, flags = SMALL
    both_arms(n, variant, flags, None, [0], system=ic.uniform_cube(n))
    b, v = ic.plummer(12289, seed=5)
    both_arms(12289, variant, flags, None, [0], system=(b, v))             # padding rows
    b, v = plummer(n, 2.0 ** -14)
    v1 = v.copy()
    v1[7, 3] = 1e-3
    both_arms(n, variant, flags, None, [0], system=(b, v1))                # leapfrog would move the mass lane
