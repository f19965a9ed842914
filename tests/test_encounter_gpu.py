"""The encounter watch of block steps (Simulation.set_encounter_watch; nb_set_encounter_watch) on the GPU.
1. An exact census on an integer lattice, f32 and f64: every body's record EQUALS an O(n^2) int64 brute force (partner, rho2, count,
   time), and so do hits and passes.  N = 1025 and 4099 are no multiple of a tile: padding rows at the origin (a body sits there),
   clamped lanes past |A|, self by index, coincident bodies, ties inside a stage and across j-chunks, |A| from N / 8 up to N and
   N - 1 against N.  N = 32771 runs the full set through the 1,024-row workgroups of the f32 pass (NG = 2) and the fold's one lane per
   row, and a set of 100 bodies through more than 32 j-chunks and the fold's 64 lanes per row; the shapes are asserted.
2. Dynamic f64 runs against the CPU restatement (tests/encounter_ref.py): the Kepler pair of e = 0.9 and the N = 300 sphere with
   the tight pair.
3. Invariants: no bit of the state moves, reset and counters, read-only calls, checkpoint, NB_ENC_STOP, refusals."""
import numpy as np
import pytest

from nbody3d_amd import Simulation, capi

import block_ref as R
import encounter_ref as E

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f64": np.float64}


def hermite(n, prec, **kw):
    return Simulation(n, precision=prec, integrator="hermite4", **kw)


def state(sim):
    return tuple(x.tobytes() for x in sim.read()) + (sim.read_jerk().tobytes(), sim.read_levels().tobytes(), repr(sorted(sim.block_stats().items())))


def records_equal(got, want):
    return all(got[k].tobytes() == np.asarray(want[k], got[k].dtype).tobytes() for k in ("rho2", "partner", "time", "count"))


# ---- 1. the exact census -------------------------------------------------------------------------------------------------------
_lattice = {}


def lattice_ref(n, second, case):
    """(b, v, levels, radii, brute-force records, hits, passes): computed once per case, shared by both precisions, never written."""
    key = (n, second, case)
    if key not in _lattice:
        if n not in _lattice:
            _lattice[n] = E.lattice(n)
        b, v, _ = _lattice[n]
        lev, rad = E.lattice_levels(n, second), E.lattice_radii(n, case)
        _lattice[key] = (b, v, lev, rad) + E.lattice_brute(b, lev, rad)
    return _lattice[key]


def lattice_run(n, prec, lev, radii, b, v, L=E.LATTICE_L):
    with hermite(n, prec, eps2=E.LATTICE_EPS2) as sim:
        sim.init(b, v)
        sim.set_params(E.LATTICE_DT, 0.0)
        sim.set_block_steps(max_level=L, frozen=True)
        sim.upload_levels(lev)
        if np.all(radii == radii[0]):
            sim.set_encounter_watch(radius=float(radii[0]))
        else:
            sim.set_encounter_watch(radii=radii)
        sim.simulate(1)
        return sim.download_encounters(), sim.encounter_stats(), sim.read()[0], sim.block_stats()


@pytest.mark.parametrize("case", E.LATTICE_CASES)
@pytest.mark.parametrize("n", [1025, 4099])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_lattice_census_equals_the_brute_force(prec, n, case):
    b, v, lev, rad, want, hits, passes = lattice_ref(n, False, case)
    got, st, x, bst = lattice_run(n, prec, lev, rad, b, v)
    bad = np.nonzero((got["partner"] != want["partner"]) | (got["rho2"] != want["rho2"]) | (got["count"] != want["count"]) | (got["time"] != want["time"]))[0]
    print("lattice %s N=%d %s: %d bodies with a record, hits %d (brute force %d), passes %d, %d records differ %s"
          % (prec, n, case, int((got["partner"] != E.NONE).sum()), st["hits"], hits, st["passes"], len(bad), bad[:8]))
    assert x.tobytes() == b.astype(DT[prec]).tobytes()                 # nothing moved
    assert bst["block_steps"] == 8 and int((want["partner"] != E.NONE).sum()) >= 8
    assert not len(bad), [(int(i), {k: (got[k][i], want[k][i]) for k in got}) for i in bad[:4]]
    assert records_equal(got, want)
    assert st["hits"] == hits and st["passes"] == passes == 8 and st["stopped"] == 0
    assert st["first_time"] == want["time"].min()


@pytest.mark.parametrize("n", [1025, 4099])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_lattice_census_with_all_but_one_body_active(prec, n):
    """Every body at level 3 except body 7 at level 0: |A| = N - 1 seven times, then N."""
    b, v, lev, rad, want, hits, passes = lattice_ref(n, True, "one")
    got, st, x, bst = lattice_run(n, prec, lev, rad, b, v)
    assert bst["body_steps"] == 8 * (n - 1) + 1 and bst["block_steps"] == 8
    assert records_equal(got, want), np.nonzero(got["partner"] != want["partner"])[0][:8]
    assert st["hits"] == hits and st["passes"] == passes == 8


def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def large_ref(mixed):
    """The large census: the brute force once (every body at level 0), the other level set derived from it."""
    n = E.LARGE_N
    if "large" not in _lattice:
        b, v, _ = E.lattice(n)
        rad = E.lattice_radii(n, "one")
        _lattice["large"] = (b, v, rad) + E.lattice_brute(b, E.large_levels(n, False), rad, L=1, dtype=np.int16)
    b, v, rad, rec, hits, passes = _lattice["large"]
    lev = E.large_levels(n, mixed)
    have = rec["partner"] != E.NONE
    want = dict(rec, count=np.where(have, 2 ** lev.astype(np.int64), 0).astype(np.uint32), time=np.where(have, 2.0 ** -lev.astype(np.float64), np.inf))
    return b, v, lev, rad, want, int(want["count"].sum()), 2 if mixed else 1


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_large_census_runs_the_1024_row_pass_and_both_ends_of_the_fold(prec, mixed):
    """N = 32771.  Every body at level 0: ONE pass with |A| = N -- f32: nb_enc_fj_pk<2>, the kernel of every full-set step, and the
    fold with one lane per row.  mixed: 100 bodies at level 1 step first, a set cut into 129 chunks of one tile (nb_enc_fj_pk<1>, the
    fold with 64 lanes per row), then the full set.  The records equal the brute force; the shapes are asserted from the
    restatement of the engine's shape rule."""
    n = E.LARGE_N
    b, v, lev, rad, want, hits, passes = large_ref(mixed)
    rows, chunks, lpr = E.pass_shape(n, n, prec == "f64", cus())
    assert rows == (256 if prec == "f64" else 1024) and chunks > 1 and lpr == 1, (rows, chunks, lpr)
    if mixed:
        rows, chunks, lpr = E.pass_shape(n, E.SMALL_SET, prec == "f64", cus())
        assert rows == (256 if prec == "f64" else 512) and chunks > 32 and lpr == 64, (rows, chunks, lpr)
    got, st, x, bst = lattice_run(n, prec, lev, rad, b, v, L=1)
    bad = np.nonzero((got["partner"] != want["partner"]) | (got["rho2"] != want["rho2"]) | (got["count"] != want["count"]) | (got["time"] != want["time"]))[0]
    print("large lattice %s N=%d mixed=%s: hits %d (brute force %d), passes %d, %d records differ %s" % (prec, n, mixed, st["hits"], hits, st["passes"], len(bad), bad[:8]))
    assert x.tobytes() == b.astype(DT[prec]).tobytes()
    assert bst["block_steps"] == passes and bst["body_steps"] == n + (E.SMALL_SET if mixed else 0)
    assert not len(bad), [(int(i), {k: (got[k][i], want[k][i]) for k in got}) for i in bad[:4]]
    assert records_equal(got, want) and st["hits"] == hits and st["passes"] == passes
    assert (want["partner"] != E.NONE).sum() > n // 2 and want["partner"][0] == 1 and want["partner"][n - 1] == 5


# ---- 2. dynamic f64 runs against the restatement -------------------------------------------------------------------------------
def test_kepler_pericentre_is_seen_inside_the_outer_step():
    """The restatement records the second pericentre passage at rho2 - eps2 = PERICENTRE2 + 2.37e-6 (its own distance from the
    analytic (a (1 - e))^2 = 0.01, measured on the CPU: E.KEPLER_DISTANCE); the engine is held to twice that, to the restatement
    within the project's fp64 bound 1e-12, and to the same partner and time.  nb_neighbors at the outer-step boundaries never
    sees the pair that close."""
    b0, v0, ref, want, rst = E.kepler_watch_ref()
    k = E.KEPLER
    boundary = []
    with hermite(2, "f64", eps2=k["eps2"]) as sim:
        sim.init(b0, v0)
        sim.set_params(k["dt"], k["G"])
        sim.set_block_steps(eta=k["eta"], max_level=k["max_level"])
        sim.set_encounter_watch(radius=k["radius"])
        sim.simulate(1)
        sim.reset_encounters()
        boundary.append(sim.neighbors(bodies=(0, 2))[1].min())
        for _ in range(k["outer"] - 1):
            sim.simulate(1)
            boundary.append(sim.neighbors(bodies=(0, 2))[1].min())
        got, st = sim.download_encounters(), sim.encounter_stats()
    seen = got["rho2"] - k["eps2"]
    print("kepler: recorded rho2 - eps2 = %s at t = %s (restatement %s at %s), distance from the analytic pericentre %s (restatement %.4g); "
          "closest boundary distance^2 %.4g; hits %d (restatement %d)"
          % (seen, got["time"], want["rho2"] - k["eps2"], want["time"], np.abs(seen - E.PERICENTRE2), E.KEPLER_DISTANCE, min(boundary), st["hits"], rst["hits"]))
    assert np.array_equal(got["partner"], [1, 0]) and np.array_equal(got["partner"], want["partner"])
    assert np.array_equal(got["time"], want["time"]) and np.all(got["time"] > k["outer"] - 1)
    assert np.abs(got["rho2"] / want["rho2"] - 1).max() <= 1e-12
    assert np.abs(seen - E.PERICENTRE2).max() <= 2 * E.KEPLER_DISTANCE
    assert min(boundary) > 4 * seen.max()                          # the boundaries never come near it


def test_dynamic_levels_on_300_bodies_against_the_restatement():
    b0, v0, ref, want, rst = E.pair300_watch_ref()
    k = E.PAIR300
    with hermite(300, "f64") as sim:
        sim.init(b0, v0)
        sim.set_params(k["dt"], k["G"])
        sim.set_block_steps(eta=k["eta"], max_level=k["max_level"])
        sim.set_encounter_watch(radius=k["radius"])
        sim.simulate(k["outer"])
        got, st = sim.download_encounters(), sim.encounter_stats()
    have = want["partner"] != E.NONE
    err = np.abs(got["rho2"][have] / want["rho2"][have] - 1).max()
    print("N=300: %d bodies with a record (restatement %d), rho2 within %.3g, hits %d (restatement %d), passes %d (%d), %d partners and %d times differ"
          % (int((got["partner"] != E.NONE).sum()), int(have.sum()), err, st["hits"], rst["hits"], st["passes"], rst["passes"],
             int((got["partner"] != want["partner"]).sum()), int((got["time"] != want["time"]).sum())))
    assert have.sum() > 50 and want["partner"][0] == 1 and want["partner"][1] == 0
    assert np.array_equal(got["partner"], want["partner"])
    assert np.array_equal(got["time"], want["time"])
    assert err <= 1e-12


# ---- 3. invariants -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_no_bit_moves(prec):
    """A twin with the watch off holds the same bits after the same steps: frozen mixed levels on the lattice system with G = 1 at
    N = 1025 (f32: the 512-row kernel, several j-chunks) and at N = 32771 (f32: 100 bodies through the 512-row kernel, the full set
    through the 1,024-row one; test_large_census asserts these shapes) and, f64, dynamic levels on the N = 300 input."""
    runs = [(1025, E.lattice(1025)[:2], dict(max_level=3, frozen=True), E.lattice_levels(1025), 2.0 ** -10, 4.0, E.LATTICE_EPS2),
            (E.LARGE_N, E.lattice(E.LARGE_N)[:2], dict(max_level=1, frozen=True), E.large_levels(E.LARGE_N, True), 2.0 ** -10, 4.0, E.LATTICE_EPS2)]
    if prec == "f64":
        runs.append((300, E.pair300(), dict(eta=0.02, max_level=12), None, 2.0 ** -4, 0.1, None))
    for n, (b0, v0), blk, lev, dt, h, eps2 in runs:
        got = []
        for watch in (True, False):
            with hermite(n, prec, **({} if eps2 is None else {"eps2": eps2})) as sim:
                sim.init(b0, v0)
                sim.set_params(dt, 1.0)
                sim.set_block_steps(**blk)
                if lev is not None:
                    sim.upload_levels(lev)
                if watch:
                    sim.set_encounter_watch(radius=h)
                sim.simulate(2)
                got.append(state(sim))
                if watch:
                    assert sim.encounter_stats()["hits"] > 0
        assert got[0] == got[1], n


def test_reset_counters_and_read_only_calls():
    b0, v0 = E.pair300()
    k = E.PAIR300
    with hermite(300, "f64") as sim:
        sim.init(b0, v0)
        sim.set_params(k["dt"], k["G"])
        sim.set_block_steps(eta=k["eta"], max_level=k["max_level"])
        sim.set_encounter_watch(radius=k["radius"])
        sim.simulate(1)
        rec, st = sim.download_encounters(), sim.encounter_stats()
        assert st["hits"] == rec["count"].sum() > 0 and st["passes"] == sim.block_stats()["block_steps"]
        # read-only calls change no record and no counter
        sim.force_pass(1)
        sim.neighbors(bodies=(0, 300), radius=0.1)
        sim.read(), sim.read_jerk(), sim.read_levels()
        assert records_equal(sim.download_encounters(), rec) and sim.encounter_stats() == st
        # reset = 1: the counters only
        assert sim.encounter_stats(reset=True) == st
        z = sim.encounter_stats()
        assert z["hits"] == 0 and z["passes"] == 0 and z["first_time"] == np.inf
        assert records_equal(sim.download_encounters(), rec)
        # nb_reset_encounters: the records too
        sim.reset_encounters()
        assert records_equal(sim.download_encounters(), E.new_records(300, np.float64))
        # a new upload keeps the configuration and clears the records
        sim.simulate(1)
        assert (sim.download_encounters()["partner"] != E.NONE).any()
        sim.init(b0, v0)
        assert records_equal(sim.download_encounters(), E.new_records(300, np.float64))
        sim.simulate(1)                                            # the same outer step again; the times count the handle's own outer steps
        again = sim.download_encounters()
        assert np.array_equal(again["partner"], rec["partner"]) and again["rho2"].tobytes() == rec["rho2"].tobytes()
        assert np.array_equal(again["count"], rec["count"])
        assert np.array_equal(again["time"][again["partner"] != E.NONE], rec["time"][rec["partner"] != E.NONE] + 2)


def test_checkpoint_continues_bit_for_bit():
    """Everything downloaded at step 2 and uploaded into a second handle (that has run two outer steps of its own, so that its
    clock stands at 2 as well): at step 4 the state and the records are those of the uninterrupted run."""
    b0, v0 = E.pair300()
    k = E.PAIR300
    blk = dict(eta=k["eta"], max_level=k["max_level"])
    with hermite(300, "f64") as one, hermite(300, "f64") as two:
        for s in (one, two):
            s.init(b0, v0)
            s.set_params(k["dt"], k["G"])
            s.set_block_steps(**blk)
        one.set_encounter_watch(radius=k["radius"])
        one.simulate(2)
        two.simulate(2)
        cb, cv, ca = one.read()
        cj, cl, crec = one.read_jerk(), one.read_levels(), one.download_encounters()
        one.simulate(2)
        two.init(cb, cv)
        two.upload_derivs(ca, cj)
        two.set_encounter_watch(radius=k["radius"])
        two.upload_levels(cl)
        two.upload_encounters(**crec)
        two.simulate(2)
        assert state(one)[:5] == state(two)[:5]
        a, b = one.download_encounters(), two.download_encounters()
        assert records_equal(a, b) and not records_equal(a, crec)


def test_stop_returns_after_the_first_hit_step():
    b0, v0, rad, ref, want, rst = E.stop_ref()
    k, outer = E.PAIR300, E.STOP["outer"]
    first = int(np.nonzero(np.array(rst["hits_after"]) > 0)[0][0]) + 1          # the restatement's first outer step with a hit
    assert 1 < first < outer
    with hermite(300, "f64") as sim:
        sim.init(b0, v0)
        sim.set_params(k["dt"], k["G"])
        sim.set_block_steps(eta=k["eta"], max_level=k["max_level"])
        sim.set_encounter_watch(radii=rad, stop=True)
        sim.simulate(outer)
        st = sim.encounter_stats()
        print("stop: returned after outer step %d (restatement: first hit in step %d, first_time %s), %s" % (sim.block_stats()["outer_steps"], first, rst["first_time"], st))
        assert sim.block_stats()["outer_steps"] == first and st["stopped"] == 1 and st["steps_left"] == outer - first
        assert st["hits"] == rst["hits_after"][first - 1] and st["first_time"] == rst["first_time"]
        rec = sim.download_encounters()
        assert set(np.nonzero(rec["partner"] != E.NONE)[0]) <= set(E.STOP["bodies"])
        sim.simulate(1)                                            # hits still stand: one outer step, stopped again
        assert sim.encounter_stats()["steps_left"] == 0 and sim.block_stats()["outer_steps"] == first + 1
        sim.reset_encounters()
        assert sim.encounter_stats()["stopped"] == 0
        sim.set_encounter_watch(radius=0.0, stop=True)             # nobody watched: nothing stops it
        sim.simulate(2)
        st = sim.encounter_stats()
        assert st["stopped"] == 0 and st["steps_left"] == 0 and st["hits"] == 0 and sim.block_stats()["outer_steps"] == first + 3


def test_refusals():
    b0, v0 = E.pair300()

    def state_error(call):
        with pytest.raises(capi.NBodyError) as e:
            call()
        assert e.value.code == 4 and "encounter" in str(e.value), str(e.value)

    with Simulation(300) as leap:                                      # not a Hermite handle
        state_error(lambda: leap.set_encounter_watch(radius=0.1))
    for prec in ("f32", "f64"):
        with hermite(300, prec) as sim:
            sim.init(b0, v0)
            sim.set_params(2.0 ** -4, 1.0)
            state_error(lambda: sim.set_encounter_watch(radius=0.1))           # block steps off
            state_error(lambda: sim.download_encounters())
            sim.set_hermite_order(6)
            state_error(lambda: sim.set_encounter_watch(radius=0.1))           # an order-6 handle
            sim.set_hermite_order(4)
            sim.set_block_steps(max_level=4)
            sim.set_block_batch()
            state_error(lambda: sim.set_encounter_watch(radius=0.1))           # a batched mode on
            sim.set_block_batch(None)
            if prec == "f64":
                sim.set_pass_precision("mixed")
                state_error(lambda: sim.set_encounter_watch(radius=0.1))       # a mixed pass
                sim.set_pass_guard(0.01)
                state_error(lambda: sim.set_encounter_watch(radius=0.1))       # a guarded pass
                sim.set_pass_precision("native")
            sim.set_encounter_watch(radius=0.1)
            for call in (sim.set_block_batch, sim.set_block_batch6, sim.set_block_batch_mixed, lambda: sim.set_hermite_order(6)):
                state_error(call)
            if prec == "f64":
                state_error(lambda: sim.set_pass_precision("mixed"))
            for call in (lambda: sim.set_pass_precision("mixed"), lambda: sim.set_neighbor_scheme(radius=0.1)):      # (f32: no mixed pass at all; block steps exclude the scheme)
                with pytest.raises(capi.NBodyError) as e:
                    call()
                assert e.value.code == 4
            sim.simulate(1)
            assert sim.encounter_stats()["passes"] > 0
            sim.set_block_steps(None)                                          # switches the watch off
            state_error(lambda: sim.encounter_stats())
            sim.set_neighbor_scheme(radius=0.1)                                # the neighbour scheme on
            state_error(lambda: sim.set_encounter_watch(radius=0.1))
