"""The encounter watch inside batched block steps (Simulation.set_block_batch_watch; nb_set_block_batch_watch) on the GPU.
1. An exact census on the integer lattice, f32 and f64, G = 0, frozen levels, L = 3: every record EQUALS the int64 brute force
   (partner, rho2, count, time), and so do hits, passes == 8 and first_time; the path every block step took (small slot or host
   step) is asserted from nb_block_batch_stats.  The level sets put |A| at, one below and one above small_max, one body alone in a
   workgroup, fewer and more j-chunks than the corrector has sum lanes, ties between the quarters of a tile (the four-wave merge)
   and between chunks, and at N = 66,307 more than one tile per chunk.
2. Dynamic f64 runs against the CPU restatement (tests/encounter_ref.py): the Kepler pair and the N = 300 sphere with the tight pair.
3. Invariants: the unwatched batch twin, small_max = 0, depth, k x 1 step, the active list, counters, read-only calls, checkpoint,
   NB_ENC_STOP, upload.
4. Switching and refusals."""
import ctypes as C

import numpy as np
import pytest

from nbody3d_amd import Simulation, capi

import encounter_ref as E
import encounter_batch_ref as B

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f64": np.float64}


def hermite(n, prec, **kw):
    return Simulation(n, precision=prec, integrator="hermite4", **kw)


def state(sim):
    return tuple(x.tobytes() for x in sim.read()) + (sim.read_jerk().tobytes(), sim.read_levels().tobytes(), repr(sorted(sim.block_stats().items())))


def records_equal(got, want):
    return all(got[k].tobytes() == np.asarray(want[k], got[k].dtype).tobytes() for k in ("rho2", "partner", "time", "count"))


def watch_on(sim, radii, **kw):
    radii = np.asarray(radii, np.float64)
    if radii.ndim == 0 or np.all(radii == radii.flat[0]):
        return sim.set_encounter_watch(radius=float(radii.flat[0]), **kw)
    return sim.set_encounter_watch(radii=radii, **kw)


def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- 1. the exact census -------------------------------------------------------------------------------------------------------
_ref = {}


def lattice(n):
    if ("lattice", n) not in _ref:
        _ref["lattice", n] = E.lattice(n)
    return _ref["lattice", n]


def census_ref(n, levels, case):
    """(b, v, levels, radii, brute-force records, hits, passes): computed once per (n, level set, case), shared by both precisions."""
    key = (n, levels, case)
    if key not in _ref:
        b, v, _ = lattice(n)
        lev = E.lattice_levels(n) if levels == "mod4" else B.small_set_levels(n, *levels)
        rad = E.lattice_radii(n, case)
        _ref[key] = (b, v, lev, rad) + E.lattice_brute(b, lev, rad)
    return _ref[key]


def census_run(n, prec, lev, radii, b, v, small_max, depth=None):
    with hermite(n, prec, eps2=E.LATTICE_EPS2) as sim:
        sim.init(b, v)
        sim.set_params(E.LATTICE_DT, 0.0)
        sim.set_block_steps(max_level=E.LATTICE_L, frozen=True)
        watch_on(sim, radii)
        sim.set_block_batch_watch(depth=depth, small_max=small_max)
        sim.upload_levels(lev)
        sim.simulate(1)
        return sim.download_encounters(), sim.encounter_stats(), sim.read()[0], sim.block_stats(), sim.block_batch_stats()


def census_check(tag, prec, n, ref, small_max, path):
    b, v, lev, rad, want, hits, passes = ref
    got, st, x, bst, qst = census_run(n, prec, lev, rad, b, v, small_max)
    bad = np.nonzero((got["partner"] != want["partner"]) | (got["rho2"] != want["rho2"]) | (got["count"] != want["count"]) | (got["time"] != want["time"]))[0]
    print("%s %s N=%d small_max=%d: %d bodies with a record, hits %d (brute force %d), passes %d, small %d, host %d, %d records differ %s"
          % (tag, prec, n, small_max, int((got["partner"] != E.NONE).sum()), st["hits"], hits, st["passes"], qst["small_steps"], qst["host_steps"], len(bad), bad[:8]))
    assert x.tobytes() == b.astype(DT[prec]).tobytes()                 # nothing moved
    assert qst["enabled"] == 1 and (qst["small_steps"], qst["host_steps"]) == path == B.expected_path(lev, small_max)
    assert bst["block_steps"] == 8 and bst["body_steps"] == sum(B.active_counts(lev))
    assert not len(bad), [(int(i), {k: (got[k][i], want[k][i]) for k in got}) for i in bad[:4]]
    assert records_equal(got, want)
    assert st["hits"] == hits > 0 and st["passes"] == passes == 8 and st["stopped"] == 0
    assert st["first_time"] == want["time"].min()
    return want


@pytest.mark.parametrize("case", E.LATTICE_CASES)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_census_with_seven_small_steps(prec, case):
    """N = 1025, l = i mod 4, small_max 1024: |A| = 256, 512, 256, 768, 256, 512, 256 in small slots, then the full set on the host;
    5 j-chunks on an MI355X, fewer than the corrector's 16 sum lanes.  With h = 4 some bodies that step in small slots have their
    smallest rho^2 tied between quarters of one tile (the four-wave merge) and some between tiles (chunks)."""
    ref = census_ref(1025, "mod4", case)
    b, lev, rad = ref[0], ref[2], ref[3]
    want = census_check("census", prec, 1025, ref, 1024, (7, 1))
    if case == "one":
        if "ties" not in _ref:
            _ref["ties"] = B.ties(b, rad)
        quarter, tile = _ref["ties"]
        small = lambda i: lev[i] > 0 and rad[i] > 0 and want["partner"][i] != E.NONE
        assert sum(small(i) for i in quarter) >= 2 and sum(small(i) for i in tile) >= 8, (quarter, tile)
    if case == "coincident":
        assert sorted(np.nonzero(want["partner"] != E.NONE)[0]) == sorted(i for p in lattice(1025)[2] for i in p)


@pytest.mark.parametrize("small_max", [1024, 1023])
@pytest.mark.parametrize("case", ["one", "per_body"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_census_at_and_below_the_largest_small_step(prec, case, small_max):
    """N = 4099, l = i mod 4: |A| = 1024 at the odd ticks -- exactly small_max = 1024, so those four are small; at 1023 every step
    parks and the eight are host steps.  17 j-chunks on an MI355X, more than the 16 sum lanes."""
    census_check("census", prec, 4099, census_ref(4099, "mod4", case), small_max, (4, 4) if small_max == 1024 else (0, 8))


@pytest.mark.parametrize("shape", [(129, 127, 256), (1, 63, 64)])
@pytest.mark.parametrize("case", E.LATTICE_CASES)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_census_of_small_sets(prec, case, shape):
    """N = 1025.  (129, 127) with small_max 256: |A| = 129 at the odd ticks (f32: a second workgroup with one slot; f64: a third
    with one), 256 at ticks 2 and 6 (= small_max), 257 at tick 4, which parks.  (1, 63) with small_max 64: |A| = 1 at the odd
    ticks (every other lane clamped), 64 at ticks 2 and 6, 65 at tick 4.  The level-3 set of the first holds the origin where
    padding rows sit, both ends of every coincident pair and two quarter-tie bodies; that of the second is body 0."""
    deep, mid, small_max = shape
    ref = census_ref(1025, (deep, mid), case)
    want = census_check("small sets", prec, 1025, ref, small_max, (6, 2))
    if case != "coincident":
        assert want["partner"][0] == 1 and want["count"][0] == 8 and want["time"][0] == 0.125 or ref[3][0] < 1.2


def large_ref():
    """N = 66,307: 100 bodies spread over the system at level 3, and only they have a radius; the brute force over those rows."""
    if "large" not in _ref:
        n = 66307
        b, v, _ = lattice(n)
        rows = np.linspace(3, n - 1, 100).astype(np.int64)
        lev, rad = np.zeros(n, np.uint8), np.zeros(n)
        lev[rows], rad[rows] = 3, 4.0
        rho2, partner = B.rows_brute(b, rows, 16)
        want = E.new_records(n, np.float64)
        have = partner != E.NONE
        want["rho2"][rows[have]], want["partner"][rows[have]] = rho2[have], partner[have]
        want["count"][rows[have]], want["time"][rows[have]] = 8, 0.125
        _ref["large"] = (n, b, v, lev, rad, rows, want, 8 * int(have.sum()))
    return _ref["large"]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_census_with_several_tiles_per_chunk(prec):
    """A lane's best runs across the tiles of one chunk.  The records' time is 2^-3: the first small step's answer, which the
    full-set step at the end of the outer step can only repeat (strictly smaller replaces), so a wrong small answer cannot hide."""
    n, b, v, lev, rad, rows, want, hits = large_ref()
    chunks, per = B.bb_shape(n, cus())
    if cus() > 258:
        pytest.skip("%d CUs: %d chunks of %d bodies, one tile per chunk" % (cus(), chunks, per))
    assert per > B.TILE and chunks > 16, (cus(), chunks, per)
    got, st, x, bst, qst = census_run(n, prec, lev, rad, b, v, 256)
    bad = np.nonzero((got["partner"] != want["partner"]) | (got["rho2"] != want["rho2"]) | (got["count"] != want["count"]) | (got["time"] != want["time"]))[0]
    print("large census %s: %d chunks of %d, %d of 100 rows with a record, hits %d (brute force %d), small %d, host %d, %d records differ %s"
          % (prec, chunks, per, int((got["partner"] != E.NONE).sum()), st["hits"], hits, qst["small_steps"], qst["host_steps"], len(bad), bad[:8]))
    assert x.tobytes() == b.astype(DT[prec]).tobytes()
    assert (qst["small_steps"], qst["host_steps"]) == (7, 1) and bst["body_steps"] == 7 * 100 + n
    assert not len(bad), [(int(i), {k: (got[k][i], want[k][i]) for k in got}) for i in bad[:4]]
    assert records_equal(got, want) and st["hits"] == hits and st["passes"] == 8 and st["first_time"] == 0.125
    have = want["partner"] != E.NONE
    assert have.sum() > 50 and set(np.nonzero(have)[0]) <= set(rows) and np.all(want["time"][have] == 0.125)
    assert want["partner"][n - 1] == 5 and want["rho2"][n - 1] == E.LATTICE_EPS2


# ---- 2. dynamic f64 runs against the restatement -------------------------------------------------------------------------------
def test_kepler_pericentre_is_seen_inside_small_slots():
    """|A| <= n = 2: every block step but the last of an outer step is a small slot.  To the restatement within the project's fp64
    bound 1e-12, the same partner and time, and to the analytic pericentre within twice the restatement's own distance."""
    b0, v0, ref, want, rst = E.kepler_watch_ref()
    k = E.KEPLER
    with hermite(2, "f64", eps2=k["eps2"]) as sim:
        sim.init(b0, v0)
        sim.set_params(k["dt"], k["G"])
        sim.set_block_steps(eta=k["eta"], max_level=k["max_level"])
        sim.set_encounter_watch(radius=k["radius"])
        sim.set_block_batch_watch()
        sim.simulate(1)
        sim.reset_encounters()
        sim.block_batch_stats(reset=True)
        sim.simulate(k["outer"] - 1)
        got, st, qst, bst = sim.download_encounters(), sim.encounter_stats(), sim.block_batch_stats(), sim.block_stats()
    seen = got["rho2"] - k["eps2"]
    print("kepler: recorded rho2 - eps2 = %s at t = %s (restatement %s at %s), distance from the analytic pericentre %s (restatement %.4g); "
          "hits %d (restatement %d), %d small and %d host steps"
          % (seen, got["time"], want["rho2"] - k["eps2"], want["time"], np.abs(seen - E.PERICENTRE2), E.KEPLER_DISTANCE, st["hits"], rst["hits"],
             qst["small_steps"], qst["host_steps"]))
    assert qst["small_steps"] > 0 and qst["host_steps"] == k["outer"] - 1
    assert st["passes"] == qst["small_steps"] + qst["host_steps"]
    assert np.array_equal(got["partner"], [1, 0]) and np.array_equal(got["partner"], want["partner"])
    assert np.array_equal(got["time"], want["time"]) and np.all(got["time"] > k["outer"] - 1) and np.all(got["time"] != np.round(got["time"]))
    assert np.abs(got["rho2"] / want["rho2"] - 1).max() <= 1e-12
    assert np.abs(seen - E.PERICENTRE2).max() <= 2 * E.KEPLER_DISTANCE


def test_dynamic_levels_on_300_bodies_against_the_restatement():
    b0, v0, ref, want, rst = E.pair300_watch_ref()
    k = E.PAIR300
    with hermite(300, "f64") as sim:
        sim.init(b0, v0)
        sim.set_params(k["dt"], k["G"])
        sim.set_block_steps(eta=k["eta"], max_level=k["max_level"])
        sim.set_encounter_watch(radius=k["radius"])
        sim.set_block_batch_watch(small_max=256)
        sim.simulate(k["outer"])
        got, st, qst, bst = sim.download_encounters(), sim.encounter_stats(), sim.block_batch_stats(), sim.block_stats()
    have = want["partner"] != E.NONE
    err = np.abs(got["rho2"][have] / want["rho2"][have] - 1).max()
    print("N=300: %d bodies with a record (restatement %d), rho2 within %.3g, hits %d (restatement %d), passes %d (%d), %d small and %d host steps, "
          "%d partners and %d times differ"
          % (int((got["partner"] != E.NONE).sum()), int(have.sum()), err, st["hits"], rst["hits"], st["passes"], rst["passes"], qst["small_steps"],
             qst["host_steps"], int((got["partner"] != want["partner"]).sum()), int((got["time"] != want["time"]).sum())))
    assert qst["small_steps"] > 0 and st["passes"] == bst["block_steps"] == qst["small_steps"] + qst["host_steps"]
    assert have.sum() > 50 and want["partner"][0] == 1 and want["partner"][1] == 0
    assert np.array_equal(got["partner"], want["partner"])
    assert np.array_equal(got["time"], want["time"])
    assert err <= 1e-12
    assert np.all(got["time"][:2] != np.round(got["time"][:2]))      # the pair's members: seen inside an outer step
    assert st["hits"] == got["count"].sum()


# ---- 3. invariants -------------------------------------------------------------------------------------------------------------
def lattice_g1(sim, n=1025):
    b, v, _ = lattice(n)
    sim.init(b, v)
    sim.set_params(2.0 ** -10, 1.0)
    sim.set_block_steps(max_level=3, frozen=True)
    return E.lattice_levels(n)


def pair300_on(sim):
    k = E.PAIR300
    sim.init(*E.pair300())
    sim.set_params(k["dt"], k["G"])
    sim.set_block_steps(eta=k["eta"], max_level=k["max_level"])
    return None


@pytest.mark.parametrize("run", ["lattice_f32", "lattice_f64", "pair300_f64"])
def test_the_unwatched_batch_twin_holds_the_same_bits(run):
    """nb_set_block_batch with the same small_max and no watch: the same state, levels, nb_block_stats and nb_block_batch_stats."""
    name, prec = run.split("_")
    n, kw, h, small_max = (1025, {"eps2": E.LATTICE_EPS2}, 4.0, 512) if name == "lattice" else (300, {}, E.PAIR300["radius"], 256)
    got = []
    for watch in (True, False):
        with hermite(n, prec, **kw) as sim:
            lev = lattice_g1(sim) if name == "lattice" else pair300_on(sim)
            if watch:
                sim.set_encounter_watch(radius=h)
                sim.set_block_batch_watch(depth=8, small_max=small_max)
            else:
                sim.set_block_batch(depth=8, small_max=small_max)
            if lev is not None:
                sim.upload_levels(lev)
            sim.simulate(2)
            got.append(state(sim) + (repr(sorted(sim.block_batch_stats().items())),))
            assert sim.block_batch_stats()["small_steps"] > 0
            if watch:
                assert sim.encounter_stats()["hits"] > 0
    assert got[0] == got[1]


@pytest.mark.parametrize("run", ["lattice_f32", "lattice_f64", "pair300_f64"])
def test_small_max_zero_is_the_watch_without_the_mode(run):
    name, prec = run.split("_")
    n, kw, h = (1025, {"eps2": E.LATTICE_EPS2}, 4.0) if name == "lattice" else (300, {}, E.PAIR300["radius"])
    got = []
    for mode in (True, False):
        with hermite(n, prec, **kw) as sim:
            lev = lattice_g1(sim) if name == "lattice" else pair300_on(sim)
            sim.set_encounter_watch(radius=h)
            if mode:
                sim.set_block_batch_watch(small_max=0)
            if lev is not None:
                sim.upload_levels(lev)
            sim.simulate(2)
            got.append((state(sim), sim.download_encounters(), sim.encounter_stats()))
            if mode:
                assert sim.block_batch_stats()["small_steps"] == 0 and sim.block_batch_stats()["host_steps"] == sim.block_stats()["block_steps"]
    assert got[0][0] == got[1][0] and records_equal(got[0][1], got[1][1]) and got[0][2] == got[1][2] and got[0][2]["hits"] > 0


@pytest.mark.parametrize("run", ["lattice_f32", "pair300_f64"])
def test_depth_and_the_split_of_nb_step_change_nothing(run):
    """Depth 1, 7 and 32, and simulate(3) against 3 x simulate(1): equal state, records and counters."""
    name, prec = run.split("_")
    n, kw, h, small_max = (1025, {"eps2": E.LATTICE_EPS2}, 4.0, 512) if name == "lattice" else (300, {}, E.PAIR300["radius"], 256)
    got = []
    for depth, split in ((1, False), (7, False), (32, False), (32, True)):
        with hermite(n, prec, **kw) as sim:
            lev = lattice_g1(sim) if name == "lattice" else pair300_on(sim)
            sim.set_encounter_watch(radius=h)
            sim.set_block_batch_watch(depth=depth, small_max=small_max)
            if lev is not None:
                sim.upload_levels(lev)
            if split:
                for _ in range(3):
                    sim.simulate(1)
            else:
                sim.simulate(3)
            st, rec = sim.encounter_stats(), sim.download_encounters()
            got.append((state(sim), rec, st))
            assert st["hits"] == rec["count"].sum() > 0 and st["passes"] == sim.block_stats()["block_steps"]
            assert sim.block_batch_stats()["small_steps"] > 0
    for g in got[1:]:
        assert g[0] == got[0][0] and records_equal(g[1], got[0][1]) and g[2] == got[0][2]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_first_step_record_does_not_depend_on_the_active_list(prec):
    """The N = 300 input with G = 0 (straight lines: the predicted rows of the first block step are the same whatever the levels
    are), frozen levels, L = 1.  Five bodies step at tick 1 alone, and among 256 (= small_max; other places in the list, other
    workgroups, no clamped lane).  Where both runs recorded the first step's answer (time 1/2), it is the same bits."""
    b0, v0 = E.pair300()
    few = np.array([3, 7, 10, 51, 299])      # (their nearest neighbours recede: the first step's answer is the smaller one)
    many = np.concatenate([np.arange(255), [299]])
    got = []
    for rows in (few, many):
        lev = np.zeros(300, np.uint8)
        lev[rows] = 1
        with hermite(300, prec) as sim:
            sim.init(b0, v0)
            sim.set_params(2.0 ** -4, 0.0)
            sim.set_block_steps(max_level=1, frozen=True)
            sim.set_encounter_watch(radius=0.5)
            sim.set_block_batch_watch(small_max=256)
            sim.upload_levels(lev)
            sim.simulate(1)
            qst = sim.block_batch_stats()
            assert (qst["small_steps"], qst["host_steps"]) == (1, 1)
            got.append(sim.download_encounters())
    a, b = got
    both = [i for i in few if a["time"][i] == 0.5 and b["time"][i] == 0.5]
    print("first-step records of %s in both runs" % both)
    assert len(both) >= 2
    for i in both:
        assert a["rho2"][i].tobytes() == b["rho2"][i].tobytes() and a["partner"][i] == b["partner"][i] != E.NONE


def test_counters_read_only_calls_and_upload():
    b0, v0 = E.pair300()
    with hermite(300, "f64") as sim:
        pair300_on(sim)
        sim.set_encounter_watch(radius=E.PAIR300["radius"])
        sim.set_block_batch_watch(small_max=256)
        sim.simulate(1)
        rec, st, bst = sim.download_encounters(), sim.encounter_stats(), state(sim)
        assert st["hits"] == rec["count"].sum() > 0 and st["passes"] == sim.block_stats()["block_steps"]
        # read-only calls change no record, no counter and no bit of the state
        sim.force_pass(1)
        sim.neighbors(bodies=(0, 300), radius=0.1)
        sim.read(), sim.read_jerk(), sim.read_levels(), sim.block_batch_stats()
        assert records_equal(sim.download_encounters(), rec) and sim.encounter_stats() == st and state(sim) == bst
        # a new upload keeps the configuration and the mode and clears the records
        sim.init(b0, v0)
        assert records_equal(sim.download_encounters(), E.new_records(300, np.float64))
        assert sim.block_batch_stats()["enabled"] == 1
        sim.block_batch_stats(reset=True)
        sim.simulate(1)                                            # the same outer step again; the times count the handle's own outer steps
        again = sim.download_encounters()
        assert sim.block_batch_stats()["small_steps"] > 0
        assert np.array_equal(again["partner"], rec["partner"]) and again["rho2"].tobytes() == rec["rho2"].tobytes()
        assert np.array_equal(again["count"], rec["count"])
        assert np.array_equal(again["time"][again["partner"] != E.NONE], rec["time"][rec["partner"] != E.NONE] + 1)


def test_checkpoint_continues_bit_for_bit():
    """Everything downloaded at step 2 and uploaded into a second handle (that has run two outer steps of its own, so that its
    clock stands at 2 as well), in the header's order and with another depth: at step 4 the state and the records are those of
    the uninterrupted run."""
    k = E.PAIR300
    with hermite(300, "f64") as one, hermite(300, "f64") as two:
        for s in (one, two):
            pair300_on(s)
        one.set_encounter_watch(radius=k["radius"])
        one.set_block_batch_watch(depth=32, small_max=256)
        one.simulate(2)
        two.simulate(2)
        cb, cv, ca = one.read()
        cj, cl, crec = one.read_jerk(), one.read_levels(), one.download_encounters()
        one.simulate(2)
        two.init(cb, cv)
        two.upload_derivs(ca, cj)
        two.set_block_steps(eta=k["eta"], max_level=k["max_level"])
        two.set_encounter_watch(radius=k["radius"])
        two.set_block_batch_watch(depth=5, small_max=256)
        two.upload_levels(cl)
        two.upload_encounters(**crec)
        two.simulate(2)
        assert state(one)[:5] == state(two)[:5]
        a, b = one.download_encounters(), two.download_encounters()
        assert records_equal(a, b) and not records_equal(a, crec)
        assert two.block_batch_stats()["small_steps"] > 0


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
        sim.set_block_batch_watch(small_max=256)
        sim.simulate(outer)
        st, qst = sim.encounter_stats(), sim.block_batch_stats()
        print("stop: returned after outer step %d (restatement: first hit in step %d, first_time %s), %s, %s" % (sim.block_stats()["outer_steps"], first, rst["first_time"], st, qst))
        assert sim.block_stats()["outer_steps"] == first and st["stopped"] == 1 and st["steps_left"] == outer - first
        assert st["hits"] == rst["hits_after"][first - 1] and st["first_time"] == rst["first_time"]
        assert qst["small_steps"] > 0 and st["first_time"] != np.round(st["first_time"])
        rec = sim.download_encounters()
        assert set(np.nonzero(rec["partner"] != E.NONE)[0]) <= set(E.STOP["bodies"]) and (rec["partner"] != E.NONE).any()
        sim.simulate(1)                                            # hits still stand: one outer step, stopped again
        assert sim.encounter_stats()["steps_left"] == 0 and sim.block_stats()["outer_steps"] == first + 1
        sim.reset_encounters()
        assert sim.encounter_stats()["stopped"] == 0
        sim.set_encounter_watch(radius=0.0, stop=True)             # re-configured while the mode is on; nobody watched: nothing stops it
        sim.simulate(2)
        st = sim.encounter_stats()
        assert st["stopped"] == 0 and st["steps_left"] == 0 and st["hits"] == 0 and sim.block_stats()["outer_steps"] == first + 3
        assert sim.block_batch_stats()["enabled"] == 1


# ---- 4. switching and refusals -------------------------------------------------------------------------------------------------
def error(call, code, *words):
    with pytest.raises(capi.NBodyError) as e:
        call()
    assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)


def test_switching():
    with hermite(300, "f64") as sim:
        pair300_on(sim)
        sim.set_encounter_watch(radius=0.1)
        enabled = lambda: sim.block_batch_stats()["enabled"]
        for off in (sim.set_block_batch_watch, sim.set_block_batch, sim.set_block_batch6, sim.set_block_batch_mixed):
            sim.set_block_batch_watch()
            assert enabled() == 1
            off(None)                                              # the mode off, the watch stays
            assert enabled() == 0
            sim.encounter_stats()
        sim.set_block_batch_watch(depth=4, small_max=128)
        sim.simulate(1)
        rec, st = sim.download_encounters(), sim.encounter_stats()
        assert st["hits"] > 0
        # re-configuration while the mode is on: radii and flags anew, records and counters kept, the mode stays
        sim.set_encounter_watch(radius=0.05, stop=False)
        assert enabled() == 1 and records_equal(sim.download_encounters(), rec) and sim.encounter_stats() == st
        sim.set_block_batch_watch(depth=9, small_max=128)          # depth anew
        assert enabled() == 1 and records_equal(sim.download_encounters(), rec)
        # a non-NULL nb_set_block_steps keeps both
        sim.set_block_steps(eta=0.02, max_level=12)
        assert enabled() == 1 and sim.encounter_stats()["hits"] == st["hits"]
        # the setters that stay refused, as on any watched handle
        for call in (sim.set_block_batch, sim.set_block_batch6, sim.set_block_batch_mixed, lambda: sim.set_hermite_order(6),
                     lambda: sim.set_pass_precision("mixed"), lambda: sim.set_neighbor_scheme(radius=0.1)):
            error(call, 4)
        assert enabled() == 1
        sim.simulate(1)
        assert sim.block_batch_stats()["small_steps"] > 0
        # the watch off: the mode goes with it
        sim.set_encounter_watch(None)
        assert enabled() == 0
        error(sim.encounter_stats, 4, "encounter")
        sim.set_block_batch()                                      # ... and the unwatched mode is free again
        assert enabled() == 1
        error(lambda: sim.set_encounter_watch(radius=0.1), 4, "encounter")      # the pinned refusal: the watch off, a batched mode on
        error(lambda: sim.set_block_batch_watch(), 4, "nb_set_block_batch_watch", "nb_set_block_batch")      # another batched mode on
        sim.set_block_batch(None)
        # block steps off: both off
        sim.set_encounter_watch(radius=0.1)
        sim.set_block_batch_watch()
        sim.set_block_steps(None)
        assert enabled() == 0
        error(sim.encounter_stats, 4, "encounter")


def test_refusals():
    b0, v0 = E.pair300()
    who = "nb_set_block_batch_watch"
    with Simulation(300) as leap:                                      # not a Hermite handle
        error(lambda: leap.set_block_batch_watch(), 4, who, "nb_set_block_steps", "nb_set_encounter_watch")
    for prec in ("f32", "f64"):
        with hermite(300, prec) as sim:
            sim.init(b0, v0)
            sim.set_params(2.0 ** -4, 1.0)
            error(lambda: sim.set_block_batch_watch(), 4, who, "nb_set_block_steps")                  # block steps off
            sim.set_hermite_order(6)
            error(lambda: sim.set_block_batch_watch(), 4, who, "nb_set_hermite_order")               # an order-6 handle
            sim.set_hermite_order(4)
            sim.set_block_steps(max_level=4)
            error(lambda: sim.set_block_batch_watch(), 4, who, "nb_set_encounter_watch", "nb_set_block_batch ")      # the watch off
            if prec == "f64":
                sim.set_pass_precision("mixed")
                error(lambda: sim.set_block_batch_watch(), 4, who, "nb_set_pass_precision")         # a mixed pass
                sim.set_pass_guard(0.01)
                error(lambda: sim.set_block_batch_watch(), 4, who, "nb_set_pass_precision")         # a guarded pass
                sim.set_pass_precision("native")
            sim.set_block_batch()
            error(lambda: sim.set_block_batch_watch(), 4, who, "nb_set_block_batch")                  # another batched mode on
            error(lambda: sim.set_encounter_watch(radius=0.1), 4, "encounter")                        # pinned: a batched mode on
            sim.set_block_batch(None)
            sim.set_encounter_watch(radius=0.1)
            for call in (sim.set_block_batch, sim.set_block_batch6, sim.set_block_batch_mixed):      # pinned: the watch on
                error(call, 4, "encounter")
            # NB_ERR_INVALID names the function and the field
            L, cfg = sim._L, capi.nb_block_batch()
            for field, value, word in (("struct_size", 8, "struct_size"), ("depth", 1025, "depth"), ("small_max", 1025, "small_max"), ("flags", 1, "flags")):
                cfg.struct_size, cfg.depth, cfg.small_max, cfg.flags = 16, 0, capi.BLOCK_BATCH_SMALL_DEFAULT, 0
                setattr(cfg, field, value)
                assert L.nb_set_block_batch_watch(sim._h, C.byref(cfg)) == 1
                msg = L.nb_last_error(sim._h).decode()
                assert who in msg and word in msg, msg
            sim.set_block_batch_watch(small_max=1024)
            sim.simulate(1)
            assert sim.block_batch_stats()["small_steps"] > 0 and sim.encounter_stats()["passes"] == sim.block_stats()["block_steps"]
