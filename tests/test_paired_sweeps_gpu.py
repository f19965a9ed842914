"""GPU tests of the paired sweeps of the wave-granular symmetric pass (nb_force_symw_pairs, kernels/symmetric.hip.h).

Two consecutive whole sweeps that both keep traveler sums run together: the lane holds one traveler of each, packed, and their
sums as one dword per traveler and component, so a traveler-step costs 7 lane moves instead of 10.  The plan, the table and the layers are
those of the single-sweep kernel (nb_force_symw<NG, 1>, still there behind NB_FLAG_SINGLE_SWEEPS); every per-pair product is
the same, only the order of the additions differs.  Checked here, for the default plan at N = 65,536 and the headline 262,144
and for the pinned 16- and 8-resident forms at 8,192, 12,289 (ragged: sweeps over the short block pair too) and 20,001:
one step against the fp64 oracle, the momentum of the pair sums, two handles, a 16-step graph replay against 16 single steps,
and (queue on, N >= 131,072) two runs -- all byte for byte -- plus the single-sweep arm on the same plan.
"""
import numpy as np
import pytest

from oracle import oracle
from nbody3d_amd import Simulation, capi, ic

pytestmark = pytest.mark.gpu

TOL_ACC = 2e-5          # tests/test_sym_gpu.py

# (the pinned forms cut these small systems in units of 2 or 8 rotation steps, so only some of their sweeps are whole -- tools/paired_share.py:
# none at 8,192, 29 .. 69 % at 12,289 and 20,001; with whole sweeps, the last two arms, most of them pair, Z's among them)
W = capi.NB_FLAG_WHOLE_SWEEPS
CASES = [(0, 65536, 0), (0, 262144, 0), (716013, 8192, 0), (716013, 12289, 0), (716013, 20001, 0), (708013, 8192, 0), (708013, 12289, 0), (708013, 20001, 0),
         (716013, 12289, W), (708013, 20001, W)]


def bodies_of(n):
    return ic.plummer(n, seed=n) if n % 2 == 0 else ic.uniform_cube(n, seed=n)


def one_step(b, v, **kw):
    with Simulation(b.shape[0], **kw) as s:
        s.init(b, v)
        s.simulate(1, 1e-3, 1.0)
        return s.read(bodies=False, vel=False)[2], s.variant


def oracle_rows(b, n):
    """(row indices, fp64 accelerations of those rows): every row up to 65,536 bodies; above, 64 blocks of 256 consecutive rows spread
    evenly over the system, the first and the last rows among them (the whole fp64 sum of 262,144 bodies is a minute of CPU)."""
    if n <= 65536:
        return np.arange(n), oracle.accel_f64(b, 1.0)
    starts = np.linspace(0, n - 256, 64).astype(np.int64)
    rows = np.concatenate([np.arange(s, s + 256) for s in starts])
    return rows, np.concatenate([oracle.accel_f64(b, 1.0, i0=int(s), i1=int(s) + 256) for s in starts])


@pytest.mark.parametrize("variant,n,flags", CASES)
def test_one_step_against_the_fp64_oracle_and_the_momentum_of_the_pair_sums(variant, n, flags):
    b, v = bodies_of(n)
    acc, name = one_step(b, v, force_variant=variant, flags=flags)
    assert "symw_ipl%d_j1" % (8 if variant == 708013 else 16) in name, name
    rows, ref = oracle_rows(b, n)
    err = np.abs(acc[rows, :3] - ref[:, :3]).max() / np.abs(ref[:, :3]).max()
    f = b[:, 3:4].astype(np.float64) * acc[:, :3].astype(np.float64)
    mom = (np.abs(f.sum(0)) / np.abs(f).sum(0)).max()
    print("%s N=%d: worst error %.3g of the largest acceleration, momentum of the pair sums %.3g of the sum of magnitudes" % (name, n, err, mom))
    assert err < TOL_ACC, name
    assert mom < 1e-6, name                      # every pair from both sides: the pair sums cancel
    assert not acc[:, 3].any()
    # the single-sweep kernel on the same plan: same pairs, same products, another order of additions
    single, sname = one_step(b, v, force_variant=variant, flags=flags | capi.NB_FLAG_SINGLE_SWEEPS)
    assert sname == name
    assert np.abs(acc[:, :3] - single[:, :3]).max() < 2e-6 * np.abs(ref[:, :3]).max(), name


@pytest.mark.parametrize("variant,n,flags", CASES)
def test_two_handles_graph_replay_and_repeated_runs_give_the_same_bytes(variant, n, flags):
    b, v = bodies_of(n)
    kw = dict(force_variant=variant, flags=flags)
    with Simulation(n, **kw) as a, Simulation(n, **kw) as c:
        a.init(b, v)
        c.init(b, v)
        a.simulate(1, 1e-3, 1.0)
        c.simulate(1, 1e-3, 1.0)
        a1, c1 = a.read(bodies=False, vel=False)[2], c.read(bodies=False, vel=False)[2]
        assert a1.tobytes() == c1.tobytes(), a.variant                   # two handles
        a.simulate(16, 1e-3, 1.0)                                        # one call: a captured graph, replayed
        for _ in range(16):
            c.step(1e-3, 1.0)
        for x, y in zip(a.read(), c.read()):
            assert x.tobytes() == y.tobytes(), a.variant
        name = a.variant
    if n >= 131072:
        q = capi.plan_query(n, force_variant=variant, flags=flags)
        assert q["ups"] == 1 and len(q["pieces"]) > 1000, name            # the queue is on: who draws a piece must not show
        again, _ = one_step(b, v, **kw)
        assert again.tobytes() == a1.tobytes(), name
