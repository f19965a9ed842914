"""nb_step on Hermite handles of orders 4 and 6, plain and with block steps, against the record of the commit before the two orders
were given one host path (tests/golden/hermite_parent.json, recorded by tests/golden/measure_hermite_parent.py;
tests/hermite_parent.py says what it holds): every downloaded array equal bit for bit (by SHA-256) after every segment, block_stats(),
the variant name and the shape report equal, and the failure of a step without nb_set_params equal in code and text on all four
step paths."""
import pytest

import hermite_parent as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def record():
    return P.load()


def same_device(record):
    cu = P.compute_units()
    if cu != record["compute_units"]:
        pytest.skip("the record is of a device with %d compute units, this one has %d: the launch rule of the full and of the gathered "
                    "pass, and with it the cut that the float bits follow, depends on the count" % (record["compute_units"], cu))


def test_the_record_holds_every_case(record):
    assert sorted(record["bits"]) == sorted(P.case_id(c) for c in P.CASES)
    assert sorted(record["messages"]) == sorted(P.message_id(b, o) for b, o in P.MSG_PATHS)
    assert record["bits"][P.case_id(P.SPLIT)] == record["bits"][P.case_id(P.SPLIT_OF)]      # two calls of simulate(1) = one of simulate(2)


@pytest.mark.parametrize("case", P.CASES, ids=[P.case_id(c) for c in P.CASES])
def test_steps_give_the_recorded_bits(record, case):
    same_device(record)
    want = record["bits"][P.case_id(case)]
    got = P.run(case)
    assert len(got) == len(want)
    bad = []
    for i, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w) and sorted(g["arrays"]) == sorted(w["arrays"]), (i, g, w)
        bad += ["segment %d %s: %s, recorded %s" % (i, k, g[k], w[k]) for k in ("variant", "shape", "stats") if g[k] != w[k]]
        bad += ["segment %d %s: %s, recorded %s" % (i, k, g["arrays"][k], w["arrays"][k]) for k in sorted(w["arrays"]) if g["arrays"][k] != w["arrays"][k]]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("block,order", P.MSG_PATHS, ids=[P.message_id(b, o) for b, o in P.MSG_PATHS])
def test_a_step_without_params_keeps_its_code_and_its_text(record, block, order):
    want = record["messages"][P.message_id(block, order)]
    got = list(P.message_of(block, order))
    assert got == want, "%r, recorded %r" % (got, want)
