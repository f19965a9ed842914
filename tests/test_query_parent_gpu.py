"""The six queries, their *_shape getters and the nb_multi_* wrappers against the record of the commit before they were given one
prologue, one staging path and one batch rule (tests/golden/query_parent.json, recorded by tests/golden/measure_query_parent.py;
tests/query_parent.py says what it holds): the launch shapes equal, every failure's return code and text equal byte for byte, every
answer on fresh handles of 771 bodies equal bit for bit (by SHA-256)."""
import pytest

import query_parent as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def record():
    return P.load()


def same_device(record):
    cu = P.compute_units()
    if cu != record["compute_units"]:
        pytest.skip("the record is of a device with %d compute units, this one has %d: the launch-shape rule, and with it the cut that "
                    "the float bits follow, depends on the count" % (record["compute_units"], cu))


def test_the_shape_getters_give_the_recorded_shapes(record):
    same_device(record)
    got = P.all_shapes()
    assert sorted(got) == sorted(record["shapes"])
    bad = ["%s %s: %s, recorded %s" % (h, k, got[h].get(k), want) for h in sorted(got) for k, want in sorted(record["shapes"][h].items())
           if got[h].get(k) != want]
    assert not bad and all(len(got[h]) == len(record["shapes"][h]) for h in got), "\n".join(bad[:20])


def test_every_failure_keeps_its_code_and_its_text(record):
    got = P.all_messages()
    assert sorted(got) == sorted(record["messages"])
    bad = ["%s: %r, recorded %r" % (k, got[k], want) for k, want in sorted(record["messages"].items()) if got[k] != want]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("precision,hermite", P.BITS_HANDLES, ids=[P.handle_id(P.BITS_N, p, h) for p, h in P.BITS_HANDLES])
def test_fresh_handles_answer_the_recorded_bits(record, precision, hermite):
    same_device(record)
    want = record["bits"][P.handle_id(P.BITS_N, precision, hermite)]
    got = P.bits_of(precision, hermite)
    assert sorted(got) == sorted(want)
    bad = ["%s: %s, recorded %s" % (k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]]
    assert not bad, "\n".join(bad)
