"""The yardstick of the unschedulable-pod diagnosis (diag_model.py), on the CPU
oracle alone: the inputs really separate the state a pod was decided on from
the state the stream ends in, the expected records are consistent, and
koordinator_amd.diagnosis reads records the way the reference host needs."""
import numpy as np
import pytest

import diag_model as M
from koordinator_amd import abi, diagnosis


def slot(bit):
    return bit.bit_length() - 1


@pytest.mark.parametrize("name,unplaced,differ", [("A", 283, 34), ("B", 121, 1), ("C", 208, 59)])
def test_cases_have_the_measured_shape(name, unplaced, differ):
    m = M.case(name)
    assert len(m.unplaced) == unplaced
    assert len(m.differ) == differ
    # interleaved: unplaced pods are followed by later commits
    later = [u for u in m.unplaced if (m.out[u + 1:] >= 0).any()]
    assert len(later) >= unplaced - 1


@pytest.mark.parametrize("name", ["A", "C"])
def test_decision_state_differs_from_final_state(name):
    """An implementation that does not rewind the stream cannot pass: at least
    10 unplaced pods have another record on the final state."""
    assert len(M.case(name).differ) >= 10


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_records_are_consistent(name):
    m = M.case(name)
    n = m.table.n
    for u in m.unplaced:
        r = m.rec[u]
        if m.out[u] == abi.UNSCHEDULABLE:
            assert r["feasible"] == 0
            assert r["first"].sum() == n
        assert r["feasible"] + r["first"].sum() == n
        assert (r["first"] <= r["any"]).all()
    placed = np.flatnonzero(m.out >= 0)
    assert not m.rec[placed]["any"].any() and not m.rec[placed]["feasible"].any()


def test_case_c_covers_every_fit_la_numa_combination():
    m = M.case("C")
    seen = set()
    for st in m.status.values():
        seen |= set(np.unique(st).tolist())
    assert seen >= set(range(1, 8))     # every non-empty combination of the three bits


def test_records_of_status_bytes():
    st = np.array([[0, 1, 3, 16, 17, 6, 8, 12, 2]], np.uint8)
    r = M.records(st)[0]
    assert r["feasible"] == 1
    assert r["any"][:5].tolist() == [3, 3, 2, 2, 2]       # FIT, LA, NUMA, RESV, STATIC
    assert r["first"][:5].tolist() == [2, 2, 1, 1, 2]
    assert r["feasible"] + r["first"].sum() == st.size


def test_unschedulable_plugins_and_summary():
    rec = np.zeros(1, abi.DIAG_DTYPE)[0]
    rec["first"][slot(abi.ST_FIT_FAIL)] = 7
    rec["first"][slot(abi.ST_STATIC_FAIL)] = 2
    rec["any"][slot(abi.ST_FIT_FAIL)] = 9
    rec["any"][slot(abi.ST_STATIC_FAIL)] = 2
    rec["any"][slot(abi.ST_LA_FAIL)] = 4            # always behind an earlier plugin: not a first failure
    assert diagnosis.unschedulable_plugins(rec) == {"NodeResourcesFit", diagnosis.STATIC_PLUGINS}
    s = diagnosis.summary(rec, 9)
    assert s.startswith("0/9 nodes are available: ")
    assert s.index("2 ") < s.index("7 ")            # Filter order: the static trio first
    assert "usage exceed" not in s
    full = np.zeros(1, abi.DIAG_DTYPE)[0]
    for b, k in zip(abi.FILTER_ORDER, range(1, 6)):
        full["first"][slot(b)] = k
    assert diagnosis.unschedulable_plugins(full) == {
        "NodeResourcesFit", "LoadAwareScheduling", "NodeNUMAResource", "Reservation", diagnosis.STATIC_PLUGINS}
    ok = np.zeros(1, abi.DIAG_DTYPE)[0]
    ok["feasible"] = 5
    assert diagnosis.unschedulable_plugins(ok) == set()
    assert diagnosis.summary(ok, 5) == "5/5 nodes are available."
