"""The FitError reasons on the CPU: the model of reasons_model.py against the
reference's Filter rows (tests/golden/filter_reasons.json) and against the
oracle's status bits, the host side's message, and the condition the GPU
tests rest on: their inputs reach every reason the profile can produce."""
import numpy as np
import pytest

import oracle
import reasons_model as RM
from koordinator_amd import abi, diagnosis
from koordinator_amd.config import to_c_config

ROWS = RM.fixture_rows()


# ------------------------------------------------------------------ the fixture
def test_fixture_is_what_the_script_writes(tmp_path):
    import importlib.util
    import json
    import os
    import golden_cases as G
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_filter_reasons_golden.py")
    spec = importlib.util.spec_from_file_location("make_filter_reasons_golden", path)
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    want = {"numa_filter": mk.NUMA_FILTER, "numa_filter_amp": mk.NUMA_FILTER_AMP, "resv_filter": mk.RESV_FILTER,
            "resv_affinity": mk.RESV_AFFINITY_CASE}
    assert json.loads(json.dumps(want)) == G.load("filter_reasons.json")
    assert len(ROWS) == 12 + 7 + 4 + 1


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_model_reproduces_fixture_row(row):
    _, w, bit, prof, t, pod = row
    o = oracle.Oracle(to_c_config(prof), t)
    st = o.eval(pod, status=True, scores=False)["status"][0].astype(np.uint32)
    m = RM.resv_mask(o, pod[0], st & bit) if bit == abi.ST_RESV_FAIL else RM.masks(o, pod)[0]
    RM.check_fixture_row(w, bit, m[0])


def test_reason_texts_are_the_fixture_strings():
    for _, w, _, _, _, _ in ROWS:
        if w["code"] != "Success":
            assert w["reason"] in RM.SLOT_OF_TEXT or w["reason"] in diagnosis.REASON_TEXT.values(), w


# ------------------------------------------------------------------ the constants
def test_reason_groups_partition_the_slots():
    groups = list(abi.REASONS_OF_BIT.values())
    assert sum(groups) == (1 << abi.REASON_COUNT) - 1
    for a in range(len(groups)):
        for b in range(a):
            assert groups[a] & groups[b] == 0
    # the Filter order is the slot order: the first failing plugin is the group of the lowest set bit
    lows = [abi.REASONS_OF_BIT[b] & -abi.REASONS_OF_BIT[b] for b in abi.FILTER_ORDER]
    assert lows == sorted(lows)
    uu = [abi.REASON_STATIC, abi.REASON_NUMA_NO_TOPOLOGY, abi.REASON_NUMA_SMT_ALIGN, abi.REASON_NUMA_FULL_PCPUS_ONLY,
          abi.REASON_NUMA_NO_ZONES, abi.REASON_RESV_AFFINITY]
    assert abi.REASON_UNRESOLVABLE_MASK == sum(1 << r for r in uu)
    assert abi.REASON_ERROR_MASK == 1 << abi.REASON_NUMA_POD_ERROR
    assert not abi.REASONS_OF_BIT[abi.ST_FIT_FAIL] & (abi.REASON_UNRESOLVABLE_MASK | abi.REASON_ERROR_MASK)


def test_header_constants_match():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "koordhip.h")).read()
    defs = dict(re.findall(r"#define KOORDHIP_(REASON\w*)\s+(0x[0-9A-Fa-f]+|\d+)u?", src))
    for name in dir(abi):
        if name.startswith("REASON_") and isinstance(getattr(abi, name), int):
            assert int(defs[name], 0) == getattr(abi, name), name
    for bit, key in ((abi.ST_STATIC_FAIL, "STATIC"), (abi.ST_FIT_FAIL, "FIT"), (abi.ST_LA_FAIL, "LA"),
                     (abi.ST_NUMA_FAIL, "NUMA"), (abi.ST_RESV_FAIL, "RESV")):
        assert int(defs["REASONS_OF_" + key], 0) == abi.REASONS_OF_BIT[bit]


# ------------------------------------------------------------------ model vs oracle status
@pytest.mark.parametrize("name", RM.CURRENT_CASES)
def test_union_is_the_oracle_status(name):
    prof, table, pods = RM.current_case(name)
    o = oracle.Oracle(to_c_config(prof), table)
    st = o.eval(pods, status=True, scores=False)["status"].astype(np.uint32)
    m = RM.masks(o, pods)
    assert np.array_equal(abi.reasons_status(m), st)
    rec = RM.records(m)
    assert (rec["feasible"] + (abi.first_reasons(m) != 0).sum(axis=1) == table.n).all()
    # every plugin but NodeResourcesFit reports one reason
    for bit, group in abi.REASONS_OF_BIT.items():
        if bit != abi.ST_FIT_FAIL:
            g = m & np.uint32(group)
            assert ((g & (g - np.uint32(1))) == 0).all(), bit


@pytest.mark.parametrize("name", ["A", "C"])
def test_decision_state_union_is_the_oracle_status(name):
    m = RM.case(name)
    assert len(m.d.unplaced) and len(m.differ)
    for u in m.d.unplaced:
        assert np.array_equal(abi.reasons_status(m.mask[int(u)]), m.d.status[int(u)].astype(np.uint32)), u


# ------------------------------------------------------------------ coverage
def test_inputs_reach_every_reason():
    """A GPU test over inputs that never reach a slot shows nothing.  Each of
    the two large cases reaches every slot its profile and snapshot can
    produce; all slots a case can produce are reached by some case; and the
    four NodeResourcesFit terms of a cpu / memory / ephemeral-storage pod fail
    together on one node."""
    reached, possible = {}, {}
    for name in RM.CURRENT_CASES:
        prof, table, pods = RM.current_case(name)
        cfg = to_c_config(prof)
        m = RM.masks(oracle.Oracle(cfg, table), pods)
        reached[name] = int(np.bitwise_or.reduce(m, axis=None))
        possible[name] = RM.possible_slots(cfg, table)
        assert reached[name] & ~possible[name] == 0, name
    for name in ("base-1003-70", "numa-ext"):
        assert reached[name] == possible[name], (name, hex(reached[name] ^ possible[name]))
    assert sum(reached.values()) and np.bitwise_or.reduce(list(reached.values())) == \
        np.bitwise_or.reduce(list(possible.values()))
    assert np.bitwise_or.reduce(list(possible.values())) == (1 << abi.REASON_RESV_AFFINITY) - 1   # slots 0..16
    four = sum(1 << r for r in (abi.REASON_FIT_PODS, abi.REASON_FIT_CPU, abi.REASON_FIT_MEM, abi.REASON_FIT_EPH))
    prof, table, pods = RM.current_case("base-1003-70")
    m = RM.masks(oracle.Oracle(to_c_config(prof), table), pods)
    assert ((m & np.uint32(four)) == four).any()
    # the decision-state cases differ from their final states somewhere, in NodeResourcesFit and beyond it
    for name in ("A", "C"):
        c = RM.case(name)
        assert c.rec["first"][:, abi.REASON_FIT_CPU].any() and c.rec["first"][:, abi.REASON_LA_USAGE].any()
    assert RM.case("C").rec["any"][:, abi.REASON_NUMA_NO_TOPOLOGY:abi.REASON_NUMA_REQUIRED_POLICY + 1].any()


def test_reservation_snapshot_reaches_both_reservation_reasons():
    prof, table, pods = RM.resv_case()
    o = oracle.Oracle(to_c_config(prof), table)
    st = o.eval(pods, status=True, scores=False)["status"].astype(np.uint32)
    got = 0
    for p in range(len(pods)):
        m = RM.resv_mask(o, pods[p], st[p] & abi.ST_RESV_FAIL)
        got |= int(np.bitwise_or.reduce(m))
        if not pods["flags"][p] & abi.POD_RESV_AFFINITY:
            assert not (m & np.uint32(1 << abi.REASON_RESV_AFFINITY)).any()
    assert got == abi.REASONS_OF_BIT[abi.ST_RESV_FAIL]


# ------------------------------------------------------------------ the host side
def _rec(n, first, unresolvable=0):
    rec = np.zeros(1, abi.REASONS_DTYPE)[0]
    for r, k in first.items():
        rec["first"][r] = k
        rec["any"][r] = k
    rec["unresolvable"] = unresolvable
    return rec


def test_fit_error_message_sorts_reason_strings():
    rec = _rec(50000, {abi.REASON_FIT_CPU: 31872, abi.REASON_FIT_MEM: 9120, abi.REASON_NUMA_NO_TOPOLOGY: 6,
                       abi.REASON_STATIC: 9002}, unresolvable=9008)
    msg = diagnosis.fit_error_message(rec, 50000)
    assert msg == ("0/50000 nodes are available: 31872 Insufficient cpu, 6 node(s) CPU Topology not found, "
                   "9002 " + diagnosis.REASON_TEXT[abi.REASON_STATIC] + ", 9120 Insufficient memory.")
    # sorted as strings, not by count: "10 ..." sorts before "9 ..."
    rec = _rec(19, {abi.REASON_FIT_PODS: 9, abi.REASON_RESV_INSUFFICIENT: 10})
    assert diagnosis.fit_error_message(rec, 19) == ("0/19 nodes are available: 10 node(s) reservations insufficient "
                                                    "resources, 9 Too many pods.")


def test_fit_error_message_multi_reason_fit():
    """A node short of cpu and memory counts under both strings, as upstream's per-reason histogram does."""
    m = np.array([[(1 << abi.REASON_FIT_CPU) | (1 << abi.REASON_FIT_MEM), 1 << abi.REASON_FIT_CPU,
                   (1 << abi.REASON_FIT_MEM) | (1 << abi.REASON_NUMA_NO_TOPOLOGY)]], np.uint32)
    rec = RM.records(m)[0]
    assert rec["first"][abi.REASON_FIT_CPU] == 2 and rec["first"][abi.REASON_FIT_MEM] == 2
    assert rec["first"][abi.REASON_NUMA_NO_TOPOLOGY] == 0 and rec["any"][abi.REASON_NUMA_NO_TOPOLOGY] == 1
    assert diagnosis.fit_error_message(rec, 3) == "0/3 nodes are available: 2 Insufficient cpu, 2 Insufficient memory."
    assert diagnosis.preemption_might_help(rec, 3)


def test_fit_error_message_all_feasible_and_preemption():
    rec = np.zeros(1, abi.REASONS_DTYPE)[0]
    rec["feasible"] = 7
    assert diagnosis.fit_error_message(rec, 7) == "0/7 nodes are available: ."
    assert not diagnosis.preemption_might_help(rec, 7)
    # every failing node is unresolvable: PostFilter has nothing to try
    m = np.array([[1 << abi.REASON_STATIC, (1 << abi.REASON_STATIC) | (1 << abi.REASON_FIT_CPU),
                   1 << abi.REASON_NUMA_SMT_ALIGN, 0]], np.uint32)
    rec = RM.records(m)[0]
    assert rec["unresolvable"] == 3 and rec["feasible"] == 1
    assert not diagnosis.preemption_might_help(rec, 4)
    # ... and a Fit failure ahead of an unresolvable NUMA reason is resolvable (the first plugin decides)
    m = np.array([[(1 << abi.REASON_FIT_CPU) | (1 << abi.REASON_NUMA_SMT_ALIGN)]], np.uint32)
    rec = RM.records(m)[0]
    assert rec["unresolvable"] == 0 and diagnosis.preemption_might_help(rec, 1)


def test_symbols_are_declared():
    lib = abi.load_library()
    for name in ("koordhip_diagnose_reasons", "koordhip_node_reasons", "koordhip_fetch_reasons",
                 "koordhip_fetch_node_reasons"):
        assert hasattr(lib, name) and name in abi.EXPORTED_SYMBOLS and name in abi.ADDITIVE_SYMBOLS
