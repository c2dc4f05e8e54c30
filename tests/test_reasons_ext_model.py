"""The yardstick of koordhip_diagnose_reasons_ext (reasons_ext_model.py) checked
on the CPU against the oracle: the masks' union is Oracle.eval_ext's status on
every (pod, node) of every case, the directed table's hand-written masks, the
record invariants and their ties to diag_ext_model's records, the constants
against the header, the message format, and that the cases reach every new
slot."""
import os
import re

import numpy as np
import pytest

import diag_ext_model as X
import reasons_ext_model as XM
from koordinator_amd import abi, diagnosis
from koordinator_amd.deviceshare import XRES

OF = abi.REASONS_OF_BIT_EXT
NEW_BITS = (abi.ST_XFIT_FAIL, abi.ST_DEVICE_FAIL, abi.ST_PTS_FAIL, abi.ST_IPA_FAIL)


def slots_of(group: int):
    return [r for r in range(abi.REASON_SLOTS) if (group >> r) & 1]


# ------------------------------------------------------------------ model vs oracle status
@pytest.mark.parametrize("name", XM.CASES)
def test_union_is_the_oracle_status(name):
    m = XM.case(name)
    st = m.x.status.astype(np.uint32)           # (on the resv cases: diag_ext_model's RESV convention, koordhip.h)
    got = abi.reasons_status_ext(m.mask)
    # Fit / NUMA on the restored rows of a Reservation snapshot have no model: their groups are left out
    loose = np.uint32((abi.ST_FIT_FAIL | abi.ST_NUMA_FAIL) if m.loose else 0)
    assert m.loose in (0, XM.RESTORED_ROW_GROUPS) and not (m.mask & np.uint32(m.loose)).any()
    assert np.array_equal(got & ~loose, st & ~loose)
    assert bool(m.loose) == name.startswith("resv")


@pytest.mark.parametrize("name", ["full-1003x70"])
def test_union_is_the_oracle_status_after_the_stream(name):
    m = XM.case(name)
    assert np.array_equal(abi.reasons_status_ext(m.mask_after), m.x.status_after.astype(np.uint32))
    assert int((m.rec_after != m.rec).sum()) >= 10      # counts move: nothing may be cached across calls


# ------------------------------------------------------------------ the directed literals
def test_directed_masks_are_the_hand_written_ones():
    m = XM.case("directed")
    assert m.mask.shape == (XM.D_PODS, XM.D_N)
    for p, want in XM.D_WANT.items():
        assert [hex(int(v)) for v in m.mask[p]] == [hex(v) for v in want], p
    n = XM.D_N
    for p, helps in XM.D_PREEMPTION_HELPS.items():
        assert diagnosis.preemption_might_help(m.rec[p], n) == helps, p
    # every scalar alone, three together, Fit and XFit together
    alone = [int(m.mask[0][j]) for j in range(abi.NXRES)]
    assert alone == [1 << (abi.REASON_FIT_X0 + j) for j in range(abi.NXRES)]
    assert bin(int(m.mask[0][8])).count("1") == 3
    assert int(m.mask[0][9]) & OF[abi.ST_FIT_FAIL] and int(m.mask[0][9]) & OF[abi.ST_XFIT_FAIL]
    r = m.rec[0]
    assert r["first"][abi.REASON_FIT_CPU] == 2 and r["first"][abi.REASON_FIT_X0 + 2] == 2    # one group: both counted
    # the UU-only pods: every failing node under one UnschedulableAndUnresolvable reason
    assert m.rec[2]["unresolvable"] == 2 == m.rec[2]["first"][abi.REASON_PTS_MISSING_LABEL]
    assert m.rec[4]["unresolvable"] == 8 == m.rec[4]["first"][abi.REASON_IPA_AFFINITY]
    # any != first: PTS / IPA behind NodeResourcesFit
    assert m.rec[1]["any"][abi.REASON_PTS_SKEW] == m.rec[1]["first"][abi.REASON_PTS_SKEW] + 1
    assert m.rec[3]["any"][abi.REASON_IPA_ANTI] == 1 and m.rec[3]["first"][abi.REASON_IPA_ANTI] == 0


# ------------------------------------------------------------------ record invariants
@pytest.mark.parametrize("name", XM.CASES)
def test_record_invariants(name):
    m = XM.case(name)
    n = m.x.table.n
    first = abi.first_reasons_ext(m.mask)
    if not m.loose:
        assert (m.rec["feasible"] + (first != 0).sum(axis=1) == n).all()
        assert np.array_equal(m.rec["feasible"], m.x.rec["feasible"])
    for b in (abi.ST_PTS_FAIL, abi.ST_IPA_FAIL, abi.ST_DEVICE_FAIL):
        g = m.mask & np.uint32(OF[b])
        assert ((g & (g - np.uint32(1))) == 0).all(), b            # one reason per failing node
    diag = m.x.rec
    for b in NEW_BITS:
        slots, k = slots_of(OF[b]), b.bit_length() - 1
        if b == abi.ST_XFIT_FAIL:                                   # a node counts once per failing scalar here
            assert (m.rec["any"][:, slots].max(axis=1) <= diag["any"][:, k]).all()
            assert (diag["any"][:, k] <= m.rec["any"][:, slots].sum(axis=1)).all()
        else:
            assert np.array_equal(m.rec["any"][:, slots].sum(axis=1), diag["any"][:, k]), b
            if not m.loose:
                assert np.array_equal(m.rec["first"][:, slots].sum(axis=1), diag["first"][:, k]), b
    if not m.loose:
        # first[FIT] + first[XFIT] of the diag record = the nodes whose first group is NodeResourcesFit
        fit_first = ((first & np.uint32(XM.FIT_ALL)) != 0).sum(axis=1)
        kf, kx = abi.ST_FIT_FAIL.bit_length() - 1, abi.ST_XFIT_FAIL.bit_length() - 1
        assert np.array_equal(fit_first, diag["first"][:, kf] + diag["first"][:, kx])
        for b in (abi.ST_STATIC_FAIL, abi.ST_LA_FAIL, abi.ST_NUMA_FAIL, abi.ST_RESV_FAIL):
            slots, k = slots_of(OF[b]), b.bit_length() - 1
            assert np.array_equal(m.rec["first"][:, slots].sum(axis=1), diag["first"][:, k]), b
    uu = ((first & np.uint32(abi.REASON_EXT_UNRESOLVABLE_MASK)) != 0).sum(axis=1)
    assert np.array_equal(m.rec["unresolvable"], uu)


def test_plain_case_has_no_ext_slot_and_the_old_first_rule():
    m = XM.case("plain")
    assert not (m.mask >> np.uint32(abi.REASON_COUNT)).any()
    assert np.array_equal(abi.first_reasons_ext(m.mask), abi.first_reasons(m.mask))
    assert np.array_equal(abi.reasons_status_ext(m.mask), abi.reasons_status(m.mask))


# ------------------------------------------------------------------ constants
def test_constants_match_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "koordhip.h")).read()
    defs = {k: int(v, 0) for k, v in re.findall(r"#define KOORDHIP_(REASON\w*)\s+(0x[0-9A-Fa-f]+|\d+)u?", src)}
    assert defs["REASON_FIT_X0"] == abi.REASON_FIT_X0 == 19 == abi.REASON_COUNT
    assert abi.REASON_FIT_X0 + abi.NXRES == abi.REASON_DEVICE_INSUFFICIENT == 27
    want = {"REASON_DEVICE_INSUFFICIENT": 27, "REASON_PTS_MISSING_LABEL": 28, "REASON_PTS_SKEW": 29,
            "REASON_IPA_AFFINITY": 30, "REASON_IPA_ANTI": 31, "REASON_EXT_COUNT": 32,
            "REASON_EXT_UNRESOLVABLE_MASK": 0x50029C01}
    for k, v in want.items():
        assert defs[k] == v == getattr(abi, k), k
    groups = {"XFIT": (abi.ST_XFIT_FAIL, 0x07F80000), "DEVICE": (abi.ST_DEVICE_FAIL, 0x08000000),
              "PTS": (abi.ST_PTS_FAIL, 0x30000000), "IPA": (abi.ST_IPA_FAIL, 0xC0000000)}
    for k, (b, v) in groups.items():
        assert defs["REASONS_OF_" + k] == v == OF[b], k
    # the older constants and helpers are where they were
    assert defs["REASON_COUNT"] == 19 and defs["REASON_UNRESOLVABLE_MASK"] == 0x00029C01 == abi.REASON_UNRESOLVABLE_MASK
    assert len(abi.REASONS_OF_BIT) == 5 and sum(abi.REASONS_OF_BIT.values()) == 2**19 - 1
    assert len(OF) == 9 and sum(OF.values()) == 2**32 - 1
    assert all(OF[b] == g for b, g in abi.REASONS_OF_BIT.items())
    assert abi.REASON_EXT_UNRESOLVABLE_MASK == (abi.REASON_UNRESOLVABLE_MASK | 1 << abi.REASON_PTS_MISSING_LABEL
                                                | 1 << abi.REASON_IPA_AFFINITY)
    for name in ("koordhip_diagnose_reasons_ext", "koordhip_node_reasons_ext"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in abi.EXPORTED_SYMBOLS and name in abi.ADDITIVE_SYMBOLS


def test_first_reasons_ext_walks_the_filter_order():
    one = lambda r: np.uint32(1 << r)
    la, pts, ipa, dev = one(abi.REASON_LA_USAGE), one(abi.REASON_PTS_SKEW), one(abi.REASON_IPA_ANTI), \
        one(abi.REASON_DEVICE_INSUFFICIENT)
    x3, cpu, numa, resv = one(abi.REASON_FIT_X0 + 3), one(abi.REASON_FIT_CPU), one(abi.REASON_NUMA_CPUS), \
        one(abi.REASON_RESV_INSUFFICIENT)
    f = lambda m: int(abi.first_reasons_ext(np.uint32(m)))
    assert f(la | pts) == pts and f(la | ipa) == ipa and f(pts | ipa) == pts       # slot order is not Filter order
    assert f(x3 | la | dev) == x3 and f(cpu | x3 | pts) == cpu | x3                # Fit and XFit: one group
    assert f(numa | dev | resv) == numa and f(dev | resv) == dev and f(la | numa) == la
    assert f(one(abi.REASON_STATIC) | cpu | x3) == 1 and f(0) == 0
    assert int(abi.reasons_status_ext(cpu | x3 | pts | dev)) == (abi.ST_FIT_FAIL | abi.ST_XFIT_FAIL | abi.ST_PTS_FAIL
                                                                  | abi.ST_DEVICE_FAIL)


# ------------------------------------------------------------------ message format
def test_fit_error_message_prints_the_ext_slots():
    rec = np.zeros(1, abi.REASONS_DTYPE)[0]
    rec["first"][abi.REASON_FIT_CPU] = 3
    rec["first"][abi.REASON_FIT_X0 + 4] = 2
    rec["first"][abi.REASON_DEVICE_INSUFFICIENT] = 7
    rec["first"][abi.REASON_PTS_MISSING_LABEL] = 1
    rec["first"][abi.REASON_PTS_SKEW] = 4
    rec["first"][abi.REASON_IPA_AFFINITY] = 5
    rec["first"][abi.REASON_IPA_ANTI] = 6
    assert diagnosis.fit_error_message(rec, 28) == (
        "0/28 nodes are available: "
        "1 node(s) didn't match pod topology spread constraints (missing required label), "
        "2 Insufficient koordinator.sh/gpu-memory, 3 Insufficient cpu, "
        "4 node(s) didn't match pod topology spread constraints, 5 node(s) didn't match pod affinity rules, "
        "6 node(s) didn't match pod anti-affinity rules, 7 Insufficient Devices.")
    assert [diagnosis.reason_text(abi.REASON_FIT_X0 + j) for j in range(abi.NXRES)] == ["Insufficient " + x for x in XRES]
    assert len(diagnosis.REASON_TEXT) == abi.REASON_COUNT
    old = np.zeros(1, abi.REASONS_DTYPE)[0]
    old["first"][abi.REASON_FIT_MEM] = 2
    assert diagnosis.fit_error_message(old, 2) == "0/2 nodes are available: 2 Insufficient memory."


def test_fit_error_message_of_the_big_case():
    """Some pod's message names a device scalar and both spread reasons."""
    m = XM.case("full-1003x70")
    n = m.x.table.n
    msgs = [diagnosis.fit_error_message(r, n) for r in m.rec]
    label = diagnosis.REASON_TEXT_EXT[abi.REASON_PTS_MISSING_LABEL]
    skew = " " + diagnosis.REASON_TEXT_EXT[abi.REASON_PTS_SKEW] + ","
    hits = [s for s in msgs if any("Insufficient " + x in s for x in XRES) and label in s and (skew in s or
            s.endswith(skew[:-1] + "."))]
    assert hits, msgs[:3]


# ------------------------------------------------------------------ coverage of the cases
def test_cases_reach_every_new_slot():
    first = np.zeros(abi.REASON_SLOTS, np.int64)
    masked = {b: 0 for b in NEW_BITS}
    for name in XM.CASES:
        m = XM.case(name)
        first += (m.rec["first"] > 0).sum(axis=0)
        for b in NEW_BITS:
            s = slots_of(OF[b])
            masked[b] += int((m.rec["any"][:, s].sum(axis=1) != m.rec["first"][:, s].sum(axis=1)).sum())
    for r in range(abi.REASON_FIT_X0, abi.REASON_EXT_COUNT):
        assert first[r] > 0, r
    assert all(v > 0 for v in masked.values()), masked
    # the restored-scalar path: some node's reservation holds extended scalars the pods ask for
    t = X.resv().table
    assert t.has_resv_dev and t["resv_xalloc"].any() and (t["resv_dev_slot"] >= 0).any()
    # ... and on resv-scalars the restored terms give another answer than the node's own scalars would
    assert XM.restored_differs(XM.case("resv-scalars")) >= 10
