"""The yardstick of the sequential-cycle diagnosis (diag_ext_model.py), on the
CPU oracle alone: records() counts `first` in the extended Filter order and
agrees with diag_model.records on the older bits, the cases reach every plugin
and make the order matter, the state a stream leaves changes the records, and
koordinator_amd.diagnosis reads the extended records.

Measured on the oracle (pods with first > 0 / with any != first), for reference:
  full(1003, 70)  FIT 4/0, XFIT 29/4, PTS 37/15, IPA 13/11, LA 70/55, NUMA 12/12, DEVICE 17/29;
                  38 of the 70 records differ after place_stream_ext places all 70
  resv            STATIC 40/0, FIT 23/8, XFIT 17/18, LA 39/40, NUMA 6/6, DEVICE 8/18, RESV 1/13
  resv8           RESV 5/23
"""
import os
import re

import numpy as np
import pytest

import diag_ext_model as X
import diag_model as M
from koordinator_amd import abi, diagnosis

ST = {"FIT": abi.ST_FIT_FAIL, "LA": abi.ST_LA_FAIL, "NUMA": abi.ST_NUMA_FAIL, "RESV": abi.ST_RESV_FAIL,
      "STATIC": abi.ST_STATIC_FAIL, "DEVICE": abi.ST_DEVICE_FAIL, "XFIT": abi.ST_XFIT_FAIL, "PTS": abi.ST_PTS_FAIL,
      "IPA": abi.ST_IPA_FAIL}
ALL = sum(ST.values())


def slot(bit):
    return bit.bit_length() - 1


def test_filter_order_ext_restricted_to_the_old_bits():
    assert [b for b in abi.FILTER_ORDER_EXT if b in abi.FILTER_ORDER] == list(abi.FILTER_ORDER)
    assert sorted(abi.FILTER_ORDER_EXT) == sorted(ST.values())
    o = abi.FILTER_ORDER_EXT
    assert o.index(abi.ST_XFIT_FAIL) == o.index(abi.ST_FIT_FAIL) + 1      # one plugin: adjacent, FIT first


def test_records_of_hand_written_status_rows():
    rows = [ST["FIT"] | ST["XFIT"], ST["PTS"] | ST["IPA"], ST["IPA"] | ST["LA"], ST["DEVICE"] | ST["RESV"], ALL, 0,
            ST["XFIT"] | ST["NUMA"], ST["NUMA"] | ST["DEVICE"]]
    r = X.records(np.array([rows], np.uint16))[0]
    first = {k: int(r["first"][slot(b)]) for k, b in ST.items()}
    anyc = {k: int(r["any"][slot(b)]) for k, b in ST.items()}
    assert first == {"FIT": 1, "PTS": 1, "IPA": 1, "DEVICE": 1, "STATIC": 1, "XFIT": 1, "NUMA": 1, "LA": 0, "RESV": 0}
    assert anyc == {"FIT": 2, "XFIT": 3, "PTS": 2, "IPA": 3, "LA": 2, "NUMA": 3, "DEVICE": 3, "RESV": 2, "STATIC": 1}
    assert r["feasible"] == 1 and r["feasible"] + r["first"].sum() == len(rows)
    assert not r["any"][9:].any() and not r["first"][9:].any()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_records_equal_the_base_records_on_base_status(name):
    m = M.case(name)
    st = np.stack([m.status[int(u)] for u in m.unplaced])
    assert X.records(st).tobytes() == M.records(st).tobytes()


@pytest.mark.parametrize("case", sorted(X.CASES))
def test_records_are_consistent(case):
    m = X.CASES[case]()
    assert (m.rec["feasible"] + m.rec["first"].sum(axis=1) == m.table.n).all()
    assert (m.rec["first"] <= m.rec["any"]).all()
    assert m.status.dtype == np.uint16 and m.status.shape == (len(m.pods), m.table.n)


def test_full_reaches_every_plugin_and_the_order_matters():
    m = X.full(*X.FULL_SHAPES[-1])
    for k in ("FIT", "XFIT", "PTS", "IPA", "LA", "NUMA", "DEVICE"):
        assert X.first_pods(m, ST[k]) > 0, k
    for k in ("XFIT", "PTS", "IPA", "LA", "NUMA", "DEVICE"):
        assert X.masked_pods(m, ST[k]) > 0, k
    # spread classes 2 and 4 carry a hard hostname constraint: the hostname-minimum pre-pass is exercised
    hard_host = [j for j in range(len(m.pods)) if m.ext["pts_n"][j] and m.ext["pts_class"][j] in (2, 4)]
    assert hard_host and any(m.rec["any"][j][slot(ST["PTS"])] > 0 for j in hard_host)


def test_full_stream_changes_the_records():
    m = X.full(*X.FULL_SHAPES[-1])
    assert (m.out >= 0).all()
    assert int((m.rec != m.rec_after).sum()) >= 10


def test_resv_cases_reach_the_reservation_paths():
    m = X.resv()
    assert (m.table["resv_dev_slot"] >= 0).any()          # reservations holding devices
    for k in ("STATIC", "FIT", "XFIT", "LA", "NUMA", "DEVICE", "RESV"):
        assert X.first_pods(m, ST[k]) > 0, k
    assert X.masked_pods(m, ST["RESV"]) > 0
    m8 = X.resv8()
    assert m8.table.resv_slots > abi.RESV_SLOTS           # the 8-slot rows
    assert X.first_pods(m8, ST["RESV"]) > 0


def test_plain_has_no_ext_bit():
    m = X.plain()
    assert m.ext is None and not (m.status & ~np.uint16(sum(abi.FILTER_ORDER))).any()
    assert m.rec.tobytes() == M.records(m.status).tobytes()


def test_diagnosis_reads_extended_records():
    rec = np.zeros(1, abi.DIAG_DTYPE)[0]
    for k, v in (("FIT", 3), ("XFIT", 2), ("PTS", 4), ("IPA", 1), ("DEVICE", 5)):
        rec["first"][slot(ST[k])] = v
        rec["any"][slot(ST[k])] = v
    rec["any"][slot(ST["LA"])] = 6            # always behind an earlier plugin: not a first failure
    assert diagnosis.unschedulable_plugins(rec) == {"NodeResourcesFit", "PodTopologySpread", "InterPodAffinity",
                                                    "DeviceShare"}
    assert diagnosis.summary(rec, 15) == (
        "0/15 nodes are available: 3 Insufficient resources, 2 Insufficient extended resources, "
        "4 node(s) didn't match pod topology spread constraints, "
        "1 node(s) didn't match pod affinity/anti-affinity rules, 5 Insufficient Devices.")


def test_diagnosis_of_an_old_record_is_unchanged():
    rec = np.zeros(1, abi.DIAG_DTYPE)[0]
    for b, k in zip(abi.FILTER_ORDER, range(1, 6)):
        rec["first"][slot(b)] = k
    rec["feasible"] = 2
    assert diagnosis.summary(rec, 17) == (
        "2/17 nodes are available: 1 node(s) didn't match the pod's node affinity/selector, taints or were "
        "unschedulable, 2 Insufficient resources, 3 node(s) usage exceed threshold, "
        "4 node(s) failed NodeNUMAResource, 5 node(s) failed Reservation.")
    assert diagnosis.unschedulable_plugins(rec) == {
        "NodeResourcesFit", "LoadAwareScheduling", "NodeNUMAResource", "Reservation", diagnosis.STATIC_PLUGINS}


def test_header_declares_both_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "koordhip.h")).read()
    for name in ("koordhip_diagnose_ext", "koordhip_node_status_ext"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in abi.EXPORTED_SYMBOLS
    assert re.search(r"#define\s+KOORDHIP_ABI_VERSION\s+15\b", src)
    tile = re.search(r"constexpr int DIAGX_PT = (\d+);",
                     open(os.path.join(root, "koordinator_amd", "csrc", "diag_ext.h")).read())
    assert tile and int(tile.group(1)) == abi.DIAG_EXT_POD_TILE     # the tile the GPU tiling test slices at
