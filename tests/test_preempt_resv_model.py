"""The Reservation mode of the preemption dry run without a GPU: the model
(preempt_resv_model.py) against the reference's own tables
(golden/resv_preemptible_cases.json), against the oracle's Reservation Filter
where nothing is preemptible, on hand-worked dry runs, the coverage the
generated cases must have, the host records and the ABI constants."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from koordinator_amd import abi, k8s, preemption as pre, reservation as rsv, synth
from koordinator_amd.config import shipped_profile, to_c_config
from koordinator_amd.marshal import MarshalError

import preempt_model as M
import preempt_resv_model as V

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resv_preemptible_cases.json")))
NAMES = ("cpu", "memory")
REASON = {None: None, "ErrReasonPreemptionFailed": "preemption_failed",
          "ErrReasonReservationInsufficientResources": "insufficient"}


def amounts(rl):
    return [int((rl or {}).get(NAMES[k], 0)) if k < 2 else 0 for k in range(abi.NRES)]


def golden_state(row) -> V.PreState:
    st = V.PreState()
    st.pn = amounts(row["preemptible"])
    if row["in_rr"] is not None:
        st.pr[0] = amounts(row["in_rr"])       # the rows' one reservation UID is slot 0
    return st


# ---------------------------------------------------- 1. the reference's rows
@pytest.mark.parametrize("row", GOLDEN["filter"], ids=lambda r: r["source"])
def test_filter_with_reservations_rows(row):
    g = GOLDEN["node"]
    node = {"alloc": [g["alloc_cpu"], g["alloc_memory"], 0, 0, 0], "alloc_pods": g["alloc_pods"], "npods": g["pods"]}
    pod = {"req": amounts(row["pod"]), "has_req": True, "scalar": [False, False],
           "keys": [n in row["pod"] for n in NAMES], "affinity": False}
    matched = []
    r = row["reservation"]
    if r is not None:
        names = r["resource_names"] if r["resource_names"] is not None else list(r["allocatable"])
        matched = [(0, {"policy": V.POLICY_NAMES[r["policy"]], "keys": [n in names for n in NAMES],
                        "ra": amounts(r["allocatable"])[:2], "rd": amounts(r["allocated"])[:2]})]
    nrs = {"nmatch": len(matched), "pod_requested": amounts(row["pod_requested"]),
           "r_allocated": amounts(row["r_allocated"])[:2]}
    assert V.filter_with_reservations(pod, node, nrs, matched, golden_state(row)) == REASON[row["want"]], row["name"]


@pytest.mark.parametrize("op", ["add", "remove"])
def test_prefilter_extension_rows(op):
    assert len(GOLDEN[op]) == 3
    for row in GOLDEN[op]:
        st = golden_state(row["state"])
        req = amounts({"cpu": row["pod_cpu"]})
        (V.add_pod if op == "add" else V.remove_pod)(st, req, 0 if row["bound"] else -1)
        want = golden_state(row["want"])
        assert st.pn == want.pn, row["name"]
        assert {q: v for q, v in st.pr.items() if V.present(v)} == {q: v for q, v in want.pr.items() if V.present(v)}, row["name"]


def test_the_golden_file_is_what_its_maker_writes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_resv_preemptible_golden", os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "golden", "make_resv_preemptible_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    assert (GOLDEN["filter"], GOLDEN["add"], GOLDEN["remove"]) == (mk.FILTER, mk.ADD, mk.REMOVE)
    assert len(mk.FILTER) == 12 and sum(r["reservation"] is None for r in mk.FILTER) == 4


# ------------------------------- 2. nothing preemptible: the oracle's verdict
@pytest.mark.parametrize("slots", [1, 4])
def test_without_state_it_is_the_oracles_reservation_filter(slots):
    prof = shipped_profile(reservation=True)
    table = synth.add_reservations(synth.make_cluster(synth.ClusterSpec(150, seed=5), prof), V.resv_spec(slots), 5)
    pods = synth.make_pods(synth.StreamSpec(24, be_frac=0.2, resv_match_frac=0.7, resv_groups=V.GROUPS,
                                            resv_affinity_frac=0.3, seed=6), prof)
    policies = {(int(f) >> abi.RESV_POLICY_SHIFT) & 3 for q in range(slots)
                for f in table[V.slot_col("resv_flags", q)] if int(f) & abi.RESV_PRESENT}
    assert policies == {abi.RESV_POLICY_DEFAULT, abi.RESV_POLICY_ALIGNED, abi.RESV_POLICY_RESTRICTED}
    st = oracle.Oracle(to_c_config(prof), table).eval(pods, status=True, scores=False)["status"]
    fails = 0
    for p in range(len(pods)):
        want = (st[p] & abi.ST_RESV_FAIL) != 0
        assert np.array_equal(V.resv_verdicts(table, pods[p]), want), p
        fails += int(want.sum())
    assert fails > 0


# ------------------------------------------------- 3. hand-worked dry runs
def statuses(m):
    return [[int(s) for s in row["status"]] for row in m.verdicts]


def test_restricted_slot_passes_only_with_its_bound_pod_removed():
    m = V.case("restricted")
    assert V.resv_verdicts(m.table, m.pres[0]["pod"]).tolist() == [True]        # insufficient as the node stands
    assert statuses(m) == [[abi.PREEMPT_CANDIDATE]] and m.victims[0] == [V.RESTRICTED_VICTIMS]
    assert int(m.res["node"][0]) == 0 and int(m.res["best"]["n_victims"][0]) == 1


def test_default_slot_is_insufficient_only_once_something_is_preemptible():
    m = V.case("default")
    st = oracle.Oracle(m.cfg, m.table).eval(np.ascontiguousarray(m.pres["pod"]), status=True, scores=False)["status"]
    assert st.tolist() == [[0]]                                                 # the Filter passes the node as it stands
    assert statuses(m) == [[abi.PREEMPT_UNFIT]] and int(m.res["node"][0]) == -1


def test_unmatched_branch_and_nodes_without_state():
    m = V.case("unmatched")
    assert statuses(m) == [V.UNMATCHED_STATUS] and m.victims[0] == V.UNMATCHED_VICTIMS
    assert int(m.res["node"][0]) == 1 and m.res["count"][0].tolist() == [2, 0, 1, 0, 0]


def test_the_literal_add_back_changes_a_victim_list():
    m, fixed = V.case("quirk"), V.case("quirk", False)
    assert statuses(m) == [[abi.PREEMPT_CANDIDATE]] and m.victims[0] == [[]]
    assert fixed.victims[0] == [V.QUIRK_FIXED_VICTIMS]


# ------------------------------------------------ 4. the generated cases' cover
def test_generated_cases_meet_the_coverage_conditions():
    V.BRANCHES.clear()
    V.case.cache_clear()
    cases = {name: V.case(name) for name in V.CASES}
    taken = dict(V.BRANCHES)
    for branch in ("affinity", "nil_fits", "nil_fails", "nil_nothing", "default_nothing", "default_fits",
                   "default_insufficient", "aligned_fits", "aligned_insufficient", "restricted_passes",
                   "restricted_insufficient", "restricted_passes_returned", "restricted_insufficient_returned",
                   "insufficient", "matched_passes"):
        assert taken.get(branch, 0) > 0, branch
    for name in ("wave", "tiles", "numa", "numa4"):
        counts = cases[name].res["count"].sum(axis=0)
        assert (counts > 0).all(), (name, counts)                               # every status occurs
        assert (cases[name].res["count"].sum(axis=1) == cases[name].table.n).all()
    t = cases["tiles"]
    lists = M.node_lists(t.assigned, t.table.n)
    assert any(V.bound_slot(t.assigned[j]) >= 0 for lst in lists for j in lst[64:])   # a bound pod at position >= 64
    assert max(len(lst) for lst in lists) > 64 and t.table.resv_slots == 4
    assert {V.bound_slot(a) for a in t.assigned} >= {-1, 0, 1, 2}
    # the literal AddPod and a fixed one disagree on some verdict
    w = cases["tiles"]
    fixed = V.dry_run(w.cfg, w.table, w.assigned, w.pdb_allowed, w.pres, literal=False, base_cfg=w.base_cfg)
    assert fixed[1].tobytes() != w.verdicts.tobytes()
    # the shipped profile, cpuset preemptors among them
    nm = cases["numa"]
    assert int(nm.cfg.filter_plugins) & abi.PLUGIN_NUMA and (nm.pres["pod"]["flags"] & abi.POD_CPUSET).any()


# ------------------------------------------------------- 5. the host records
def _pod(name, node, bound=None, reserve=False):
    ann = {}
    if bound is not None:
        ann[rsv.ANNOTATION_RESERVATION_ALLOCATED] = json.dumps({"uid": bound[0], "name": bound[1]})
    if reserve:
        ann[rsv.ANNOTATION_RESERVE_POD] = "true"
    return k8s.Pod(name=name, node_name=node, annotations=ann, containers=[k8s.Container(requests=k8s.rl(cpu="1"))])


def test_assigned_records_resolve_reservation_slots():
    prof = shipped_profile(reservation=True)
    nodes = {"n0": 0, "n1": 1}
    rs = [rsv.Reservation(name="a", uid="u-a", node_name="n0"), rsv.Reservation(name="b", uid="u-b", node_name="n1"),
          rsv.Reservation(name="c", uid="u-c", node_name="n0")]
    slots = rsv.available_by_node(nodes, rs)
    pods = [_pod("p0", "n0", ("u-c", "c")), _pod("p1", "n1", ("u-b", "b")), _pod("p2", "n0"),
            _pod("r", "n0", reserve=True), _pod("p3", "n0", ("", "a"))]
    rec, _, keys = pre.assigned_records(pods, prof, nodes, pre.QuotaIds(), reservation_slots=slots)
    assert keys == ["default/p0", "default/p1", "default/p2", "default/p3"]          # the reserve pod is not listed
    field = (rec["flags"] & abi.ASG_RESV_SLOT_MASK).tolist()
    assert field == [abi.asg_resv_slot(1), abi.asg_resv_slot(0), 0, 0]              # an empty UID counts as not bound
    assert (rec["flags"] & abi.ASG_IN_QUOTA).all()
    with pytest.raises(MarshalError):                                               # u-b has no slot on n0
        pre.assigned_records([_pod("x", "n0", ("u-b", "b"))], prof, nodes, pre.QuotaIds(), reservation_slots=slots)
    others = [p for p in pods if p.name != "r"]
    plain, _, k2 = pre.assigned_records(others, prof, nodes, pre.QuotaIds())        # without slots: as before
    assert len(k2) == 4 and not (plain["flags"] & abi.ASG_RESV_SLOT_MASK).any()


# --------------------------------------------------------- 6. the constants
PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "koordhip.h"
int main(void) {
  printf("%u %u %u %u %u %u\n", KOORDHIP_PREEMPT_NUMA_FROZEN, KOORDHIP_PREEMPT_RESV, KOORDHIP_ASG_RESV_SLOT(0),
         KOORDHIP_ASG_RESV_SLOT(3), KOORDHIP_ASG_RESV_SLOT_MASK, KOORDHIP_ASG_RESV_SLOT_OF(KOORDHIP_ASG_RESV_SLOT(3) | 3u));
  printf("%zu %zu %d %d\n", offsetof(koordhip_assigned, flags), offsetof(koordhip_assigned, reserved),
         KOORDHIP_RESV_SLOTS, KOORDHIP_ABI_VERSION);
  return 0;
}
"""


def test_abi_constants_match_the_header():
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(src, "w").write(PROBE)
        subprocess.run(["gcc", "-std=c11", "-I", inc, src, "-o", exe], check=True)
        rows = [[int(x) for x in ln.split()] for ln in
                subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")]
    assert rows[0] == [abi.PREEMPT_NUMA_FROZEN, abi.PREEMPT_RESV, abi.asg_resv_slot(0), abi.asg_resv_slot(3),
                       abi.ASG_RESV_SLOT_MASK, 4]
    assert abi.PREEMPT_RESV == 2 and abi.asg_resv_slot(0) == 1 << 8 and abi.ASG_RESV_SLOT_MASK == 15 << 8
    assert rows[1] == [abi.ASSIGNED_DTYPE.fields["flags"][1], abi.ASSIGNED_DTYPE.fields["reserved"][1], abi.RESV_SLOTS, 15]
