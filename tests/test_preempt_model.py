"""The preemption model (preempt_model.py) itself: hand-worked one- and
two-node cases with the expected verdicts written out, the generated cases'
inputs (no degenerate case: candidates, nodes without victims, unfit nodes and
reprieved pods all occur), and the byte layout of the three new ABI structs
against gcc's view of the header.  No GPU."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from koordinator_amd import abi
from koordinator_amd.config import PLUGIN_FIT, Profile, to_c_config, with_upstream
from koordinator_amd.snapshot import NodeTable

import preempt_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAND, NOV, UNFIT, ERR, UNRES = range(5)
B = 1 << 31
ALLOC = 10000


def A(node, cpu, prio, start=0, quota=0, flags=abi.ASG_IN_QUOTA, pdb=0):
    """One assigned pod requesting `cpu` milli-CPU."""
    a = np.zeros((), abi.ASSIGNED_DTYPE)
    a["pod"]["req"][abi.RES_CPU] = a["pod"]["nz_cpu_m"] = a["qreq"][0] = cpu
    a["pod"]["flags"] = abi.POD_HAS_REQ
    a["node"], a["priority"], a["start_time"], a["quota"], a["flags"], a["pdb_mask"] = node, prio, start, quota, flags, pdb
    return a


def preemptor(cpu, prio=1000, quota=0, used=0, runtime=None):
    p = np.zeros((), abi.PREEMPTOR_DTYPE)
    p["pod"]["req"][abi.RES_CPU] = p["pod"]["nz_cpu_m"] = p["q_req"][0] = cpu
    p["pod"]["flags"] = abi.POD_HAS_REQ
    p["priority"], p["quota"], p["q_used"][0] = prio, quota, used
    if runtime is not None:
        p["q_mask"], p["q_runtime"][0] = 1, runtime
    return p


def run(n, pods, pre, pdb=(), extra=None, static_off=()):
    """Nodes of 10 CPUs whose Requested is their pods' (plus extra[i]); returns
    (verdicts as tuples, victims per node, the pick)."""
    prof = Profile(filters=(PLUGIN_FIT,), scores={PLUGIN_FIT: 1})
    if static_off:
        prof = with_upstream(prof)
    t = NodeTable.empty(n)
    t["alloc0"][:] = ALLOC
    t["alloc1"][:] = 1 << 40
    t["alloc_pods"][:] = 110
    a = np.array(pods, abi.ASSIGNED_DTYPE) if pods else np.zeros(0, abi.ASSIGNED_DTYPE)
    for x in a:
        t["requested0"][x["node"]] += x["pod"]["req"][abi.RES_CPU]
        t["nz_cpu_m"][x["node"]] += x["pod"]["nz_cpu_m"]
        t["npods"][x["node"]] += 1
    for i, e in enumerate(extra or ()):
        t["requested0"][i] += e
    for i in static_off:
        t["static_allow"][i] = 0
    ver, vic, _ = M.select_victims(to_c_config(prof), t, a, pdb, pre)
    return [tuple(int(x) for x in v) for v in ver], vic, M.pick(ver)


ZERO = (0, 0, 0, 0, 0)


def test_candidate_with_a_reprieved_pod():
    # free 0; without a0 and a1 5 CPUs are free; a0 back leaves 2 (< 3): victim; a1 back leaves 3: reprieved
    ver, vic, res = run(1, [A(0, 3000, 100, 10), A(0, 2000, 50, 20), A(0, 4000, 2000, 5)], preemptor(3000), extra=[1000])
    assert ver == [(CAND, 1, 0, 100, 100 + B, 10)]
    assert vic == [[0]]
    assert int(res["node"]) == 0 and list(res["count"]) == [1, 0, 0, 0, 0]


def test_no_victims():
    # a higher priority, another quota, a non-preemptible pod: canPreempt accepts none
    pods = [A(0, 3000, 2000), A(0, 3000, 10, quota=1), A(0, 3000, 10, flags=abi.ASG_NONPREEMPTIBLE)]
    ver, vic, res = run(1, pods, preemptor(3000))
    assert ver == [(NOV,) + ZERO]
    assert int(res["node"]) == -1 and list(res["count"]) == [0, 1, 0, 0, 0]
    # postFilterState.skip: the ids still differ
    ver, _, _ = run(1, [A(0, 3000, 10)], preemptor(3000, quota=-1))
    assert ver == [(NOV,) + ZERO]
    # equal priority is not lower
    ver, _, _ = run(1, [A(0, 3000, 1000)], preemptor(3000, prio=1000))
    assert ver == [(NOV,) + ZERO]


def test_unfit():
    ver, _, res = run(1, [A(0, 500, 0)], preemptor(3000), extra=[9500])
    assert ver == [(UNFIT,) + ZERO]
    assert list(res["count"]) == [0, 0, 1, 0, 0]


def test_unresolvable():
    pods = [A(0, 3000, 10), A(1, 3000, 10)]
    ver, _, res = run(2, pods, preemptor(3000), extra=[7000, 7000], static_off=[0])
    assert ver == [(UNRES,) + ZERO, (CAND, 1, 0, 10, 10 + B, 0)]
    assert int(res["node"]) == 1 and list(res["count"]) == [1, 0, 0, 0, 1]


def test_error_a_pod_removed_twice():
    # a0 does not fit back (removed once) and used 0 + 3000 > runtime 2000 (removed again): RemovePod fails
    pods = [A(0, 3000, 100), A(0, 2000, 50)]
    ver, vic, res = run(1, pods, preemptor(3000, used=5000, runtime=2000), extra=[5000])
    assert ver == [(ERR,) + ZERO]
    assert vic == [[]]
    assert int(res["node"]) == -1 and list(res["count"]) == [0, 0, 0, 1, 0]


def test_victim_by_quota_alone():
    # both fit back (5 CPUs free without them, the preemptor asks 2); with a0 back used 3000 + 2000 > 4500
    pods = [A(0, 3000, 100, 7), A(0, 2000, 50, 9)]
    ver, vic, _ = run(1, pods, preemptor(2000, used=5000, runtime=4500), extra=[5000])
    assert ver == [(CAND, 1, 0, 100, 100 + B, 7)]
    assert vic == [[0]]
    # a pod the quota does not count moves no `used`: with runtime 1999 every pod is over, none is reprieved
    pods = [A(0, 3000, 100, 7, flags=0), A(0, 2000, 50, 9)]
    ver, vic, _ = run(1, pods, preemptor(2000, used=2000, runtime=1999), extra=[5000])
    assert ver == [(CAND, 2, 0, 100, 150 + 2 * B, 7)]
    assert vic == [[0, 1]]


def test_pdb_budget_zero_counts_a_violation():
    ver, vic, _ = run(1, [A(0, 3000, 100, 3, pdb=1)], preemptor(3000), pdb=(0,), extra=[7000])
    assert ver == [(CAND, 1, 1, 100, 100 + B, 3)]
    # budget 1: the first matching pod is within it, the second violates; a reprieved violating pod counts nothing
    pods = [A(0, 3000, 100, 3, pdb=1), A(0, 1000, 50, 4, pdb=1)]
    ver, vic, _ = run(1, pods, preemptor(3000), pdb=(1,), extra=[6000])
    assert vic == [[0]]                     # a1 (violating) goes first and fits back; a0 does not
    assert ver == [(CAND, 1, 0, 100, 100 + B, 3)]


def test_violating_pod_of_lower_priority_is_listed_first():
    pods = [A(0, 3000, 100, 5), A(0, 2000, 50, 6, pdb=1)]
    # 5 CPUs free without them, the preemptor asks 4: neither fits back
    ver, vic, _ = run(1, pods, preemptor(4000), pdb=(0,), extra=[5000])
    assert vic == [[1, 0]]
    assert ver == [(CAND, 2, 1, 50, 150 + 2 * B, 5)]   # top_priority 50, not the maximum 100


def test_list_order_ties():
    # equal priority: the earlier start first; equal start too: the lower input index first
    pods = [A(0, 1000, 7, 30), A(0, 1000, 7, 20), A(0, 1000, 7, 20), A(0, 1000, 9, 40)]
    assert M.node_lists(np.array(pods, abi.ASSIGNED_DTYPE), 1) == [[3, 1, 2, 0]]
    _, vic, _ = run(1, pods, preemptor(ALLOC))   # the preemptor asks the whole node: all victims, in that order
    assert vic == [[3, 1, 2, 0]]


# every pod of these nodes becomes a victim: the preemptor asks the whole node
def two_nodes(pods, pdb=()):
    ver, vic, res = run(2, pods, preemptor(ALLOC, prio=1 << 30), pdb=pdb)
    assert [v[0] for v in ver] == [CAND, CAND]
    return ver, int(res["node"]), res


def test_pick_by_pdb_violations():
    ver, node, _ = two_nodes([A(0, 1000, 100, pdb=1), A(1, 1000, 100)], pdb=(0,))
    assert (ver[0][2], ver[1][2]) == (1, 0) and node == 1


def test_pick_by_top_priority():
    ver, node, _ = two_nodes([A(0, 1000, 200), A(1, 1000, 100), A(1, 1000, 100)])
    assert (ver[0][3], ver[1][3]) == (200, 100) and node == 1


def test_pick_by_sum_priority():
    ver, node, _ = two_nodes([A(0, 1000, 100), A(0, 1000, 100), A(1, 1000, 100), A(1, 1000, 50)])
    assert ver[0][3] == ver[1][3] and ver[0][4] > ver[1][4] and node == 1


def test_pick_by_victim_count():
    # a victim of priority -2^31 adds 0 to the sum: equal sums, three victims against two
    lo = -(1 << 31)
    ver, node, _ = two_nodes([A(0, 1000, 0), A(0, 1000, 0), A(0, 1000, lo), A(1, 1000, 0), A(1, 1000, 0)])
    assert ver[0][2:5] == ver[1][2:5] and (ver[0][1], ver[1][1]) == (3, 2) and node == 1


def test_pick_by_latest_start():
    ver, node, _ = two_nodes([A(0, 1000, 100, 10), A(0, 1000, 50, 99), A(1, 1000, 100, 20), A(1, 1000, 50, 1)])
    assert ver[0][1:5] == ver[1][1:5] and (ver[0][5], ver[1][5]) == (10, 20) and node == 1


def test_pick_by_node_index():
    ver, node, res = two_nodes([A(0, 1000, 100, 10), A(1, 1000, 100, 10)])
    assert ver[0] == ver[1] and node == 0
    assert tuple(res["best"].item()) == ver[0]


def test_a_candidate_without_victims_wins_outright():
    # node 0: one victim of priority -5, the smaller key field by field; node 1: the preemptor fits with its pod back
    pods = [A(0, 3000, -5), A(1, 1000, 10)]
    ver, vic, res = run(2, pods, preemptor(3000), extra=[7000, 6000])
    assert ver == [(CAND, 1, 0, -5, -5 + B, 0), (CAND,) + ZERO]
    assert vic == [[0], []]
    assert int(res["node"]) == 1 and int(res["best"]["n_victims"]) == 0


def test_victims_array_pads_and_truncates():
    assert M.victims_array([[4, 2, 9], []], 2).tolist() == [[4, 2], [-1, -1]]
    assert M.victims_array([[4]], 3).tolist() == [[4, -1, -1]]


# ------------------------------------------------------ the generated cases
@pytest.mark.parametrize("name", list(M.CASES))
def test_generated_case_is_not_degenerate(name):
    m = M.case(name)
    n = m.table.n
    assert (m.res["count"].sum(axis=1) == n).all()
    # the preemptors are unschedulable as the rows stand
    import oracle
    st = oracle.Oracle(m.cfg, m.table).eval(np.ascontiguousarray(m.pres["pod"]), status=True, scores=False)["status"]
    assert (st != 0).all()
    seen = [set(np.unique(m.verdicts[p]["status"]).tolist()) for p in range(len(m.pres))]
    if n == 1:   # one node has one status: the case is the candidate
        assert seen == [{abi.PREEMPT_CANDIDATE}]
    else:
        assert any({abi.PREEMPT_CANDIDATE, abi.PREEMPT_NO_VICTIMS, abi.PREEMPT_UNFIT} <= s for s in seen)
    reprieved = [(p, i) for p in range(len(m.pres)) for i in range(n)
                 if m.verdicts[p]["status"][i] == abi.PREEMPT_CANDIDATE and len(m.victims[p][i]) < len(m.potential[p][i])]
    assert reprieved
    # ties, duplicates and every kind of pod occur
    a = m.assigned
    assert len(np.unique(a["priority"])) < len(a) and len(np.unique(a["start_time"])) <= len(M.STARTS)
    if n > 1:
        assert (a["flags"] & abi.ASG_NONPREEMPTIBLE).any() and (a["pdb_mask"] != 0).any()
        assert len(np.unique(a["quota"])) == 3
        assert np.bincount(a["node"], minlength=n).max() <= abi.PREEMPT_NODE_PODS


def test_generated_cases_cover_the_rare_verdicts():
    allv = np.concatenate([M.case(c).verdicts.reshape(-1) for c in M.CASES])
    assert set(np.unique(allv["status"]).tolist()) == set(range(abi.PREEMPT_STATUSES))
    assert (allv["n_pdb_violations"] > 0).any()
    cand = allv[allv["status"] == abi.PREEMPT_CANDIDATE]
    assert (cand["n_victims"] > 1).any()
    other = allv[allv["status"] != abi.PREEMPT_CANDIDATE]
    for f in ("n_victims", "n_pdb_violations", "top_priority", "sum_priority", "earliest_start"):
        assert not other[f].any(), f
    # a pod made a victim by the quota alone: more victims than pods that do not fit back is not observable
    # from the verdict, so look at a short-runtime preemptor's chosen victims against an ample-runtime twin
    m = M.case("tiles")
    p = next(p for p in range(len(m.pres)) if m.pres["quota"][p] >= 0 and m.pres["q_runtime"][p][0] < (1 << 39))
    twin = m.pres[p].copy()
    twin["q_runtime"][0] = 1 << 50
    v2, _, _ = M.select_victims(m.cfg, m.table, m.assigned, m.pdb_allowed, twin)
    both = (m.verdicts[p]["status"] == abi.PREEMPT_CANDIDATE) & (v2["status"] == abi.PREEMPT_CANDIDATE)
    assert (m.verdicts[p]["n_victims"][both] > v2["n_victims"][both]).any()


# ------------------------------------------------------------- struct layout
PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "koordhip.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(koordhip_assigned), sizeof(koordhip_preemptor), sizeof(koordhip_preempt_node),
         sizeof(koordhip_preempt_result));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(koordhip_assigned, node), offsetof(koordhip_assigned, priority),
         offsetof(koordhip_assigned, start_time), offsetof(koordhip_assigned, quota), offsetof(koordhip_assigned, flags),
         offsetof(koordhip_assigned, pdb_mask), offsetof(koordhip_assigned, reserved), offsetof(koordhip_assigned, qreq));
  printf("%zu %zu %zu %zu %zu %zu\n", offsetof(koordhip_preemptor, priority), offsetof(koordhip_preemptor, quota),
         offsetof(koordhip_preemptor, q_used), offsetof(koordhip_preemptor, q_runtime), offsetof(koordhip_preemptor, q_req),
         offsetof(koordhip_preemptor, q_mask));
  printf("%zu %zu %zu %zu %zu %zu\n", offsetof(koordhip_preempt_node, status), offsetof(koordhip_preempt_node, n_victims),
         offsetof(koordhip_preempt_node, n_pdb_violations), offsetof(koordhip_preempt_node, top_priority),
         offsetof(koordhip_preempt_node, sum_priority), offsetof(koordhip_preempt_node, earliest_start));
  printf("%zu %zu %zu\n", offsetof(koordhip_preempt_result, node), offsetof(koordhip_preempt_result, count),
         offsetof(koordhip_preempt_result, best));
  printf("%d %d %d %d\n", KOORDHIP_PREEMPT_QRES, KOORDHIP_PREEMPT_PDBS, KOORDHIP_PREEMPT_NODE_PODS, KOORDHIP_ABI_VERSION);
  printf("%d %d %d %d %d %u %u\n", KOORDHIP_PREEMPT_CANDIDATE, KOORDHIP_PREEMPT_NO_VICTIMS, KOORDHIP_PREEMPT_UNFIT,
         KOORDHIP_PREEMPT_ERROR, KOORDHIP_PREEMPT_UNRESOLVABLE, KOORDHIP_ASG_NONPREEMPTIBLE, KOORDHIP_ASG_IN_QUOTA);
  return 0;
}
"""


def offsets(dt, names):
    return [dt.fields[f][1] for f in names]


def test_struct_layout_matches_header():
    inc = os.path.join(ROOT, "include")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(src, "w").write(PROBE)
        subprocess.run(["gcc", "-std=c11", "-I", inc, src, "-o", exe], check=True)
        rows = [[int(x) for x in ln.split()] for ln in
                subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")]
    assert rows[0] == [abi.ASSIGNED_DTYPE.itemsize, abi.PREEMPTOR_DTYPE.itemsize, abi.PREEMPT_NODE_DTYPE.itemsize,
                       abi.PREEMPT_RESULT_DTYPE.itemsize]
    assert rows[1] == offsets(abi.ASSIGNED_DTYPE, ["node", "priority", "start_time", "quota", "flags", "pdb_mask",
                                                   "reserved", "qreq"])
    assert rows[2] == offsets(abi.PREEMPTOR_DTYPE, ["priority", "quota", "q_used", "q_runtime", "q_req", "q_mask"])
    assert rows[3] == offsets(abi.PREEMPT_NODE_DTYPE, ["status", "n_victims", "n_pdb_violations", "top_priority",
                                                       "sum_priority", "earliest_start"])
    assert rows[4] == offsets(abi.PREEMPT_RESULT_DTYPE, ["node", "count", "best"])
    assert rows[5] == [abi.PREEMPT_QRES, abi.PREEMPT_PDBS, abi.PREEMPT_NODE_PODS, 15]
    assert rows[6] == [abi.PREEMPT_CANDIDATE, abi.PREEMPT_NO_VICTIMS, abi.PREEMPT_UNFIT, abi.PREEMPT_ERROR,
                       abi.PREEMPT_UNRESOLVABLE, abi.ASG_NONPREEMPTIBLE, abi.ASG_IN_QUOTA]
    assert abi.ASSIGNED_DTYPE.fields["pod"][1] == 0 and abi.PREEMPTOR_DTYPE.fields["pod"][1] == 0


def test_symbols_are_exported_and_abi_stays_15():
    lib = abi.load_library()
    for name in ("koordhip_preempt_load_pods", "koordhip_preempt", "koordhip_preempt_node_verdicts"):
        assert hasattr(lib, name) and name in abi.EXPORTED_SYMBOLS
    assert lib.koordhip_abi_version() == 15
