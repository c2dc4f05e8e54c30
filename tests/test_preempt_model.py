"""The preemption model (preempt_model.py) itself: the hand-worked one- and
two-node cases of preempt_cases.py with the expected verdicts written out
(here again, and there in full), the construction of the contest cluster the
device's pick runs on (every contest's key level, placement and answer), the
generated cases' inputs (no degenerate case: candidates, nodes without
victims, unfit nodes and reprieved pods all occur), and the byte layout of the
three new ABI structs against gcc's view of the header.  No GPU."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from koordinator_amd import abi

import preempt_cases as K
import preempt_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAND, NOV, UNFIT, ERR, UNRES, B, ZERO = K.CAND, K.NOV, K.UNFIT, K.ERR, K.UNRES, K.B, K.ZERO


def run(case):
    """The model on a hand-worked case, and the case's whole expectation against it."""
    ver, vic, res = K.run_case(case)
    assert ver == case.ver
    assert vic == case.vic
    assert int(res["node"]) == case.node and list(res["count"]) == case.count
    assert tuple(res["best"].item()) == case.best
    return ver, vic, res


@pytest.mark.parametrize("name", list(K.WALK) + list(K.PICK) + list(K.EXTREME))
def test_hand_worked_case(name):
    run({**K.WALK, **K.PICK, **K.EXTREME}[name])


def test_candidate_with_a_reprieved_pod():
    ver, vic, res = run(K.WALK["reprieved"])
    assert ver == [(CAND, 1, 0, 100, 100 + B, 10)]
    assert vic == [[0]]
    assert int(res["node"]) == 0 and list(res["count"]) == [1, 0, 0, 0, 0]


def test_no_victims():
    ver, vic, res = run(K.WALK["no_victims"])
    assert ver == [(NOV,) + ZERO]
    assert int(res["node"]) == -1 and list(res["count"]) == [0, 1, 0, 0, 0]
    ver, _, _ = run(K.WALK["no_victims_skip"])
    assert ver == [(NOV,) + ZERO]
    ver, _, _ = run(K.WALK["no_victims_equal_priority"])
    assert ver == [(NOV,) + ZERO]


def test_unfit():
    ver, _, res = run(K.WALK["unfit"])
    assert ver == [(UNFIT,) + ZERO]
    assert list(res["count"]) == [0, 0, 1, 0, 0]


def test_unresolvable():
    ver, _, res = run(K.WALK["unresolvable"])
    assert ver == [(UNRES,) + ZERO, (CAND, 1, 0, 10, 10 + B, 0)]
    assert int(res["node"]) == 1 and list(res["count"]) == [1, 0, 0, 0, 1]


def test_error_a_pod_removed_twice():
    ver, vic, res = run(K.WALK["error"])
    assert ver == [(ERR,) + ZERO]
    assert vic == [[]]
    assert int(res["node"]) == -1 and list(res["count"]) == [0, 0, 0, 1, 0]


def test_victim_by_quota_alone():
    ver, vic, _ = run(K.WALK["quota_alone"])
    assert ver == [(CAND, 1, 0, 100, 100 + B, 7)]
    assert vic == [[0]]
    ver, vic, _ = run(K.WALK["quota_alone_uncounted"])
    assert ver == [(CAND, 2, 0, 100, 150 + 2 * B, 7)]
    assert vic == [[0, 1]]


def test_pdb_budget_zero_counts_a_violation():
    ver, vic, _ = run(K.WALK["pdb_zero"])
    assert ver == [(CAND, 1, 1, 100, 100 + B, 3)]
    ver, vic, _ = run(K.WALK["pdb_one"])
    assert vic == [[0]]                     # a1 (violating) goes first and fits back; a0 does not
    assert ver == [(CAND, 1, 0, 100, 100 + B, 3)]


def test_violating_pod_of_lower_priority_is_listed_first():
    ver, vic, _ = run(K.WALK["violating_first"])
    assert vic == [[1, 0]]
    assert ver == [(CAND, 2, 1, 50, 150 + 2 * B, 5)]   # top_priority 50, not the maximum 100


def test_list_order_ties():
    case = K.WALK["list_order"]
    assert M.node_lists(case.assigned, 1) == [[3, 1, 2, 0]] == case.lists
    _, vic, _ = run(case)
    assert vic == [[3, 1, 2, 0]]


def two_nodes(name):
    ver, _, res = run(K.PICK[name])
    assert [v[0] for v in ver] == [CAND, CAND]
    return ver, int(res["node"]), res


def test_pick_by_pdb_violations():
    ver, node, _ = two_nodes("pdb")
    assert (ver[0][2], ver[1][2]) == (1, 0) and node == 1


def test_pick_by_top_priority():
    ver, node, _ = two_nodes("top")
    assert (ver[0][3], ver[1][3]) == (200, 100) and node == 1


def test_pick_by_sum_priority():
    ver, node, _ = two_nodes("sum")
    assert ver[0][3] == ver[1][3] and ver[0][4] > ver[1][4] and node == 1


def test_pick_by_victim_count():
    ver, node, _ = two_nodes("count")
    assert ver[0][2:5] == ver[1][2:5] and (ver[0][1], ver[1][1]) == (3, 2) and node == 1


def test_pick_by_latest_start():
    ver, node, _ = two_nodes("start")
    assert ver[0][1:5] == ver[1][1:5] and (ver[0][5], ver[1][5]) == (10, 20) and node == 1


def test_pick_by_node_index():
    ver, node, res = two_nodes("index")
    assert ver[0] == ver[1] and node == 0
    assert tuple(res["best"].item()) == ver[0]


def test_a_candidate_without_victims_wins_outright():
    ver, vic, res = run(K.PICK["zero"])
    assert ver == [(CAND, 1, 0, -5, -5 + B, 0), (CAND,) + ZERO]
    assert vic == [[0], []]
    assert int(res["node"]) == 1 and int(res["best"]["n_victims"]) == 0


def test_three_equal_candidates():
    run(K.THREE)


# ------------------------------------------------------- the contest cluster
@pytest.fixture(scope="module")
def cluster():
    return K.contest_cluster()


def test_each_level_is_the_first_at_which_its_contest_differs():
    """What keeps the device test honest: the contest named for a level is decided there and nowhere before."""
    assert list(K.LEVELS.values()) == list(range(7))
    for name, level in K.LEVELS.items():
        assert K.first_difference(K.PICK[name]) == level, name
    for name, level in K.EXTREME_LEVEL.items():
        assert K.first_difference(K.EXTREME[name]) == level, name
    assert set(K.EXTREME_LEVEL) == set(K.EXTREME)
    # the halves: which 32 bits of the deciding field differ
    def halves(name, field):
        x, y = (v[field] & ((1 << 64) - 1) for v in K.EXTREME[name].ver)
        return (x >> 32) != (y >> 32), (x & 0xFFFFFFFF) != (y & 0xFFFFFFFF)
    assert halves("start_high_half", 5) == (True, False) and halves("start_low_half", 5) == (False, True)
    assert halves("sum_high_half", 4) == (True, False) and halves("sum_low_half", 4) == (False, True)
    for name, field in (("start_halves_disagree", 5), ("sum_halves_disagree", 4)):
        x, y = (v[field] for v in K.EXTREME[name].ver)
        assert (x < y) != ((x & 0xFFFFFFFF) < (y & 0xFFFFFFFF)), name
    # with the high word of the sums lost the next level (fewer victims) would pick the other node
    v = K.EXTREME["sum_high_half"].ver
    assert v[1][4] < v[0][4] and v[1][1] > v[0][1]
    assert {K.EXTREME["start_min_max"].ver[i][5] for i in (0, 1)} == {K.I64_MIN, K.I64_MAX}
    assert K.EXTREME["start_sign"].ver[0][5] < 0 <= K.EXTREME["start_sign"].ver[1][5]
    assert {K.EXTREME["top_lowest"].ver[i][3] for i in (0, 1)} == {K.LO, K.LO + 1}
    assert {K.EXTREME["top_highest"].ver[i][3] for i in (0, 1)} == {(1 << 30) - 1, (1 << 30) - 2}


def test_contests_cover_levels_placements_and_orientations(cluster):
    n, cts = K.CLUSTER_N, cluster.contests
    assert n == 65 * 256 + 1 and (n + 255) // 256 == K.CLUSTER_BLOCKS == 66
    assert len(cts) == len(cluster.pres) == 116 and len(cts) % 32 != 0 and (len(cts) + 31) // 32 == 4
    names = {ct.name for ct in cts}
    assert len(names) == len(cts)
    for placement in K.PLACEMENTS:
        for level in K.LEVELS:
            assert {f"{level}/{placement}/lo", f"{level}/{placement}/hi"} <= names
    for placement in ("wave", "far"):
        for name in K.EXTREME:
            assert {f"{name}/{placement}/lo", f"{name}/{placement}/hi"} <= names
    assert {"start/ragged/hi", "three"} <= names
    # the node sets are disjoint, and so are the quotas
    used = [i for ct in cts for i in ct.nodes]
    assert len(used) == len(set(used)) and 0 <= min(used) and max(used) == n - 1
    assert [ct.quota for ct in cts] == list(range(len(cts)))
    assert (cluster.pres["quota"] == np.arange(len(cts))).all() and (cluster.pres["q_mask"] == 0).all()
    for ct in cts:
        own = cluster.assigned[ct.base:ct.base + len(ct.case.pods)]
        assert (own["quota"] == ct.quota).all() and set(own["node"].tolist()) <= set(ct.nodes)
        assert ((own["pdb_mask"] != 0).any()) == ct.name.startswith("pdb/")
    # the placements straddle what they are named for
    every = set(K.PLACEMENTS) | {"ragged", "three"}
    assert {ct.placement for ct in cts} == every
    for ct in cts:
        i, j = sorted(ct.nodes)[:2]
        wave, group = (i // 64, j // 64), (i // 256, j // 256)
        if ct.placement == "wave":
            assert wave[0] == wave[1]
        elif ct.placement == "lanes":
            assert (i % 64, j) == (63, i + 1) and group[0] == group[1]
        elif ct.placement == "groups":
            assert (i % 256, j) == (255, i + 1)
        elif ct.placement == "strided":
            assert group[1] == group[0] + 64          # the same lane of the pick, the loop's next trip
        elif ct.placement == "far":
            assert group == (1, 33)                   # lanes 1 and 33 differ in bit 5 alone: shuffle offset 32
        elif ct.placement == "ragged":
            assert group == (0, 65) and j == n - 1 and ct.node == j
        else:
            assert len({x // 256 for x in ct.nodes}) == 3 and ct.node == min(ct.nodes)
    # orientation: the better node at the lower and at the higher index; equal keys: the lower index wins
    for ct in cts:
        if ct.name.startswith("index/"):
            assert ct.node == min(ct.nodes), ct.name
        elif ct.name.endswith("/lo"):
            assert ct.node == min(ct.nodes), ct.name
        elif ct.name.endswith("/hi"):
            assert ct.node == max(ct.nodes), ct.name


def test_every_contests_two_node_reduction(cluster):
    """Each contest alone, on as many nodes as it has, in the orientation it has in the cluster."""
    for ct in cluster.contests:
        order = np.argsort(ct.nodes)                  # local node k of this run = the contest's k-th lowest node
        local = {int(ct.nodes[c]): k for k, c in enumerate(order)}
        sel = slice(ct.base, ct.base + len(ct.case.pods))
        pods = cluster.assigned[sel].copy()
        pods["node"] = [local[int(x)] for x in pods["node"]]
        t = K.table(ct.case.n, pods)
        for node, k in local.items():
            t["requested0"][k] = cluster.table["requested0"][node]
        ver, vic, _ = M.select_victims(cluster.cfg, t, pods, cluster.pdb_allowed, cluster.pres[ct.quota])
        res = M.pick(ver)
        assert int(res["node"]) == local[ct.node], ct.name
        assert tuple(res["best"].item()) == tuple(ct.best), ct.name
        assert [ct.base + j for j in vic[int(res["node"])]] == ct.victims, ct.name
        assert list(res["count"]) == [ct.case.n, 0, 0, 0, 0], ct.name


def test_full_cluster_for_one_contest_per_placement(cluster):
    """The model on all 16641 nodes: the contest's own nodes are the only candidates."""
    lists = M.node_lists(cluster.assigned, K.CLUSTER_N)
    want = ["start/wave/hi", "index/lanes/lo", "count/groups/lo", "zero/strided/hi", "pdb/far/lo", "start/ragged/hi",
            "three", "sum_high_half/far/hi"]
    by_name = {ct.name: ct for ct in cluster.contests}
    for name in want:
        ct = by_name[name]
        ver, vic, _ = M.select_victims(cluster.cfg, cluster.table, cluster.assigned, cluster.pdb_allowed,
                                       cluster.pres[ct.quota], lists)
        res = M.pick(ver)
        assert res.tobytes() == cluster.res[ct.quota].tobytes(), name
        assert list(res["count"]) == [ct.case.n, K.CLUSTER_N - ct.case.n, 0, 0, 0], name
        assert sorted(np.flatnonzero(ver["status"] == abi.PREEMPT_CANDIDATE).tolist()) == sorted(ct.nodes), name
        assert vic[ct.node] == ct.victims, name
    assert cluster.victims.shape == (len(cluster.pres), 4)


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
