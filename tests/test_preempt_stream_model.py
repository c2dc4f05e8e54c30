"""The sequential dry run's model (preempt_stream_model.py) itself: hand-worked
one- and two-node cases with the expected answers written out, the conditions
that keep the generated cases from being degenerate (the stream really differs
from the independent batch, no pod is a victim twice, both kinds of global
flag rise in `tiles` and none in `clean`), that every directed case reaches
the situation it is named for, and the byte layout of
koordhip_preempt_stream_stats against gcc's view of the header.  No GPU."""
import os
import subprocess
import tempfile
from collections import Counter

import numpy as np
import pytest

from koordinator_amd import abi
from koordinator_amd.config import PLUGIN_FIT, Profile, to_c_config
from koordinator_amd.snapshot import NodeTable

import preempt_model as M
import preempt_stream_model as S
from preempt_cases import A, preemptor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAND, NOV, UNFIT, ERR, UNRES = range(5)
B = 1 << 31
ALLOC = 10000


def setup(n, pods, extra):
    """Nodes of 10 CPUs whose Requested is their pods' plus extra[i]."""
    cfg = to_c_config(Profile(filters=(PLUGIN_FIT,), scores={PLUGIN_FIT: 1}))
    t = NodeTable.empty(n)
    t["alloc0"][:] = ALLOC
    t["alloc1"][:] = 1 << 40
    t["alloc_pods"][:] = 110
    a = np.array(pods, abi.ASSIGNED_DTYPE)
    for x in a:
        t["requested0"][x["node"]] += x["pod"]["req"][abi.RES_CPU]
        t["nz_cpu_m"][x["node"]] += x["pod"]["nz_cpu_m"]
        t["npods"][x["node"]] += 1
    for i, e in enumerate(extra):
        t["requested0"][i] += e
    return cfg, t, a


def both(n, pods, pres, pdb=(), extra=()):
    """(the independent batch's results, the stream's results, the stream's victims, its stats)."""
    cfg, t, a = setup(n, pods, extra)
    pres = np.array(pres, abi.PREEMPTOR_DTYPE)
    ind = M.dry_run(cfg, t, a, pdb, pres)[0]
    res, chosen, stats = S.stream(cfg, t, a, pdb, pres)
    return ind, res, chosen, stats


def best(r):
    return tuple(int(x) for x in r["best"].item())


def test_second_preemptor_cannot_take_the_firsts_victims():
    # two full nodes; both preemptors alone pick node 0 (its victim has the lower priority)
    pods = [A(0, 3000, 10), A(1, 3000, 50)]
    ind, res, chosen, _ = both(2, pods, [preemptor(3000), preemptor(3000)], extra=[7000, 7000])
    assert ind["node"].tolist() == [0, 0]
    # in sequence a0 is gone and the first preemptor (equal priority) fills node 0 again: no pod left to take there
    assert res["node"].tolist() == [0, 1]
    assert chosen == [[0], [1]]
    assert list(res["count"][0]) == [2, 0, 0, 0, 0] and list(res["count"][1]) == [1, 1, 0, 0, 0]
    assert best(res[1]) == (CAND, 1, 0, 50, 50 + B, 0)


def test_unfit_only_because_of_a_nominated_pod_of_equal_priority():
    # 5 CPUs free without a0 and a1; a1 (2 CPUs) fits back beside the first preemptor's 3, a0 does not: victim a0
    pods = [A(0, 3000, 10), A(0, 2000, 20)]
    first = preemptor(3000)
    ind, res, chosen, _ = both(1, pods, [first, preemptor(2500, prio=1000)], extra=[5000])
    assert ind["node"].tolist() == [0, 0]
    assert chosen[0] == [0]
    # equal priority: the nominated 3 CPUs count, a1's 2 CPUs do not make room for 2.5
    assert int(res["node"][1]) == -1 and list(res["count"][1]) == [0, 0, 1, 0, 0]
    # a higher priority does not see the nominated pod: 5 CPUs free without a1, and a1 fits back
    _, res, chosen, _ = both(1, pods, [first, preemptor(2500, prio=1001)], extra=[5000])
    assert int(res["node"][1]) == 0 and best(res[1]) == (CAND, 0, 0, 0, 0, 0)
    assert chosen == [[0], []]


def test_spent_pdb_budget_makes_the_next_victim_violating():
    pods = [A(0, 3000, 10, pdb=1), A(1, 3000, 20, pdb=1)]
    ind, res, chosen, stats = both(2, pods, [preemptor(3000), preemptor(3000)], pdb=(1,), extra=[7000, 7000])
    assert [best(r)[2] for r in ind] == [0, 0]          # alone, each victim is within the budget of 1
    assert res["node"].tolist() == [0, 1] and chosen == [[0], [1]]
    assert best(res[0]) == (CAND, 1, 0, 10, 10 + B, 0)
    assert best(res[1]) == (CAND, 1, 1, 20, 20 + B, 0)  # the budget is spent: a1 violates it
    assert stats["pdb_flag"] and stats["full_recomputes"] == 1
    # the floor: with budget 0 nothing changes, so nothing forces a recompute
    _, res, _, stats = both(2, pods, [preemptor(3000), preemptor(3000)], pdb=(0,), extra=[7000, 7000])
    assert [best(r)[2] for r in res] == [1, 1] and not stats["pdb_flag"]


def test_freed_quota_turns_an_error_node_into_a_candidate():
    # the second preemptor's quota: used 6 CPUs, runtime 4.  Alone, with the node's pod removed and not fitting back
    # used is 3 and 3 + 3 > 4: the pod is removed a second time, ERROR on both nodes.
    pods = [A(0, 3000, 10), A(1, 3000, 100)]
    pres = [preemptor(3000, used=6000, runtime=1 << 40), preemptor(3000, used=6000, runtime=4000)]
    ind, res, chosen, stats = both(2, pods, pres, extra=[7000, 7000])
    assert int(ind["node"][1]) == -1 and list(ind["count"][1]) == [0, 0, 0, 2, 0]
    # in sequence the first preemptor's victim freed 3 CPUs of the quota: 0 + 3 <= 4
    assert res["node"].tolist() == [0, 1] and chosen == [[0], [1]]
    assert list(res["count"][1]) == [1, 1, 0, 0, 0]
    assert stats["quota_flags"] == 1 and stats["full_recomputes"] == 1 and not stats["pdb_flag"]
    # another quota's preemptor sees no freed amount (and other quotas' pods are not its victims)
    pres[1]["quota"] = 1
    _, res, _, stats = both(2, pods, pres, extra=[7000, 7000])
    assert int(res["node"][1]) == -1 and stats["quota_flags"] == 0


def test_a_preemptor_without_a_node_changes_nothing():
    pods = [A(0, 3000, 10), A(1, 3000, 50)]
    pres = [preemptor(3000, prio=5), preemptor(3000), preemptor(3000)]
    ind, res, chosen, stats = both(2, pods, pres, extra=[7000, 7000])
    assert int(res["node"][0]) == -1 and chosen[0] == []
    assert res[1].tobytes() == ind[1].tobytes()           # the second is the first to change anything
    assert res["node"].tolist() == [-1, 0, 1]
    assert stats["block_recomputes"] == 1 and stats["blocks_skipped"] == 2


# ------------------------------------------------------ the generated cases
def test_prio_case_is_what_its_docstring_says():
    m = S.case("prio")
    assert m.res["node"].tolist() == [1, 1, 2]
    assert m.chosen == [[1], [2], [3]]
    assert list(m.res["count"][2]) == [1, 2, 0, 0, 0]
    # were the nominated pod of priority 100 counted for the preemptor of priority 1000, node 1 would be UNFIT
    assert list(m.res["count"][1]) == [2, 0, 1, 0, 0]


# --------------------------------------------------------- the directed cases
def alone(m, k):
    """Preemptor k of the case on the loaded state, as koordhip_preempt answers it."""
    return M.select_victims(m.cfg, m.table, m.assigned, m.pdb_allowed, m.pres[k])


def test_word1_reads_the_second_overlay_word():
    m = S.case("word1")
    assert int((m.assigned["node"] == 0).sum()) == abi.PREEMPT_NODE_PODS
    assert m.res["node"].tolist() == [0, 0, 0]
    pos = {j: k for k, j in enumerate(M.node_lists(m.assigned, 2)[0])}
    first = sorted(pos[j] for j in m.chosen[0])
    assert first == list(range(58, 128))            # 6 positions of the first word, all 64 of the second
    # the later preemptors of the same quota walk the same list without them
    assert sorted(pos[j] for j in m.chosen[1]) == list(range(48, 58))
    assert sorted(pos[j] for j in m.chosen[2]) == list(range(38, 48))
    assert len({int(q) for q in m.pres["quota"]}) == 1
    assert [best(r) for r in m.res] == [(CAND, 70, 0, 386, 70 * B + sum(400 - p // 4 for p in range(58, 128)), 2),
                                        (CAND, 10, 0, 388, 10 * B + sum(400 - p // 4 for p in range(48, 58)), 0),
                                        (CAND, 10, 0, 391, 10 * B + sum(400 - p // 4 for p in range(38, 48)), 2)]
    assert m.res["count"].tolist() == [[1, 0, 1, 0, 0], [2, 0, 0, 0, 0], [1, 0, 1, 0, 0]]
    # the input order is not the list's
    assert [pos[j] for j in range(4)] == [0, 37, 74, 111]


def test_chain_of_nominated_pods_straddles_the_last_priority():
    m = S.case("chain")
    assert m.res["node"].tolist() == [0, 0, 0, 0, 0]     # four nominated on node 0 before the fifth looks at it
    prio = [int(p) for p in m.pres["priority"]]
    assert prio == list(S.CHAIN_PRIORITIES)
    assert sorted(p >= prio[4] for p in prio[:4]) == [False, False, True, True]
    assert m.chosen == [[0], [1], [2], [4, 3], [5]]
    assert [best(r) for r in m.res] == [(CAND, 1, 0, 1, 1 + B, 1), (CAND, 1, 0, 2, 2 + B, 2), (CAND, 1, 0, 3, 3 + B, 3),
                                        (CAND, 2, 0, 5, 9 + 2 * B, 5), (CAND, 1, 0, 6, 6 + B, 6)]
    assert m.res["count"].tolist() == [[2, 0, 0, 0, 0]] * 3 + [[1, 1, 0, 0, 0], [2, 0, 0, 0, 0]]
    # alone, the fifth would take the three pods of the lowest priorities
    ver, vic, _ = alone(m, 4)
    assert vic[0] == [2, 1, 0]


def test_budget_is_spent_once_and_stays_at_zero():
    m = S.case("budget")
    assert m.pdb_allowed == (1,)
    assert m.res["node"].tolist() == [0, 3, 1, 2] and m.chosen == [[0], [3], [1], [2]]
    npdb = [best(r)[2] for r in m.res]
    assert npdb == [0, 0, 1, 1]                          # a violation after a 0 before
    assert m.stats["pdb_flag"]
    assert [int(m.assigned["pdb_mask"][v[0]]) for v in m.chosen] == [1, 0, 1, 1]   # two more matching victims at 0
    assert [best(r) for r in m.res] == [(CAND, 1, 0, 10, 10 + B, 0), (CAND, 1, 0, 500, 500 + B, 0),
                                        (CAND, 1, 1, 20, 20 + B, 0), (CAND, 1, 1, 30, 30 + B, 0)]
    assert m.res["count"].tolist() == [[4, 0, 0, 0, 0], [3, 1, 0, 0, 0], [2, 2, 0, 0, 0], [1, 3, 0, 0, 0]]
    # alone every one of them takes node 0 within the budget
    ind = M.dry_run(m.cfg, m.table, m.assigned, m.pdb_allowed, m.pres)[0]
    assert ind["node"].tolist() == [0] * 4 and not ind["best"]["n_pdb_violations"].any()


def test_quota_used_is_floored_at_zero():
    m = S.case("floor")
    assert m.res["node"].tolist() == [0, 1, -1] and m.chosen == [[0], [1], []]
    freed = int(m.assigned["qreq"][0][0])
    assert freed > int(m.pres["q_used"][1][0]) == int(m.pres["q_used"][2][0]) > 0     # more freed than used
    # preemptor 1 alone: both pods of node 1 are victims, neither because it does not fit back
    ver, vic, _ = alone(m, 1)
    assert vic[1] == [2, 1] and best_of(ver[1]) == (CAND, 2, 0, 45, 85 + 2 * B, 0)
    ample = m.pres[1].copy()
    ample["q_runtime"][0] = 1 << 40
    assert alone_with(m, ample)[1][1] == [1]             # by fit the pod of 40 alone
    # in sequence: one victim, and that one by fit
    assert best(m.res[1]) == (CAND, 1, 0, 40, 40 + B, 0) and list(m.res["count"][1]) == [1, 1, 0, 0, 0]
    # preemptor 2: ERROR with used 0; a candidate had used gone to -1
    assert list(m.res["count"][2]) == [0, 1, 0, 1, 0]
    assert m.stats["quota_flags"] == 2


def best_of(v):
    return tuple(int(x) for x in v)


def alone_with(m, pre):
    return M.select_victims(m.cfg, m.table, m.assigned, m.pdb_allowed, pre)


def test_tiles3_raises_the_pdb_flag_inside_the_second_tile():
    m = S.case("tiles3")
    assert len(m.pres) == S.TILES3_PRE == 65 and (len(m.pres) + 31) // 32 == 3
    assert 257 <= m.table.n <= 300
    k0 = S.TILES3_K0
    assert 32 + 8 <= k0 < 64 - 8                         # well inside the second tile
    a = m.assigned
    assert S.TILES3_VICTIM in m.chosen[k0] and int(a["pdb_mask"][S.TILES3_VICTIM]) == 1
    # no earlier victim spends the budget, so the flag rises with k0's pick and not before
    assert not any(int(a["pdb_mask"][j]) for k in range(k0) for j in m.chosen[k])
    assert m.stats["pdb_flag"] and m.stats["quota_flags"] == 0
    assert m.stats["full_recomputes"] == len(m.pres) - 1 - k0
    # up to k0 the answers are those without any PDB; after it a victim violates
    plain = S.stream(m.cfg, m.table, _without_pdb(a), (), m.pres[:k0 + 1])[0]
    assert plain.tobytes() == m.res[:k0 + 1].tobytes()
    later = m.res["best"]["n_pdb_violations"][k0 + 1:]
    assert not m.res["best"]["n_pdb_violations"][:k0 + 1].any() and (later > 0).any()
    assert int(m.res["node"][64]) >= 0                   # the third tile's only preemptor has an answer to get wrong
    assert (m.res["node"][32:k0] >= 0).any() and (m.res["node"][k0 + 1:64] >= 0).any()


def _without_pdb(a):
    b = a.copy()
    b["pdb_mask"] = 0
    return b


@pytest.mark.parametrize("name", S.CASES)
def test_no_pod_is_a_victim_twice(name):
    m = S.case(name)
    allv = [j for v in m.chosen for j in v]
    assert len(allv) == len(set(allv))
    assert (m.res["count"].sum(axis=1) == m.table.n).all()
    for k, v in enumerate(m.chosen):
        assert len(v) == int(m.res["best"]["n_victims"][k])


def test_tiles_differs_from_the_independent_batch():
    m, ind = S.case("tiles"), M.case("tiles")
    assert int((m.res["node"] != ind.res["node"]).sum()) >= 10
    placed = Counter(int(x) for x in m.res["node"] if x >= 0)
    assert max(placed.values()) > 1                      # a node is chosen by more than one preemptor
    assert m.stats["pdb_flag"] and m.stats["quota_flags"] > 0
    assert m.stats["full_recomputes"] > 0
    # the independent batch is what the stream replaces: its picks collide
    dup = Counter(j for v in ind.chosen for j in v)
    assert any(c > 1 for c in dup.values())


def test_first_preemptor_equals_the_independent_one():
    for name in M.CASES:
        assert S.case(name).res[0].tobytes() == M.case(name).res[0].tobytes()
        assert S.case(name).chosen[0] == M.case(name).chosen[0]


def test_clean_raises_no_global_flag():
    m = S.case("clean")
    assert len(m.pres) == 16 and m.table.n >= 257
    assert not m.stats["pdb_flag"] and m.stats["quota_flags"] == 0 and m.stats["full_recomputes"] == 0
    assert m.stats["blocks_skipped"] > 0 and m.stats["block_recomputes"] > 0
    assert int((m.res["node"] >= 0).sum()) >= 8


# ------------------------------------------------------------- struct layout
PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "koordhip.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(koordhip_preempt_stream_stats), offsetof(koordhip_preempt_stream_stats, full_recomputes),
         offsetof(koordhip_preempt_stream_stats, block_recomputes), offsetof(koordhip_preempt_stream_stats, blocks_skipped));
  printf("%d\n", KOORDHIP_ABI_VERSION);
  return 0;
}
"""


def test_stats_layout_matches_header():
    inc = os.path.join(ROOT, "include")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(src, "w").write(PROBE)
        subprocess.run(["gcc", "-std=c11", "-I", inc, src, "-o", exe], check=True)
        rows = [[int(x) for x in ln.split()] for ln in
                subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")]
    dt = abi.PREEMPT_STREAM_STATS_DTYPE
    assert rows[0] == [dt.itemsize] + [dt.fields[f][1] for f in ("full_recomputes", "block_recomputes", "blocks_skipped")]
    assert rows[1] == [15]


def test_symbol_is_exported_and_abi_stays_15():
    lib = abi.load_library()
    assert hasattr(lib, "koordhip_preempt_stream") and "koordhip_preempt_stream" in abi.EXPORTED_SYMBOLS
    assert lib.koordhip_abi_version() == 15
