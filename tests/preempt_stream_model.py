"""The sequential preemption dry run (koordhip_preempt_stream), computed with
the CPU oracle alone: a Python loop over the preemptors on top of
preempt_model.select_victims / pick / node_lists.  Preemptor k is answered on
the hypothetical state S_k that the earlier preemptors left:

    gone        the victims of every earlier preemptor that found a node: off
                their rows, out of the lists (never a victim again, no PDB
                budget consumed in the split)
    nominated   the earlier preemptors themselves on their nodes, added to the
                row for a later preemptor of equal or lower priority
    allowed     the PDB budgets, lowered by one per victim and matching PDB,
                floored at 0
    freed       per quota id the qreq of the IN_QUOTA victims: a later
                preemptor of the same quota sees max(0, q_used - freed)

Also the bookkeeping the engine reports as koordhip_preempt_stream_stats (which
256-node blocks it has to evaluate again), the two generated cases `clean`
and `prio` beside preempt_model.CASES, and the directed cases for the state
the overlay carries (DIRECTED; test_preempt_stream_model.py asserts that each
reaches the situation it is named for).
"""
import functools

import numpy as np

from koordinator_amd import abi, synth
from koordinator_amd.config import to_c_config
from koordinator_amd.snapshot import NodeTable

import preempt_cases as K
import preempt_model as M

BLOCK = 256   # nodes per workgroup of the engine's evaluation (the unit of its skip)


def stream(cfg, table, assigned, pdb_allowed, pres, lists=None, rule=M.Rule):
    """(results [p] PREEMPT_RESULT_DTYPE, full victim lists per preemptor,
    stats dict) of the preemptors processed in input order.  rule: select_victims'."""
    n = table.n
    lists = lists if lists is not None else M.node_lists(assigned, n)
    nb = (n + BLOCK - 1) // BLOCK
    gone = set()
    nominated = []                       # (node, pod record, priority)
    allowed = [int(x) for x in pdb_allowed]
    freed = {}                           # quota id -> [QRES]
    touched = set()                      # blocks whose rows / lists differ from S_0
    pdb_flag = False
    res = np.zeros(len(pres), abi.PREEMPT_RESULT_DTYPE)
    chosen = []
    stats = dict(full_recomputes=0, block_recomputes=0, blocks_skipped=0, pdb_flag=False, quota_flags=0)
    for k in range(len(pres)):
        pre = pres[k].copy()
        prio, quota = int(pre["priority"]), int(pre["quota"])
        t = table.copy()
        cols = {c: t[c] for c in M.ROW_COLS}

        def move(i, pod, sign):
            for r in range(M.NRES):
                cols[f"requested{r}"][i] += sign * int(pod["req"][r])
            cols["nz_cpu_m"][i] += sign * int(pod["nz_cpu_m"])
            cols["nz_mem"][i] += sign * int(pod["nz_mem"])
            cols["npods"][i] += sign

        for j in gone:
            move(int(assigned["node"][j]), assigned["pod"][j], -1)
        for node, pod, p in nominated:
            if p >= prio:
                move(node, pod, +1)
        lists_k = [[j for j in l if j not in gone] for l in lists] if gone else lists
        qflag = quota >= 0 and any(freed.get(quota, ()))
        if quota >= 0 and quota in freed:
            for d in range(abi.PREEMPT_QRES):
                pre["q_used"][d] = max(0, int(pre["q_used"][d]) - freed[quota][d])
        if n:
            if pdb_flag or qflag:
                stats["full_recomputes"] += 1
                stats["block_recomputes"] += nb
            else:
                stats["block_recomputes"] += len(touched)
                stats["blocks_skipped"] += nb - len(touched)
            stats["quota_flags"] += bool(qflag)
        ver, vic, _ = M.select_victims(cfg, t, assigned, allowed, pre, lists_k, rule)
        res[k] = M.pick(ver)
        c = int(res[k]["node"])
        if c < 0:
            chosen.append([])
            continue
        v = list(vic[c])
        chosen.append(v)
        gone.update(v)
        nominated.append((c, pres[k]["pod"].copy(), prio))
        touched.add(c // BLOCK)
        for j in v:
            a = assigned[j]
            for b in range(len(allowed)):
                if (int(a["pdb_mask"]) >> b) & 1 and allowed[b] > 0:
                    allowed[b] -= 1
                    pdb_flag = True
            if quota >= 0 and int(a["flags"]) & abi.ASG_IN_QUOTA:
                f = freed.setdefault(quota, [0] * abi.PREEMPT_QRES)
                for d in range(abi.PREEMPT_QRES):
                    f[d] += int(a["qreq"][d])
    stats["pdb_flag"] = pdb_flag
    return res, chosen, stats


# ---------------------------------------------------------------- generators
def _clean() -> M.Inputs:
    """~300 nodes, 16 preemptors, every preemptor in a quota of its own with an
    ample runtime, no PDB: neither global flag can rise."""
    inp = M.inputs("base", 300, 16, M.SEED + 11, False)
    a, pres = inp.assigned, inp.pres
    a["pdb_mask"] = 0
    # 16 quotas, one per preemptor; the assigned pods are spread over them
    a["quota"] = (synth.splitmix64(M.SEED + 11, len(a), 730) % np.uint64(16)).astype(np.int32)
    inq = (a["flags"] & abi.ASG_IN_QUOTA) != 0
    for p in range(len(pres)):
        pres["quota"][p] = p
        pres["q_used"][p] = a["qreq"][inq & (a["quota"] == p)].sum(axis=0)
        pres["q_runtime"][p] = pres["q_used"][p] + pres["q_req"][p] + (1 << 40)
    return M.Inputs(inp.prof, inp.table, a, (), pres)


def _prio() -> M.Inputs:
    """Three hand-made full nodes of 10 CPUs.  Preemptor 0 (priority 100, 3
    CPUs) takes node 1's pod of priority 10.  Preemptor 1 (priority 1000, 8
    CPUs) must not see the nominated pod of lower priority: node 1 without its
    other pod (priority 500) has 10 CPUs free, with the nominated 3 CPUs
    counted it would have 7 and be UNFIT; its victim of priority 500 beats
    node 0's of priority 900, so preemptor 1 lands on node 1 as well.
    Preemptor 2 (priority 100, 4 CPUs) sees both nominated pods (priorities
    100 and 1000 >= 100) and no pod left on node 1, and takes node 2's pod."""
    from koordinator_amd.config import PLUGIN_FIT, Profile
    prof = Profile(filters=(PLUGIN_FIT,), scores={PLUGIN_FIT: 1})
    n = 3
    t = NodeTable.empty(n)
    t["alloc0"][:] = 10000
    t["alloc1"][:] = 1 << 40
    t["alloc_pods"][:] = 110

    def A(node, cpu, prio, start):
        a = np.zeros((), abi.ASSIGNED_DTYPE)
        a["pod"]["req"][abi.RES_CPU] = a["pod"]["nz_cpu_m"] = a["qreq"][0] = cpu
        a["pod"]["flags"] = abi.POD_HAS_REQ
        a["node"], a["priority"], a["start_time"], a["quota"], a["flags"] = node, prio, start, 0, abi.ASG_IN_QUOTA
        return a

    a = np.array([A(0, 10000, 900, 1), A(1, 3000, 10, 2), A(1, 7000, 500, 3), A(2, 4000, 50, 4), A(2, 6000, 2000, 5)],
                 abi.ASSIGNED_DTYPE)
    for x in a:
        t["requested0"][x["node"]] += x["pod"]["req"][abi.RES_CPU]
        t["nz_cpu_m"][x["node"]] += x["pod"]["nz_cpu_m"]
        t["npods"][x["node"]] += 1
    pres = np.zeros(3, abi.PREEMPTOR_DTYPE)
    for p, (cpu, prio) in enumerate([(3000, 100), (8000, 1000), (4000, 100)]):
        pres["pod"]["req"][p, abi.RES_CPU] = pres["pod"]["nz_cpu_m"][p] = pres["q_req"][p, 0] = cpu
        pres["pod"]["flags"][p] = abi.POD_HAS_REQ
        pres["priority"][p] = prio
    return M.Inputs(prof, t, a, (), pres)


# ------------------------------------------------- directed cases: the overlay
def _hand(n, pods, pres, pdb=(), extra=(), alloc=None) -> M.Inputs:
    """Nodes of 10 CPUs (alloc[i]: of more) whose Requested is their pods' plus extra[i]."""
    a = K.records(pods)
    t = K.table(n, a, extra)
    for i, x in (alloc or {}).items():
        t["alloc0"][i] = x
    return M.Inputs(K.profile(), t, a, tuple(pdb), np.array(pres, abi.PREEMPTOR_DTYPE))


WORD1_PODS = abi.PREEMPT_NODE_PODS


def _word1() -> M.Inputs:
    """The second word of a node's gone mask (list positions 64..127).  Node 0
    has 128 CPUs and 128 pods of 1 CPU; the pod of input index j sits at list
    position 37 j mod 128 (four pods per priority, told apart by their start).
    Preemptor 0 (70 CPUs) removes all, the first 58 fit back: positions 58..127
    are its victims, 64 of them in the second word.  Preemptor 1 (equal
    priority, 10 CPUs) sees the 70 CPUs nominated and the node full again: of
    positions 0..57 the first 48 fit back.  Preemptor 2 (priority above both,
    90 CPUs) sees no nominated pod and 80 CPUs free: of positions 0..47 the
    first 38 fit back.  Reading the second word as 0 in the removal loop leaves
    64 CPUs too many on the row; in the skip test it removes them twice.  Node
    1 (10 CPUs, one pod of priority 900) is UNFIT for 0 and 2 and the worse
    candidate for 1."""
    pods = []
    for j in range(WORD1_PODS):
        pos = (37 * j) % WORD1_PODS
        pods.append(K.A(0, 1000, 400 - pos // 4, pos % 4))
    pods.append(K.A(1, 10000, 900, 0))
    pres = [K.preemptor(70000, prio=1000), K.preemptor(10000, prio=1000), K.preemptor(90000, prio=2000)]
    inp = _hand(2, pods, pres, alloc={0: 128000})
    inp.table["alloc_pods"][0] = 400
    return inp


CHAIN_PRIORITIES = (100, 300, 200, 50, 150)


def _chain() -> M.Inputs:
    """Four preemptors nominated on node 0, whose priorities straddle the
    fifth's.  Node 0: 20 CPUs, 4 requested by others, eight pods of 2 CPUs and
    priorities 1..8.  Node 1: 20 CPUs, one pod of 20 CPUs and priority 90: the
    worse candidate for every preemptor above 90, NO_VICTIMS for the one of 50.

      k  prio  CPUs  sees nominated  node 0 before              victim(s)
      0  100   2     -               20 of 20                   priority 1
      1  300   4     -               18 (0 is below 300)        2
      2  200   2     1               16 + 4                     3
      3   50   2     0, 1, 2         14 + 8 = 22 of 20          5, 4
      4  150   5     1, 2            10 + 6                     6

    Preemptor 4 counting all four nominated pods would lose 8, 7 and 6;
    counting none it would need no victim."""
    pods = [K.A(0, 2000, p, p) for p in range(1, 9)] + [K.A(1, 20000, 90, 0)]
    pres = [K.preemptor(cpu, prio=p) for cpu, p in zip((2000, 4000, 2000, 2000, 5000), CHAIN_PRIORITIES)]
    return _hand(2, pods, pres, extra=[4000], alloc={0: 20000, 1: 20000})


def _budget() -> M.Inputs:
    """One budget of 1.  Nodes 0, 1, 2 are full with one pod of 3 CPUs each
    that matches the PDB (priorities 10, 20, 30); node 3 with one of priority
    500 that does not.  Four preemptors of 3 CPUs and one priority.  The first
    takes node 0 within the budget (1 -> 0).  For the second the pods of nodes
    1 and 2 now violate: node 3 wins by the first level of the key in spite of
    its victim's priority.  The third and the fourth take nodes 1 and 2 with
    one violation each; the budget stays at 0."""
    pods = [K.A(0, 3000, 10, pdb=1), K.A(1, 3000, 20, pdb=1), K.A(2, 3000, 30, pdb=1), K.A(3, 3000, 500)]
    return _hand(4, pods, [K.preemptor(3000) for _ in range(4)], pdb=(1,), extra=[7000] * 4)


def _floor() -> M.Inputs:
    """A quota's used floored at 0.  Node 0: one pod of 6 CPUs the quota counts
    (and 4 CPUs of others); node 1: two pods of 2 CPUs, priorities 40 and 45,
    that the quota does not count (and 6 CPUs of others).  Preemptor 0 (6 CPUs,
    no quota check) takes node 0: 6 CPUs freed.  Preemptors 1 and 2 (2 CPUs)
    state used 5: 5 - 6 is floored at 0.  Preemptor 1 (runtime 6): alone both
    pods of node 1 are victims by quota alone (5 + 2 > 6, and removing them
    moves no used); in sequence 0 + 2 <= 6, the pod of 45 is reprieved and the
    pod of 40 goes only because it does not fit back.  Preemptor 2 (runtime
    1.5) pins the floor itself: with used 0 it is over (0 + 2 > 1.5) and the
    pod of 45 does not fit back beside the nominated preemptor 1: ERROR; with
    used -1 it would not be over (-1 + 2 <= 1.5) and node 1 a candidate."""
    pods = [K.A(0, 6000, 10), K.A(1, 2000, 40, flags=0), K.A(1, 2000, 45, flags=0)]
    pres = [K.preemptor(6000), K.preemptor(2000, used=5000, runtime=6000), K.preemptor(2000, used=5000, runtime=1500)]
    return _hand(2, pods, pres, extra=[4000, 6000])


TILES3_PRE = 65
TILES3_K0 = 45        # the preemptor whose victim spends the budget
TILES3_VICTIM = 1434  # that victim's input index


def _tiles3() -> M.Inputs:
    """Three phase-1 tiles: `clean` with 65 preemptors, each in a quota of its
    own, and one budget of 1.  The PDB's bit is on the first victim of
    preemptor TILES3_K0, in the middle of the second tile, and on every pod of
    the later preemptors' quotas: nothing differs from a run without PDBs up to
    TILES3_K0, whose victim spends the budget; from there on every victim
    violates, every block evaluates again and the third tile's phase 1 is
    skipped."""
    inp = M.inputs("base", 300, TILES3_PRE, M.SEED + 11, False)
    a, pres = inp.assigned, inp.pres
    a["quota"] = (synth.splitmix64(M.SEED + 11, len(a), 730) % np.uint64(TILES3_PRE)).astype(np.int32)
    inq = (a["flags"] & abi.ASG_IN_QUOTA) != 0
    for p in range(len(pres)):
        pres["quota"][p] = p
        pres["q_used"][p] = a["qreq"][inq & (a["quota"] == p)].sum(axis=0)
        pres["q_runtime"][p] = pres["q_used"][p] + pres["q_req"][p] + (1 << 40)
    a["pdb_mask"] = np.where(a["quota"] > TILES3_K0, 1, 0)
    a["pdb_mask"][TILES3_VICTIM] = 1
    return M.Inputs(inp.prof, inp.table, a, (1,), pres)


DIRECTED = {"word1": _word1, "chain": _chain, "budget": _budget, "floor": _floor, "tiles3": _tiles3}
GENERATED = {"clean": _clean, "prio": _prio, **DIRECTED}
CASES = list(M.CASES) + list(GENERATED)


class Model:
    pass


@functools.lru_cache(maxsize=None)
def case(name: str) -> Model:
    """The case's inputs and the expected answers of the sequential dry run.
    Computed once; callers must not modify it."""
    m = Model()
    if name in M.CASES:
        b = M.case(name)
        m.prof, m.table, m.assigned, m.pdb_allowed, m.pres, m.cfg = b.prof, b.table, b.assigned, b.pdb_allowed, b.pres, b.cfg
    else:
        inp = GENERATED[name]()
        m.prof, m.table, m.assigned, m.pdb_allowed, m.pres = inp.prof, inp.table, inp.assigned, inp.pdb_allowed, inp.pres
        m.cfg = to_c_config(inp.prof)
    m.name = name
    m.res, m.chosen, m.stats = stream(m.cfg, m.table, m.assigned, m.pdb_allowed, m.pres)
    return m
