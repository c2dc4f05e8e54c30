"""The hand-worked cases of the preemption dry run, shared by the model's own
tests (test_preempt_model.py) and the device's (test_gpu_preempt_cases.py).

Every case is a named entry of two parts: its inputs (nodes of 10 CPUs, the
assigned records, the PDB budgets, one preemptor) and its expectation, written
out by hand: the verdict of every node as a tuple (status, n_victims,
n_pdb_violations, top_priority, sum_priority, earliest_start), the victims of
every node as input indices in append order, the picked node and the counts
per status.  Nothing here is computed by the model: a test compares the model
or the device with these literals.

WALK     the cases of the per-node walk (SelectVictimsOnNode)
PICK     two candidates whose keys differ first at one level of the pick's
         key; LEVELS orders them as pick_before compares
EXTREME  two candidates whose keys differ in one half of a 64-bit field, in
         sign, or at the ends of the 32-bit priority range
THREE    three equal candidates

contest_cluster() lays many of the two-node cases into one cluster of 16641
nodes (66 workgroups of 256), each at a chosen pair of nodes.
"""
from dataclasses import dataclass, field

import numpy as np

from koordinator_amd import abi
from koordinator_amd.config import PLUGIN_FIT, Profile, to_c_config, with_upstream
from koordinator_amd.snapshot import NodeTable

import preempt_model as M

CAND, NOV, UNFIT, ERR, UNRES = range(5)
B = 1 << 31
ALLOC = 10000
ZERO = (0, 0, 0, 0, 0)
LO = -(1 << 31)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


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


def profile(static=False):
    prof = Profile(filters=(PLUGIN_FIT,), scores={PLUGIN_FIT: 1})
    return with_upstream(prof) if static else prof


def table(n, a, extra=None, static_off=()):
    """n nodes of 10 CPUs whose Requested is their pods' (plus extra[i])."""
    t = NodeTable.empty(n)
    t["alloc0"][:] = ALLOC
    t["alloc1"][:] = 1 << 40
    t["alloc_pods"][:] = 110
    np.add.at(t["requested0"], a["node"], a["pod"]["req"][:, abi.RES_CPU])
    np.add.at(t["nz_cpu_m"], a["node"], a["pod"]["nz_cpu_m"])
    np.add.at(t["npods"], a["node"], 1)
    for i, e in enumerate(extra or ()):
        t["requested0"][i] += e
    for i in static_off:
        t["static_allow"][i] = 0
    return t


def records(pods):
    return np.array(pods, abi.ASSIGNED_DTYPE) if pods else np.zeros(0, abi.ASSIGNED_DTYPE)


@dataclass
class Case:
    # the inputs
    n: int
    pods: list
    pre: np.ndarray
    # the expectation, by hand
    ver: list            # per node (status, n_victims, n_pdb_violations, top_priority, sum_priority, earliest_start)
    vic: list            # per node the victims' input indices in append order
    node: int            # the pick, -1: none
    count: list          # nodes per status
    # the inputs again
    pdb: tuple = ()
    extra: list = None
    static_off: tuple = ()
    lists: list = None   # expected list order per node, where the case is about it

    @property
    def prof(self):
        return profile(bool(self.static_off))

    @property
    def assigned(self):
        return records(self.pods)

    @property
    def table(self):
        return table(self.n, self.assigned, self.extra, self.static_off)

    @property
    def best(self):
        """The picked node's verdict (zeros without a pick)."""
        return self.ver[self.node] if self.node >= 0 else (0,) + ZERO


def run(n, pods, pre, pdb=(), extra=None, static_off=()):
    """The model on such nodes: (verdicts as tuples, victims per node, the pick)."""
    a = records(pods)
    ver, vic, _ = M.select_victims(to_c_config(profile(bool(static_off))), table(n, a, extra, static_off), a, pdb, pre)
    return [tuple(int(x) for x in v) for v in ver], vic, M.pick(ver)


def run_case(c: Case):
    return run(c.n, c.pods, c.pre, c.pdb, c.extra, c.static_off)


def verdict_records(tuples) -> np.ndarray:
    out = np.zeros(len(tuples), abi.PREEMPT_NODE_DTYPE)
    for i, t in enumerate(tuples):
        out[i] = tuple(t)
    return out


def result_record(node, count, best) -> np.ndarray:
    r = np.zeros((), abi.PREEMPT_RESULT_DTYPE)
    r["node"], r["count"] = node, count
    if node >= 0:
        r["best"] = tuple(best)
    return r


# ------------------------------------------------------------------ the walk
WALK = {
    # free 0; without a0 and a1 5 CPUs are free; a0 back leaves 2 (< 3): victim; a1 back leaves 3: reprieved
    "reprieved": Case(1, [A(0, 3000, 100, 10), A(0, 2000, 50, 20), A(0, 4000, 2000, 5)], preemptor(3000), extra=[1000],
                      ver=[(CAND, 1, 0, 100, 100 + B, 10)], vic=[[0]], node=0, count=[1, 0, 0, 0, 0]),
    # a higher priority, another quota, a non-preemptible pod: canPreempt accepts none
    "no_victims": Case(1, [A(0, 3000, 2000), A(0, 3000, 10, quota=1), A(0, 3000, 10, flags=abi.ASG_NONPREEMPTIBLE)],
                       preemptor(3000), ver=[(NOV,) + ZERO], vic=[[]], node=-1, count=[0, 1, 0, 0, 0]),
    # postFilterState.skip: the ids still differ
    "no_victims_skip": Case(1, [A(0, 3000, 10)], preemptor(3000, quota=-1),
                            ver=[(NOV,) + ZERO], vic=[[]], node=-1, count=[0, 1, 0, 0, 0]),
    # equal priority is not lower
    "no_victims_equal_priority": Case(1, [A(0, 3000, 1000)], preemptor(3000, prio=1000),
                                      ver=[(NOV,) + ZERO], vic=[[]], node=-1, count=[0, 1, 0, 0, 0]),
    "unfit": Case(1, [A(0, 500, 0)], preemptor(3000), extra=[9500],
                  ver=[(UNFIT,) + ZERO], vic=[[]], node=-1, count=[0, 0, 1, 0, 0]),
    "unresolvable": Case(2, [A(0, 3000, 10), A(1, 3000, 10)], preemptor(3000), extra=[7000, 7000], static_off=(0,),
                         ver=[(UNRES,) + ZERO, (CAND, 1, 0, 10, 10 + B, 0)], vic=[[], [1]], node=1, count=[1, 0, 0, 0, 1]),
    # a0 does not fit back (removed once) and used 0 + 3000 > runtime 2000 (removed again): RemovePod fails
    "error": Case(1, [A(0, 3000, 100), A(0, 2000, 50)], preemptor(3000, used=5000, runtime=2000), extra=[5000],
                  ver=[(ERR,) + ZERO], vic=[[]], node=-1, count=[0, 0, 0, 1, 0]),
    # both fit back (5 CPUs free without them, the preemptor asks 2); with a0 back used 3000 + 2000 > 4500
    "quota_alone": Case(1, [A(0, 3000, 100, 7), A(0, 2000, 50, 9)], preemptor(2000, used=5000, runtime=4500), extra=[5000],
                        ver=[(CAND, 1, 0, 100, 100 + B, 7)], vic=[[0]], node=0, count=[1, 0, 0, 0, 0]),
    # a pod the quota does not count moves no `used`: with runtime 1999 every pod is over, none is reprieved
    "quota_alone_uncounted": Case(1, [A(0, 3000, 100, 7, flags=0), A(0, 2000, 50, 9)],
                                  preemptor(2000, used=2000, runtime=1999), extra=[5000],
                                  ver=[(CAND, 2, 0, 100, 150 + 2 * B, 7)], vic=[[0, 1]], node=0, count=[1, 0, 0, 0, 0]),
    "pdb_zero": Case(1, [A(0, 3000, 100, 3, pdb=1)], preemptor(3000), pdb=(0,), extra=[7000],
                     ver=[(CAND, 1, 1, 100, 100 + B, 3)], vic=[[0]], node=0, count=[1, 0, 0, 0, 0]),
    # budget 1: the first matching pod is within it, the second violates; a reprieved violating pod counts nothing:
    # a1 (violating) goes first and fits back; a0 does not
    "pdb_one": Case(1, [A(0, 3000, 100, 3, pdb=1), A(0, 1000, 50, 4, pdb=1)], preemptor(3000), pdb=(1,), extra=[6000],
                    ver=[(CAND, 1, 0, 100, 100 + B, 3)], vic=[[0]], node=0, count=[1, 0, 0, 0, 0]),
    # 5 CPUs free without them, the preemptor asks 4: neither fits back; top_priority 50, not the maximum 100
    "violating_first": Case(1, [A(0, 3000, 100, 5), A(0, 2000, 50, 6, pdb=1)], preemptor(4000), pdb=(0,), extra=[5000],
                            ver=[(CAND, 2, 1, 50, 150 + 2 * B, 5)], vic=[[1, 0]], node=0, count=[1, 0, 0, 0, 0]),
    # equal priority: the earlier start first; equal start too: the lower input index first.  The preemptor asks the
    # whole node: all are victims, in that order; the earliest start of the pods of the highest priority (9) is 40
    "list_order": Case(1, [A(0, 1000, 7, 30), A(0, 1000, 7, 20), A(0, 1000, 7, 20), A(0, 1000, 9, 40)], preemptor(ALLOC),
                       ver=[(CAND, 4, 0, 9, 30 + 4 * B, 40)], vic=[[3, 1, 2, 0]], node=0, count=[1, 0, 0, 0, 0],
                       lists=[[3, 1, 2, 0]]),
}


# ------------------------------------------------------------------ the pick
# every pod of these nodes becomes a victim: the preemptor asks the whole node
def two_nodes(pods, ver, vic, node, pdb=()):
    return Case(2, pods, preemptor(ALLOC, prio=1 << 30), pdb=pdb, ver=ver, vic=vic, node=node, count=[2, 0, 0, 0, 0])


PICK = {
    # node 0: one victim of priority -5, the smaller key field by field; node 1: the preemptor fits with its pod back
    "zero": Case(2, [A(0, 3000, -5), A(1, 1000, 10)], preemptor(3000), extra=[7000, 6000],
                 ver=[(CAND, 1, 0, -5, -5 + B, 0), (CAND,) + ZERO], vic=[[0], []], node=1, count=[2, 0, 0, 0, 0]),
    "pdb": two_nodes([A(0, 1000, 100, pdb=1), A(1, 1000, 100)], pdb=(0,),
                     ver=[(CAND, 1, 1, 100, 100 + B, 0), (CAND, 1, 0, 100, 100 + B, 0)], vic=[[0], [1]], node=1),
    "top": two_nodes([A(0, 1000, 200), A(1, 1000, 100), A(1, 1000, 100)],
                     ver=[(CAND, 1, 0, 200, 200 + B, 0), (CAND, 2, 0, 100, 200 + 2 * B, 0)], vic=[[0], [1, 2]], node=1),
    "sum": two_nodes([A(0, 1000, 100), A(0, 1000, 100), A(1, 1000, 100), A(1, 1000, 50)],
                     ver=[(CAND, 2, 0, 100, 200 + 2 * B, 0), (CAND, 2, 0, 100, 150 + 2 * B, 0)],
                     vic=[[0, 1], [2, 3]], node=1),
    # a victim of priority -2^31 adds 0 to the sum: equal sums, three victims against two
    "count": two_nodes([A(0, 1000, 0), A(0, 1000, 0), A(0, 1000, LO), A(1, 1000, 0), A(1, 1000, 0)],
                       ver=[(CAND, 3, 0, 0, 2 * B, 0), (CAND, 2, 0, 0, 2 * B, 0)], vic=[[0, 1, 2], [3, 4]], node=1),
    "start": two_nodes([A(0, 1000, 100, 10), A(0, 1000, 50, 99), A(1, 1000, 100, 20), A(1, 1000, 50, 1)],
                       ver=[(CAND, 2, 0, 100, 150 + 2 * B, 10), (CAND, 2, 0, 100, 150 + 2 * B, 20)],
                       vic=[[0, 1], [2, 3]], node=1),
    "index": two_nodes([A(0, 1000, 100, 10), A(1, 1000, 100, 10)],
                       ver=[(CAND, 1, 0, 100, 100 + B, 10), (CAND, 1, 0, 100, 100 + B, 10)], vic=[[0], [1]], node=0),
}
# the levels in the order pick_before compares them, with the position in preempt_model.pick_key that decides
LEVELS = {"zero": 0, "pdb": 1, "top": 2, "sum": 3, "count": 4, "start": 5, "index": 6}


def _one_each(p0, s0, p1, s1, node):
    """One victim per node: priorities p0 / p1, start times s0 / s1."""
    return two_nodes([A(0, 1000, p0, s0), A(1, 1000, p1, s1)],
                     ver=[(CAND, 1, 0, p0, p0 + B, s0), (CAND, 1, 0, p1, p1 + B, s1)], vic=[[0], [1]], node=node)


H5, H6 = 5 << 32, 6 << 32
EXTREME = {
    # earliest_start: the latest wins.  Were a half of the 64 bits lost on the way the two would tie and the lower
    # index win, so every pair also runs with the better node at the higher index
    "start_high_half": _one_each(100, H5 | 7, 100, H6 | 7, node=1),
    "start_low_half": _one_each(100, H5 | 7, 100, H5 | 8, node=1),
    # the halves disagree: the low word of the later start is the smaller
    "start_halves_disagree": _one_each(100, H5 | 9, 100, H6 | 1, node=1),
    "start_sign": _one_each(100, -1, 100, 0, node=1),
    "start_min_max": _one_each(100, I64_MIN, 100, I64_MAX, node=1),
    "start_min": _one_each(100, I64_MIN, 100, I64_MIN + 1, node=1),
    # sum_priority: 100 + 2^31 + 2^32 against 100 + 2^31, equal low words.  The smaller sum has the more victims
    # (three of priority -2^31 add 0), so with the high word lost the victim count would pick node 0
    "sum_high_half": two_nodes([A(0, 1000, 100), A(0, 1000, 0), A(0, 1000, 0),
                                A(1, 1000, 100), A(1, 1000, LO), A(1, 1000, LO), A(1, 1000, LO)],
                               ver=[(CAND, 3, 0, 100, 100 + B + (1 << 32), 0), (CAND, 4, 0, 100, 100 + B, 0)],
                               vic=[[0, 1, 2], [3, 4, 5, 6]], node=1),
    # 2^32 + 199 against 2^32 + 198
    "sum_low_half": two_nodes([A(0, 1000, 100), A(0, 1000, 99), A(1, 1000, 100), A(1, 1000, 98)],
                              ver=[(CAND, 2, 0, 100, 199 + 2 * B, 0), (CAND, 2, 0, 100, 198 + 2 * B, 0)],
                              vic=[[0, 1], [2, 3]], node=1),
    # 2^32 against 2^31: the low word of the larger sum is the smaller
    "sum_halves_disagree": two_nodes([A(0, 1000, 0), A(0, 1000, 0), A(1, 1000, 0)],
                                     ver=[(CAND, 2, 0, 0, 2 * B, 0), (CAND, 1, 0, 0, B, 0)], vic=[[0, 1], [2]], node=1),
    # top_priority at both ends of what a victim can have below a preemptor of priority 2^30
    "top_lowest": _one_each(LO + 1, 0, LO, 0, node=1),
    "top_highest": _one_each((1 << 30) - 1, 0, (1 << 30) - 2, 0, node=1),
}
# the key position that decides each
EXTREME_LEVEL = {"start_high_half": 5, "start_low_half": 5, "start_halves_disagree": 5, "start_sign": 5,
                 "start_min_max": 5, "start_min": 5, "sum_high_half": 3, "sum_low_half": 3, "sum_halves_disagree": 3,
                 "top_lowest": 2, "top_highest": 2}

# three equal candidates: the lowest index wins
THREE = Case(3, [A(0, 1000, 100, 10), A(1, 1000, 100, 10), A(2, 1000, 100, 10)], preemptor(ALLOC, prio=1 << 30),
             ver=[(CAND, 1, 0, 100, 100 + B, 10)] * 3, vic=[[0], [1], [2]], node=0, count=[3, 0, 0, 0, 0])


def first_difference(c: Case):
    """The first position of the pick's key at which the case's two candidates differ."""
    k0, k1 = (M.pick_key(verdict_records(c.ver)[i], i) for i in (0, 1))
    return next(lv for lv in range(len(k0)) if k0[lv] != k1[lv])


# --------------------------------------------------------- the contest cluster
WG = 256                     # nodes per workgroup of k_preempt
CLUSTER_N = 65 * WG + 1      # 66 workgroups; the last holds the single node n - 1
CLUSTER_BLOCKS = 66


@dataclass
class Contest:
    name: str            # "<case>/<placement>/<lo|hi>"
    case: Case
    placement: str
    nodes: tuple         # the cluster node of the case's node 0, 1 (, 2)
    quota: int           # = its preemptor's index
    base: int            # the cluster input index of the case's pod 0
    # by construction, from the case's hand-written expectation
    node: int = -1       # the winner's cluster node
    best: tuple = ()
    victims: list = field(default_factory=list)
    count: list = field(default_factory=list)


def _place(kind, s):
    """The s-th pair of nodes (lower, higher) of a placement kind; the kinds' regions do not meet."""
    if kind == "wave":       # one wave of workgroup 2, lanes t and 63 - t
        base, t = 2 * WG + 64 * (s // 32), s % 32
        return base + t, base + 63 - t
    if kind == "lanes":      # lanes 63 | 64: the last lane of a wave and the first of the next wave of its workgroup
        k = 12 + s + s // 3  # waves 12, 13, 14, 16, ...: never the last of a workgroup
        return 64 * k + 63, 64 * k + 64
    if kind == "groups":     # nodes 255 | 256: the last node of a workgroup and the first of the next
        g = 40 + s
        return WG * g + 255, WG * g + 256
    if kind == "strided":    # workgroups 0 and 64: the same lane of the pick's strided loop, one trip apart
        return 7 + 2 * s, 64 * WG + 7 + 2 * s
    if kind == "far":        # workgroups 1 and 33: lanes 1 and 33 of the pick meet only at shuffle offset 32
        return WG + 5 * s + 1, 33 * WG + 3 * s + 2
    if kind == "ragged":     # workgroups 0 and 65: lanes 0 and 1 of the pick; n - 1 is the last workgroup's only node
        assert s == 0
        return 3, CLUSTER_N - 1
    raise KeyError(kind)


PLACEMENTS = ("wave", "lanes", "groups", "strided", "far")   # and "ragged", which has room for one contest
THREE_NODES = (15 * WG + 9, 16 * WG + 100, 17 * WG + 200)


class Cluster:
    pass


def contest_cluster() -> Cluster:
    """Inputs: one table of CLUSTER_N otherwise empty nodes, the contests' pods
    (each contest under a quota id of its own) and one preemptor per contest;
    expectation: per contest the winner, its verdict, its victims and the counts."""
    # (name, case, placement, rev).  In every case but "index" node 1 is the better; rev puts it at the lower index
    specs = []
    seq = dict.fromkeys(PLACEMENTS, 0)
    for placement in PLACEMENTS:
        for level in LEVELS:
            for where in ("lo", "hi"):
                specs.append((f"{level}/{placement}/{where}", PICK[level], placement, where == "lo"))
    # workgroup 65 has one node: one contest, whose winner sits there
    specs.append(("start/ragged/hi", PICK["start"], "ragged", False))
    for placement in ("wave", "far"):
        for name, case in EXTREME.items():
            for where in ("lo", "hi"):
                specs.append((f"{name}/{placement}/{where}", case, placement, where == "lo"))
    # interleave the kinds, so that every tile of 32 preemptors holds several
    specs = [specs[i] for i in sorted(range(len(specs)), key=lambda i: (i * 37) % len(specs))]
    specs.insert(50, ("three", THREE, "three", False))

    cl = Cluster()
    cl.contests, pods, pres, extra = [], [], [], {}
    for q, (name, case, placement, rev) in enumerate(specs):
        if placement == "three":
            nodes = THREE_NODES
        else:
            lo, hi_node = _place(placement, seq.get(placement, 0))
            if placement in seq:
                seq[placement] += 1
            nodes = (hi_node, lo) if rev else (lo, hi_node)
        ct = Contest(name, case, placement, nodes, q, len(pods))
        for a in case.pods:
            a = a.copy()
            a["node"], a["quota"] = nodes[int(a["node"])], q
            pods.append(a)
        for i, e in enumerate(case.extra or ()):
            extra[nodes[i]] = e
        pre = case.pre.copy()
        pre["quota"] = q
        pres.append(pre)
        # equal keys: the lower cluster index wins, wherever the case's node 0 went
        w = int(np.argmin(nodes)) if first_difference(case) == LEVELS["index"] else case.node
        ct.node, ct.best = nodes[w], case.ver[w]
        ct.victims = [ct.base + j for j in case.vic[w]]
        ct.count = [case.n, CLUSTER_N - case.n, 0, 0, 0]
        cl.contests.append(ct)
    cl.prof = profile()
    cl.cfg = to_c_config(cl.prof)
    cl.assigned = records(pods)
    cl.pres = np.array(pres, abi.PREEMPTOR_DTYPE)
    cl.pdb_allowed = (0,)    # one global budget of 0; only the "pdb" contests' pods carry its bit
    cl.table = table(CLUSTER_N, cl.assigned)
    for i, e in extra.items():
        cl.table["requested0"][i] += e
    cl.max_victims = max(len(ct.victims) for ct in cl.contests)
    cl.res = np.array([result_record(ct.node, ct.count, ct.best) for ct in cl.contests], abi.PREEMPT_RESULT_DTYPE)
    cl.victims = M.victims_array([ct.victims for ct in cl.contests], cl.max_victims)
    return cl
