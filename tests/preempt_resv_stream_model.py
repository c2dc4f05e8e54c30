"""The sequential preemption dry run under Reservation
(koordhip_preempt_stream_resv in the KOORDHIP_PREEMPT_RESV mode):
preempt_stream_model.stream's sequence with preempt_resv_model.ResvRule's state.

S_k is preempt_stream_model's (gone pods off the rows and out of the lists,
nominated preemptors of preemptor k's priority and above on the rows, budgets
and quota lowered), and for (preemptor k, node) the RESV walk changes so:

    gone        a gone listed pod bound to slot q has left its reservation:
                Allocated[q][c] = max(0, Allocated[q][c] - req[c]) for c in
                {cpu, memory} where the slot holds c, the assigned count drops
                by one, floored at 0 (RemoveAssignedPod)
    class       class, restore and podRequested are those of the lowered slots
    once        an AllocateOnce slot that had an assigned pod on S_0 stays class
                0 for the whole call (the reference marks it Succeeded)
    order       gone pods off row and slots, restore, podRequested frozen
                WITHOUT any nominated pod, then the nominated pods onto the row
    nominated   AddPod of every qualifying nominated pod on a CLONE of the
                state at every fit test: Pn_eff = max(0, Pn - N); Pr untouched
    two passes  on a node with a qualifying nominated pod "fits" is
                T(row + nominated, Pn_eff) and then T(row, Pn)

Computed twice.  stream() is the overlay form: preempt_stream_model.stream with
a rule per preemptor (StreamResvRule) that starts ResvRule's state from S_k.
rebuilt() is the restatement from scratch: for preemptor k a table of its own
with V_0..V_{k-1} deleted from rows, lists, slot Allocated and assigned counts,
budgets floored, q_used lowered and NO nominated pod on any row; on it one walk
(NominatedRule) takes the nominated pods as an explicit list and restates
RunFilterPluginsWithNominatedPods: clone, AddPod per pod, Filter, second pass.
case() asserts that both agree on every verdict of every node, the pick and the
victims.

The table has no phase column, so the rebuilt table carries the AllocateOnce
rule by the count: such a slot's assigned count is not lowered below 1.  The
overlay form states the rule directly (the slot is out).

The engine builds the call as the per-preemptor chain, so its
koordhip_preempt_stream_stats follow from the results by chain_stats().
"""
import functools
from unittest import mock

import numpy as np

import oracle
from koordinator_amd import abi
from koordinator_amd.config import to_c_config
from koordinator_amd.snapshot import slot_col

import preempt_cases as K
import preempt_dev_stream_model as DS
import preempt_model as M
import preempt_resv_model as V
import preempt_stream_model as S
import reasons_model as R

NRES = abi.NRES
BRANCHES = {}          # branch name -> times taken (the coverage conditions read it)
NAMED = ("allocated_freed", "class_drops", "once_stays_out", "unmasked", "floor", "nominated_pn", "second_pass",
         "below_priority")
KEYS = (abi.RESV_KEY_CPU, abi.RESV_KEY_MEM)


def _took(name):
    BRANCHES[name] = BRANCHES.get(name, 0) + 1


chain_stats = DS.chain_stats
claimed_twice = DS.claimed_twice


# ------------------------------------------------------------ the slots of S_k
def once_slots(table):
    """(node, slot) of the AllocateOnce slots that have an assigned pod on S_0."""
    out = set()
    for q in range(max(1, table.resv_slots)):
        f, cnt = table[slot_col("resv_flags", q)], table[slot_col("resv_assigned", q)]
        for i in np.flatnonzero(((f & abi.RESV_PRESENT) != 0) & ((f & abi.RESV_ALLOCATE_ONCE) != 0) & (cnt > 0)):
            out.add((int(i), q))
    return out


def lowered(table, assigned, gone):
    """A copy of `table` whose slots the gone pods (indices of `assigned`) have left: RemoveAssignedPod."""
    t = table.copy()
    for j in gone:
        a = assigned[j]
        i, q = int(a["node"]), V.bound_slot(a)
        if q < 0:
            continue
        f = int(t[slot_col("resv_flags", q)][i])
        for k in range(2):
            req = int(a["pod"]["req"][k])
            if not f & KEYS[k]:
                if req:
                    _took("unmasked")
                continue
            col = t[slot_col(f"resv_allocated{k}", q)]
            if int(col[i]) < req:
                _took("floor")
            col[i] = max(0, int(col[i]) - req)
        cnt = t[slot_col("resv_assigned", q)]
        cnt[i] = max(0, int(cnt[i]) - 1)
    return t


def _move(t, i, pod, sign):
    for r in range(NRES):
        t[f"requested{r}"][i] += sign * int(pod["req"][r])
    t["nz_cpu_m"][i] += sign * int(pod["nz_cpu_m"])
    t["nz_mem"][i] += sign * int(pod["nz_mem"])
    t["npods"][i] += sign


def _status_at(rows, i, pods, sign):
    """The oracle's status of node i's hypothetical row with `pods` added (sign +1) or taken off (-1)."""
    t = rows.table.copy()
    for c in M.ROW_COLS:
        t[c][:] = rows.cols[c]
    for pod in pods:
        _move(t, i, pod, sign)
    return int(oracle.Oracle(rows.cfg, t).eval(rows.pod, status=True, scores=False)["status"][0][i])


def _index_of(assigned, a):
    return int((a.__array_interface__["data"][0] - assigned.__array_interface__["data"][0]) // assigned.itemsize)


# ------------------------------------------------------------ the overlay form
class StreamResvRule(V.ResvRule):
    """ResvRule started from S_k.  `table` is what preempt_stream_model.stream
    moved: S_0's rows without the gone pods and WITH the qualifying nominated
    pods, S_0's slots.  gone: table indices; nominated: (node, pod, priority);
    once_out: once_slots(S_0)."""

    def __init__(self, cfg, table, pre, rows, literal=True, base_cfg=None, assigned=None, gone=(), nominated=(),
                 once_out=frozenset()):
        n = table.n
        self.rows, self.literal, self.assigned = rows, literal, assigned
        self.pod = V.pod_record(pre["pod"])
        prio = int(pre["priority"])
        self.nom = [[] for _ in range(n)]             # the qualifying nominated pods per node
        for i, pod, p in nominated:
            if p < prio:
                _took("below_priority")
                continue
            self.nom[i].append(pod)
        # the snapshot NodeInfo of S_k: the slots the gone pods have left, the rows without any nominated pod
        low = lowered(table, assigned, gone)
        snap = low.copy()
        for i, q in once_out:
            snap[slot_col("resv_flags", q)][i] = 0    # Succeeded: never Available again
        bound_nodes = sorted({int(assigned["node"][j]) for j in gone if V.bound_slot(assigned[j]) >= 0})
        slots0 = {i: V.slots_of(table, i) for i in bound_nodes}       # as they were on S_0
        # (`table` is rows.table, this preemptor's own copy: the oracle restores the rows it is given by the
        # table's slots, so the hypothetical rows get S_k's)
        for q in range(max(1, table.resv_slots)):
            for col in ("resv_flags", "resv_allocated0", "resv_allocated1", "resv_assigned"):
                table[slot_col(col, q)][:] = snap[slot_col(col, q)]
        for i in range(n):
            for pod in self.nom[i]:
                _move(snap, i, pod, -1)
        self.info = [V.node_state(snap, i, self.pod) for i in range(n)]
        self.alloc = [[int(table[f"alloc{k}"][i]) for k in range(NRES)] for i in range(n)]
        self.alloc_pods = [int(table["alloc_pods"][i]) for i in range(n)]
        self.state = [V.PreState() for _ in range(n)]
        self.resv_on = bool(int(cfg.filter_plugins) & abi.PLUGIN_RESERVATION)
        self.out = [set() for _ in range(n)]          # the listed pods off node i at the moment
        # where a gone pod was bound: what the slots were on S_0, for the named situations
        self.rd0 = {}
        for i in bound_nodes:
            s0, s1, sl = slots0[i], V.slots_of(snap, i), V.slots_of(low, i)
            for q, (a, b) in enumerate(zip(s0, s1)):
                if (i, q) in once_out:
                    if V.slot_class(sl[q], self.pod) == 1:    # it has no assigned pod left and would match
                        _took("once_stays_out")
                    continue
                if V.slot_class(a, self.pod) == 2 and V.slot_class(b, self.pod) == 0:
                    _took("class_drops")
                if a["rd"] != b["rd"]:
                    self.rd0[(i, q)] = a["rd"]
        # UNRESOLVABLE: the start row of S_k with the qualifying nominated pods on it
        start = V.without_reservation(table, np.array([x[2] for x in self.info], np.int64),
                                      np.array([x[3] for x in self.info], np.int32))
        mask = R.masks(oracle.Oracle(base_cfg if base_cfg is not None else cfg, start),
                       np.ascontiguousarray(pre["pod"].reshape(1)))[0]
        self.first = abi.first_reasons(mask)

    def _filter(self, i, npods, st, matched=None):
        nrs, m, _, dn = self.info[i]
        node = {"alloc": self.alloc[i], "alloc_pods": self.alloc_pods[i], "npods": npods + dn}
        return V.filter_with_reservations(self.pod, node, nrs, m if matched is None else matched, st)

    def _pn_eff(self, i):
        st = self.state[i]
        n_sum = [sum(int(pod["req"][k]) for pod in self.nom[i]) for k in range(NRES)]
        clone = V.PreState()
        clone.pn = [max(0, a - b) for a, b in zip(st.pn, n_sum)]
        clone.pr = {q: list(v) for q, v in st.pr.items()}
        return clone

    def resv_reason(self, i):
        """The first pass: on the row with the nominated pods, preemptible[node] lowered by their AddPod."""
        if not self.resv_on:
            return None
        npods = int(self.rows.cols["npods"][i])
        st = self.state[i]
        if not self.nom[i]:
            got = self._filter(i, npods, st)
        else:
            got = self._filter(i, npods, self._pn_eff(i))
            if got != self._filter(i, npods, st):
                _took("nominated_pn")
        if got is None and any(k[0] == i for k in self.rd0):
            # with the gone pods still in Allocated a Restricted slot would have refused
            nrs, matched, _, _ = self.info[i]
            old = [(q, dict(s, rd=self.rd0.get((i, q), s["rd"]))) for q, s in matched]
            if any(s["policy"] == abi.RESV_POLICY_RESTRICTED for _, s in matched) and \
                    self._filter(i, npods, st if not self.nom[i] else self._pn_eff(i), old) is not None:
                _took("allocated_freed")
        return got

    def fits(self, status, i):
        if not super().fits(status, i):
            return False
        if not self.nom[i]:
            return True
        # the second pass: the row and the plugin's state without the nominated pods
        st2 = _status_at(self.rows, i, self.nom[i], -1)
        ok = (st2 & ~abi.ST_RESV_FAIL) == 0 and \
            (not self.resv_on or self._filter(i, int(self.rows.cols["npods"][i]) - len(self.nom[i]), self.state[i]) is None)
        if not ok:
            _took("second_pass")
        return ok

    def moved(self, i, a, sign):
        j = _index_of(self.assigned, a)
        (self.out[i].add if sign < 0 else self.out[i].discard)(j)
        super().moved(i, a, sign)


class _Sequence:
    """The rule of preempt_stream_model.stream's k-th select_victims call.  What
    the sequence decided for k - 1 (its pick, read where stream() calls
    preempt_model.pick; its victims, the pods off the picked node when the walk
    ended) is settled when the rule of k is made."""

    def __init__(self, table, assigned, pres, base_cfg, literal=True):
        self.assigned, self.pres, self.base_cfg, self.literal = assigned, pres, base_cfg, literal
        self.once_out = frozenset(once_slots(table))
        self.gone, self.nominated, self.verdicts = [], [], []
        self.rule, self.node = None, -1

    def __call__(self, cfg, table, pre, rows):
        k = len(self.verdicts)
        if self.rule is not None and self.node >= 0:
            self.gone += sorted(self.rule.out[self.node])
            self.nominated.append((self.node, self.pres[k - 1]["pod"].copy(), int(self.pres[k - 1]["priority"])))
        self.rule = StreamResvRule(cfg, table, pre, rows, literal=self.literal, base_cfg=self.base_cfg,
                                   assigned=self.assigned, gone=tuple(self.gone), nominated=tuple(self.nominated),
                                   once_out=self.once_out)
        return self.rule

    def picked(self, verdicts, res):
        self.verdicts.append(verdicts.copy())
        self.node = int(res["node"])


def stream(cfg, table, assigned, pdb_allowed, pres, base_cfg=None):
    """(results, full victim lists per preemptor, stats, verdicts [p][n]).  cfg: the profile with the Reservation
    plugin; base_cfg: without it (for the start rows' reasons)."""
    seq = _Sequence(table, assigned, pres, base_cfg)
    pick = M.pick

    def observed(verdicts):
        res = pick(verdicts)
        seq.picked(verdicts, res)
        return res

    with mock.patch.object(M, "pick", observed):
        res, chosen, stats = S.stream(cfg, table, assigned, pdb_allowed, pres, rule=seq)
    ver = np.array(seq.verdicts, abi.PREEMPT_NODE_DTYPE).reshape(len(pres), table.n)
    return res, chosen, chain_stats(stats, table.n, len(pres)), ver


# --------------------------------------------------- the restatement from scratch
def rebuilt_inputs(table, assigned, pdb_allowed, pres, k, chosen, nodes):
    """S_k as a table of its own: V_0..V_{k-1} deleted from rows, lists, slot
    Allocated and assigned counts (an AllocateOnce slot with an assigned pod on
    S_0 keeps a count of at least 1), budgets floored, q_used lowered, and no
    nominated pod on any row.  (table, assigned, budgets, preemptor k, keep: the
    rebuilt array's indices in `assigned`, nominated: (node, pod, priority) of
    every earlier preemptor that found a node)."""
    allowed = [int(x) for x in pdb_allowed]
    pre = pres[k].copy()
    quota = int(pre["quota"])
    freed = [0] * abi.PREEMPT_QRES
    gone, nominated = [], []
    for j in range(k):
        if nodes[j] < 0:
            continue
        for v in chosen[j]:
            a = assigned[v]
            gone.append(int(v))
            for b in range(len(allowed)):
                if (int(a["pdb_mask"]) >> b) & 1:
                    allowed[b] = max(0, allowed[b] - 1)
            if quota >= 0 and int(pres[j]["quota"]) == quota and int(a["flags"]) & abi.ASG_IN_QUOTA:
                for d in range(abi.PREEMPT_QRES):
                    freed[d] += int(a["qreq"][d])
        nominated.append((nodes[j], pres[j]["pod"].copy(), int(pres[j]["priority"])))
    t = lowered(table, assigned, gone)
    for i, q in once_slots(table):
        cnt = t[slot_col("resv_assigned", q)]
        cnt[i] = max(1, int(cnt[i]))
    for v in gone:
        _move(t, int(assigned["node"][v]), assigned["pod"][v], -1)
    for d in range(abi.PREEMPT_QRES):
        pre["q_used"][d] = max(0, int(pre["q_used"][d]) - freed[d])
    keep = np.setdiff1d(np.arange(len(assigned)), np.array(gone, np.int64))
    return t, np.ascontiguousarray(assigned[keep]), tuple(allowed), np.array([pre], abi.PREEMPTOR_DTYPE), keep, nominated


class NominatedRule(V.ResvRule):
    """ResvRule on a rebuilt table (its rows hold no nominated pod) with the
    node's nominated pods as an explicit list: every fit test is
    RunFilterPluginsWithNominatedPods."""

    def __init__(self, cfg, table, pre, rows, literal=True, base_cfg=None, nominated=()):
        super().__init__(cfg, table, pre, rows, literal=literal, base_cfg=base_cfg)
        prio = int(pre["priority"])
        self.nom = [[] for _ in range(table.n)]
        for i, pod, p in nominated:
            if p >= prio:                             # addNominatedPods: priority >= the pod's
                self.nom[i].append(pod)
        # UNRESOLVABLE is decided on the start row with the nominated pods on it
        with_nom = table.copy()
        for i in range(table.n):
            for pod in self.nom[i]:
                _move(with_nom, i, pod, +1)
        start = V.without_reservation(with_nom, np.array([x[2] for x in self.info], np.int64),
                                      np.array([x[3] for x in self.info], np.int32))
        mask = R.masks(oracle.Oracle(base_cfg if base_cfg is not None else cfg, start),
                       np.ascontiguousarray(pre["pod"].reshape(1)))[0]
        self.first = abi.first_reasons(mask)

    def _run_filters(self, status, i, npods, st):
        if (status & ~abi.ST_RESV_FAIL) != 0:
            return False
        if not self.resv_on:
            return True
        nrs, matched, _, dn = self.info[i]
        node = {"alloc": self.alloc[i], "alloc_pods": self.alloc_pods[i], "npods": npods + dn}
        return V.filter_with_reservations(self.pod, node, nrs, matched, st) is None

    def fits(self, status, i):
        npods = int(self.rows.cols["npods"][i])
        added, ok = self.nom[i], False
        for p in range(2):
            if p == 0:
                # addNominatedPods: the NodeInfo and the cycle state cloned, AddPod of every nominated pod
                st = V.PreState()
                st.pn, st.pr = list(self.state[i].pn), {q: list(v) for q, v in self.state[i].pr.items()}
                for pod in added:
                    V.add_pod(st, [int(x) for x in pod["req"]], -1, self.literal)
                ok = self._run_filters(_status_at(self.rows, i, added, +1) if added else status, i,
                                       npods + len(added), st)
            elif not added or not ok:
                break
            else:
                ok = self._run_filters(status, i, npods, self.state[i])
        return ok

    def unresolvable(self, i):
        if self.first[i]:
            return bool(self.first[i] & abi.REASON_UNRESOLVABLE_MASK)
        return self.resv_on and not self.info[i][1] and self.pod["affinity"]


def rebuilt(cfg, base_cfg, table, assigned, pdb_allowed, pres, k, chosen, nodes):
    """Preemptor k alone on that table: (result, verdicts [n], victims as indices of `assigned`)."""
    t, a_k, allowed, pre, keep, nominated = rebuilt_inputs(table, assigned, pdb_allowed, pres, k, chosen, nodes)
    ver, vic, _ = M.select_victims(cfg, t, a_k, allowed, pre[0], None,
                                   functools.partial(NominatedRule, base_cfg=base_cfg, nominated=tuple(nominated)))
    res = M.pick(ver)
    c = int(res["node"])
    return res, ver, [int(keep[j]) for j in vic[c]] if c >= 0 else []


def check_rebuilt(cfg, base_cfg, table, assigned, pdb_allowed, pres, res, chosen, ver):
    """The overlay form's answers are the rebuilt tables': every verdict of every node, the pick, the victims."""
    nodes = [int(x) for x in res["node"]]
    for k in range(len(pres)):
        r, v, vic = rebuilt(cfg, base_cfg, table, assigned, pdb_allowed, pres, k, chosen, nodes)
        assert v.tobytes() == ver[k].tobytes(), f"preemptor {k}: verdicts differ at node " \
            f"{int(np.flatnonzero(v != ver[k])[0])}"
        assert r.tobytes() == res[k].tobytes(), f"preemptor {k}: pick {r} against {res[k]}"
        assert vic == [int(j) for j in chosen[k]], f"preemptor {k}: victims {vic} against {chosen[k]}"


# ------------------------------------------------------------ hand-worked cases
# Nodes of 10 CPUs, the profile Fit + Reservation, cpu-only slots, preempt_resv_model's helpers.  As there, a
# reserve pod's Allocatable is part of the row, so two Default slots of 3 CPUs put 6 CPUs on it.
def _many(t, a, pres) -> M.Inputs:
    return M.Inputs(V._directed_profile(), t, a, (), np.array(pres, abi.PREEMPTOR_DTYPE))


def _allocated_freed(mem=0, rd=4000, second=4000) -> M.Inputs:
    """A gone pod's Allocated is free for the next preemptor.  preempt_resv_model's
    `restricted` node: a Restricted slot of 4 CPUs, all allocated to its one
    assigned pod, pod 0 (4 CPUs, priority 10, bound); pod 1 (2 CPUs, priority
    20).  Requested 4 + 4 + 2 = 10000.  Preemptors 0 (priority 1000) and 1
    (priority 2000) ask 4 CPUs and match.

    Preemptor 0 is `restricted`: pod 0 is its victim.  Alone, preemptor 1 answers
    the same: both claim pod 0.
    In sequence preemptor 1 does not see preemptor 0 (1000 < 2000).  Pod 0 is
    gone: Requested 6000, Allocated 4000 - 4000 = 0, no assigned pod.  Start row
    6000 - 4000 = 2000, podRequested 6000, rRemained 4000.  Pod 1 removed: Pn =
    2000: fitsNode 4000 > 10000 - (6000 - 4000 - 2000): fits; Restricted 4000 <=
    4000 - 0: passes.  Pod 1 back: fitsNode 4000 > 10000 - 2000: fits,
    Restricted as before: reprieved: no victim.  With Allocated still 4000 the
    slot would refuse (4000 > 0) and the node with it."""
    a = K.records([V._bound(K.A(0, 4000, 10, start=1), 0), K.A(0, 2000, 20, start=2)])
    if mem:
        a["pod"]["req"][:, abi.RES_MEM] = a["pod"]["nz_mem"] = mem
    t = V._table(a)
    if mem:
        t["requested1"][0] = t["nz_mem"][0] = 2 * mem
    V._slot(t, 0, 0, abi.RESV_POLICY_RESTRICTED, 4000, rd, 1)
    return _many(t, a, [V._pre(4000, prio=1000), V._pre(second, prio=2000)])


def _unmasked() -> M.Inputs:
    """`allocated_freed` with 1 GiB of memory on either listed pod.  The slot
    holds cpu only: Mask(requests, ResourceNames) drops the gone pod's memory, the
    slot's memory Allocated (0) is not touched and nothing floors.  The answers
    are `allocated_freed`'s.  (Under NodeResourcesFit a cpu-only slot's memory
    Allocated can only make fitsNode more lenient than Fit, so no verdict can
    show it; test_preempt_resv_stream_model.py pins lowered() on such a slot.)"""
    return _allocated_freed(mem=1 << 30)


def _floor() -> M.Inputs:
    """`allocated_freed` with Allocated 3000, less than its only assigned pod's
    4 CPUs; preemptor 1 asks 5 CPUs.

    Preemptor 0: start row 6000, podRequested 10000, rAllocated 3000, rRemained
    1000.  Both removed: Pn = 2000, Pr[0] = 4000: fitsNode 4000 > 10000 - (10000 -
    4000 - 6000): fits; Restricted: a = max(0, 3000 - 4000) = 0, 4000 <= 4000:
    passes.  Pod 1 back: fits: reprieved.  Pod 0 back: Pr[0] deleted: a = 3000,
    4000 > 1000: insufficient: pod 0 is the victim.
    Preemptor 1: Allocated = max(0, 3000 - 4000) = 0.  Start row 2000: Fit 5000 <=
    8000 passes, Restricted 5000 > 4000 - 0: insufficient.  Pod 1 removed: the
    same: UNFIT, no node.  Allocated -1000 would leave 5000: the slot and the
    node would pass."""
    return _allocated_freed(rd=3000, second=5000)


def _class_drops() -> M.Inputs:
    """An unmatched slot loses its only assigned pod.  Slot 0: Default, owner
    group 1 (no preemptor matches), 4 CPUs, Allocated 3000 (the host's figure; the
    listed pod requests 2000), one assigned pod: pod 0 (2 CPUs, priority 10,
    bound, counted by the quota).  Pod 1 (3 CPUs, priority 20), 1 CPU of others.
    Requested 4 + 2 + 3 + 1 = 10000.

    Preemptor 0 (priority 15, 1 CPU, used 2000 of runtime 2500): the slot is class
    2: the reserve pod leaves, its remainder 1000 comes back: start row 7000.
    Pod 0 is removed and fits back, but used 2000 + 1000 > 2500: a victim by
    quota alone.
    Preemptor 1 (priority 1000, 3 CPUs, no quota check) alone: start row 7000.
    Both removed, pod 1 back: Pn = 0, Pr[0] present: fitsNode(nil) 3000 > 10000 -
    7000 is false: fits; pod 0 back: nothing present, Fit 3000 <= 3000: no victim.
    In sequence it does not see preemptor 0 (15 < 1000).  Pod 0 is gone: Requested
    8000, Allocated 1000, no assigned pod: class 0, no restore: start row 8000,
    1000 above the independent one.  Pod 1 removed: Fit 3000 <= 5000; back: 3000
    > 2000: pod 1 is the victim."""
    a = K.records([V._bound(K.A(0, 2000, 10, start=1), 0), K.A(0, 3000, 20, start=2)])
    t = K.table(1, a, extra=[1000])
    t.set_resv_slots(1)
    V._slot(t, 0, 0, abi.RESV_POLICY_DEFAULT, 4000, 3000, 1, group=1)
    first = V._pre(1000, match=False, prio=15)
    first["q_used"][0], first["q_mask"], first["q_runtime"][0] = 2000, 1, 2500
    return _many(t, a, [first, V._pre(3000, match=False, prio=1000)])


def _once_stays_out() -> M.Inputs:
    """A matched AllocateOnce slot stays out.  Slot 0: Default, AllocateOnce, 4
    CPUs, all allocated to its one assigned pod, pod 0 (4 CPUs, priority 10,
    bound); pod 1 (2 CPUs, priority 20).  Requested 10000.  With an assigned pod
    the slot is class 0 for everybody: no restore, no nodeRState.

    Preemptor 0 (priority 1000, 4 CPUs, matches): both removed: Fit 4000 <= 6000;
    pod 1 back: 4000 <= 4000: reprieved; pod 0 back: victim.
    Preemptor 1 (priority 2000, 6 CPUs, matches) does not see preemptor 0.  Pod 0
    is gone, Requested 6000; the slot is Succeeded and stays class 0: start row
    6000.  Pod 1 removed: 6000 <= 6000; back: 6000 > 4000: pod 1 is the victim.
    As a class-1 slot again it would be restored (row 2000) and pod 1 reprieved."""
    a = K.records([V._bound(K.A(0, 4000, 10, start=1), 0), K.A(0, 2000, 20, start=2)])
    t = V._table(a)
    V._slot(t, 0, 0, abi.RESV_POLICY_DEFAULT, 4000, 4000, 1, once=True)
    return _many(t, a, [V._pre(4000, prio=1000), V._pre(6000, prio=2000)])


def _two_default(p0, p1, extra, pres) -> M.Inputs:
    """preempt_resv_model's `default` node: two Default slots of 3 CPUs, nothing allocated, both matched; pod 0
    (priority 10) and pod 1 (priority 20), neither bound.  Per slot fitsNode gives back that slot's remainder only."""
    a = K.records([K.A(0, p0, 10, start=1), K.A(0, p1, 20, start=2)])
    t = K.table(1, a, extra=[extra])
    t.set_resv_slots(2)
    V._slot(t, 0, 0, abi.RESV_POLICY_DEFAULT, 3000, 0, 0)
    V._slot(t, 0, 1, abi.RESV_POLICY_DEFAULT, 3000, 0, 0)
    return _many(t, a, pres)


def _nominated_pn(second_prio=1000) -> M.Inputs:
    """A nominated pod lowers preemptible[node].  Pod 0 of 3 CPUs, pod 1 of 4, 1
    CPU of others: Requested 6 + 3 + 4 + 1 = 14000.  Preemptor 0 (priority 1000,
    2.5 CPUs), preemptor 1 (priority 1000, 5 CPUs).

    Preemptor 0: podRequested 14000, start row 8000 (Fit 2500 > 2000).  Both
    removed: Pn = 7000: fitsNode 2500 > 10000 - (14000 - 3000 - 7000) is false.
    Pod 1 back: Pn = 3000: 2500 > 10000 - 8000: both slots insufficient: victim.
    Pod 0 back: Pn = 4000: 2500 > 10000 - 7000 is false: reprieved.
    Preemptor 1 sees preemptor 0 (1000 >= 1000), N = 2500.  Pod 1 is gone:
    podRequested 10000 (frozen without the nominated pod), start row 10000 - 6000
    + 2500 = 6500.  Pod 0 removed: Pn = 3000, in the clone Pn_eff = 500: fitsNode
    5000 > 10000 - (10000 - 3000 - 500) = 3500: both slots insufficient: UNFIT,
    no node.  With Pn itself: 5000 > 6000 is false in both passes, and pod 0
    would be its victim."""
    return _two_default(3000, 4000, 1000, [V._pre(2500, prio=1000), V._pre(5000, prio=second_prio)])


def _below_priority() -> M.Inputs:
    """`nominated_pn` with preemptor 1 at priority 2000: it does not see
    preemptor 0 (1000 < 2000), neither on the row nor in Pn.  Start row 4000 (Fit
    5000 <= 6000).  Pod 0 removed: Pn = 3000: fitsNode 5000 > 10000 - (10000 -
    3000 - 3000) is false; back: nothing present, Fit passes: no victim."""
    return _nominated_pn(second_prio=2000)


def _second_pass() -> M.Inputs:
    """The second pass fails where the first passes.  Pod 0 of 1 CPU, pod 1 of 4,
    4 CPUs of others: Requested 6 + 1 + 4 + 4 = 15000.  Preemptor 0 (priority
    1000, 2 CPUs), preemptor 1 (priority 1000, 4 CPUs).

    Preemptor 0: podRequested 15000, start row 9000 (Fit 2000 > 1000).  Both
    removed: Pn = 5000: fitsNode 2000 > 10000 - 7000 is false.  Pod 1 back: Pn =
    1000: 2000 > 10000 - 11000: insufficient: victim.  Pod 0 back: Pn = 4000: 2000
    > 10000 - 8000 is false: reprieved.
    Preemptor 1: N = 2000, podRequested 11000, start row 11000 - 6000 + 2000 = 7000
    (Fit 4000 > 3000).  Pod 0 removed: row 6000, Pn = 1000.  First pass: Pn_eff =
    max(0, 1000 - 2000) = 0 is absent and no Pr is present: no Default slot is
    tested, Fit 4000 <= 4000: passes.  Second pass: row 4000, Pn = 1000 is
    present: fitsNode 4000 > 10000 - (11000 - 3000 - 1000) = 3000: both slots
    insufficient: UNFIT, no node.  One pass would go on and take pod 0."""
    return _two_default(1000, 4000, 4000, [V._pre(2000, prio=1000), V._pre(4000, prio=1000)])


_DIRECTED = {"allocated_freed": _allocated_freed, "class_drops": _class_drops, "once_stays_out": _once_stays_out,
             "unmasked": _unmasked, "floor": _floor, "nominated_pn": _nominated_pn, "second_pass": _second_pass,
             "below_priority": _below_priority}
DIRECTED = tuple(_DIRECTED)
# by hand: per preemptor (node, victims in append order)
EXPECTED = {
    "allocated_freed": [(0, [0]), (0, [])],
    "class_drops": [(0, [0]), (0, [1])],
    "once_stays_out": [(0, [0]), (0, [1])],
    "unmasked": [(0, [0]), (0, [])],
    "floor": [(0, [0]), (-1, [])],
    "nominated_pn": [(0, [1]), (-1, [])],
    "second_pass": [(0, [1]), (-1, [])],
    "below_priority": [(0, [1]), (0, [])],
}
# ... and of the independent batch (koordhip_preempt in the RESV mode), where it is part of the case's point
EXPECTED_INDEPENDENT = {
    "allocated_freed": [(0, [0]), (0, [0])],
    "class_drops": [(0, [0]), (0, [])],
}


def _ascending() -> M.Inputs:
    """`wave`'s shape with six preemptors of strictly ascending priorities: no
    preemptor sees an earlier one, so S_k differs from S_0 by the gone pods alone
    and the rebuilt table alone says all of it (the device runs koordhip_preempt
    on it)."""
    inp = V.inputs(130, 6, M.SEED + 40, 1, False, False)
    order = np.argsort(inp.pres["priority"], kind="stable")
    pres = inp.pres[order].copy()
    pres["priority"] += np.arange(len(pres), dtype=pres["priority"].dtype)
    assert (np.diff(pres["priority"]) > 0).all()
    return M.Inputs(inp.prof, inp.table, inp.assigned, inp.pdb_allowed, pres)


GENERATED = tuple(V.CASES)                        # preempt_resv_model.CASES' shapes
ALL_CASES = list(GENERATED) + ["ascending"] + list(DIRECTED)


class Model:
    pass


@functools.lru_cache(maxsize=None)
def case(name: str) -> Model:
    """The case's inputs and the expected answers of koordhip_preempt_stream_resv
    in the RESV mode, in both forms.  Computed once; callers must not modify it."""
    if name in _DIRECTED:
        inp = _DIRECTED[name]()
    elif name == "ascending":
        inp = _ascending()
    else:
        inp = V.inputs(*V.CASES[name])
    m = Model()
    m.name, m.prof, m.table, m.assigned, m.pdb_allowed, m.pres = name, inp.prof, inp.table, inp.assigned, inp.pdb_allowed, inp.pres
    m.cfg = to_c_config(inp.prof)
    m.base_cfg = to_c_config(V.without_plugin(inp.prof))
    before = dict(BRANCHES)
    m.res, m.chosen, m.stats, m.verdicts = stream(m.cfg, m.table, m.assigned, m.pdb_allowed, m.pres, m.base_cfg)
    m.branches = {k: v - before.get(k, 0) for k, v in BRANCHES.items() if v - before.get(k, 0)}
    check_rebuilt(m.cfg, m.base_cfg, m.table, m.assigned, m.pdb_allowed, m.pres, m.res, m.chosen, m.verdicts)
    nodes = [int(x) for x in m.res["node"]]
    prio = [int(x) for x in m.pres["priority"]]
    # per preemptor: a pod bound to a reservation is gone before it; some earlier placed preemptor qualifies for it
    bound = np.array([V.bound_slot(a) >= 0 for a in m.assigned], bool)
    m.gone_bound = [any(bound[j] for c in m.chosen[:k] for j in c) for k in range(len(m.pres))]
    m.sees_nominated = [any(nodes[j] >= 0 and prio[j] >= prio[k] for j in range(k)) for k in range(len(m.pres))]
    return m
