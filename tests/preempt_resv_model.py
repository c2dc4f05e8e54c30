"""The preemption dry run under Reservation
(koordhip_preempt_set_mode(KOORDHIP_PREEMPT_RESV)): a plain-Python restatement
of the plugin's preemptible cycle state, independent of the device code.

    remove_pod / add_pod       the PreFilterExtensions (reservation/plugin.go:254-323)
    fits_node                  fitsNode (:445-494)
    filter_with_reservations   filterWithReservations (:373-440)

on small dict records, so that the reference's own test tables
(tests/golden/resv_preemptible_cases.json) run through them unchanged.  The
table side (slots_of, node_state) restates the BeforePreFilter restore
(transformer.go:85-175) on a NodeTable's resv_* columns.

ResvRule gives preempt_model's walk that state: every "does the preemptor fit"
is the oracle's status of the hypothetical row without its Reservation bit,
and filter_with_reservations on the state the walk has reached.
UNRESOLVABLE follows the diagnosis: on the row the walk starts from, the first
failing plugin in abi.FILTER_ORDER holds an UnschedulableAndUnresolvable reason.

add_pod(literal=True) keeps the reference's quirk: AddPod of a pod bound to a
reservation deletes the entry when the difference is zero and otherwise leaves
the OLD value in place (:278-286 never stores the difference).  literal=False
stores it; the tests use it to show that the quirk decides verdicts.

Also the generated cases the GPU tests run and four hand-worked ones
(`restricted`, `default`, `unmatched` with its three nodes, `quirk`).
"""
import functools
from unittest import mock

import numpy as np

import oracle
from koordinator_amd import abi, synth
import dataclasses

from koordinator_amd.config import PLUGIN_FIT, PLUGIN_RESERVATION, Profile, shipped_profile, to_c_config
from koordinator_amd.snapshot import NodeTable, slot_col

import preempt_cases as K
import preempt_model as M
import preempt_numa_model as N
import reasons_model as R

NRES = abi.NRES
GI = synth.GI
POLICY_NAMES = {"Default": abi.RESV_POLICY_DEFAULT, "Aligned": abi.RESV_POLICY_ALIGNED,
                "Restricted": abi.RESV_POLICY_RESTRICTED}
BRANCHES = {}          # branch name -> times taken (the coverage conditions read it)


def _took(name):
    BRANCHES[name] = BRANCHES.get(name, 0) + 1


# ------------------------------------------------------- the plugin, restated
def present(x) -> bool:
    """len(resourceList) > 0 as the engine states it: some resource is non-zero."""
    return x is not None and any(v != 0 for v in x)


class PreState:
    """preemptible[node] (pn) and preemptibleInRRs[node] (pr: slot -> amounts) of one node."""

    def __init__(self):
        self.pn = [0] * NRES
        self.pr = {}

    def any_present(self):
        return present(self.pn) or any(present(v) for v in self.pr.values())


def remove_pod(st: PreState, req, slot: int):
    """RemovePod (:292-323); slot -1: the pod is bound to no reservation."""
    if not present(req):
        return
    if slot < 0:
        st.pn = [a + b for a, b in zip(st.pn, req)]
    else:
        st.pr[slot] = [a + b for a, b in zip(st.pr.get(slot, [0] * NRES), req)]


def add_pod(st: PreState, req, slot: int, literal: bool = True):
    """AddPod (:254-290)."""
    if not present(req):
        return
    if slot < 0:
        st.pn = [max(0, a - b) for a, b in zip(st.pn, req)]
        return
    diff = [max(0, a - b) for a, b in zip(st.pr.get(slot, [0] * NRES), req)]
    if not present(diff):
        st.pr.pop(slot, None)
    elif not literal:
        st.pr[slot] = diff


def fits_node(pod, node, nrs, slot, pre) -> bool:
    """pod: req [NRES], has_req, scalar (batch-cpu, batch-memory keys); node:
    alloc [NRES], alloc_pods, npods; nrs: nmatch, pod_requested [NRES],
    r_allocated [2]; slot: the reservation (None: rRemained 0); pre: preemptible [NRES]."""
    if node["npods"] - nrs["nmatch"] + 1 > node["alloc_pods"]:
        return False
    if not pod["has_req"]:
        return True
    rem = [0, 0]
    if slot is not None:
        rem = [max(0, slot["ra"][k] - slot["rd"][k]) if slot["keys"][k] else 0 for k in range(2)]
    for k in range(NRES):
        if k >= abi.RES_BCPU and not pod["scalar"][k - abi.RES_BCPU]:
            continue
        requested = nrs["pod_requested"][k] - (rem[k] + nrs["r_allocated"][k] if k < 2 else 0) - pre[k]
        if pod["req"][k] > node["alloc"][k] - requested:
            return False
    return True


def filter_with_reservations(pod, node, nrs, matched, st: PreState):
    """None when the node passes, else the reason.  matched: [(slot index, slot record)]."""
    if not matched:
        if pod["affinity"]:
            _took("affinity")
            return "affinity"
        if st.any_present():
            ok = fits_node(pod, node, nrs, None, st.pn)
            _took("nil_fits" if ok else "nil_fails")
            return None if ok else "preemption_failed"
        _took("nil_nothing")
        return None
    pn_on = present(st.pn)
    tot, bad = [0, 0, 0], [0, 0, 0]
    for q, slot in matched:
        prq = st.pr.get(q)
        pr_on = present(prq)
        pre = [a + b for a, b in zip(prq or [0] * NRES, st.pn)]
        pol = slot["policy"]
        tot[pol] += 1
        if pol == abi.RESV_POLICY_DEFAULT:
            if pr_on or pn_on:
                ok = fits_node(pod, node, nrs, slot, pre)
                _took("default_fits" if ok else "default_insufficient")
                bad[pol] += 0 if ok else 1
            else:
                _took("default_nothing")
            continue
        fits = fits_node(pod, node, nrs, slot, pre)
        if pol == abi.RESV_POLICY_ALIGNED:
            _took("aligned_fits" if fits else "aligned_insufficient")
            if fits:
                return None
            bad[pol] += 1
            continue
        le = True
        for k in range(2):
            if not slot["keys"][k]:
                continue
            held = max(0, slot["rd"][k] - prq[k]) if pr_on else slot["rd"][k]
            left = max(0, slot["ra"][k] - held)
            if pod["keys"][k] and pod["req"][k] > left:
                le = False
        _took(("restricted_passes" if le and fits else "restricted_insufficient") + ("_returned" if pr_on else ""))
        if le and fits:
            return None
        bad[pol] += 1
    if any(tot[g] > 0 and tot[g] == bad[g] for g in range(3)):
        _took("insufficient")
        return "insufficient"
    _took("matched_passes")
    return None


# ------------------------------------------------------------ the table side
def pod_record(pod) -> dict:
    f = int(pod["flags"])
    return {"req": [int(x) for x in pod["req"]], "has_req": bool(f & abi.POD_HAS_REQ),
            "scalar": [bool(f & abi.POD_REQ_BCPU), bool(f & abi.POD_REQ_BMEM)],
            "keys": [bool(f & abi.POD_KEY_CPU), bool(f & abi.POD_KEY_MEM)], "affinity": bool(f & abi.POD_RESV_AFFINITY),
            "match": int(pod["resv_match"])}


def slots_of(table: NodeTable, i: int):
    out = []
    for q in range(max(1, table.resv_slots)):
        f = int(table[slot_col("resv_flags", q)][i])
        out.append({"flags": f, "policy": (f >> abi.RESV_POLICY_SHIFT) & 3, "group": (f >> abi.RESV_GROUP_SHIFT) & 63,
                    "keys": [bool(f & abi.RESV_KEY_CPU), bool(f & abi.RESV_KEY_MEM)],
                    "ra": [int(table[slot_col(f"resv_alloc{k}", q)][i]) for k in range(2)],
                    "rd": [int(table[slot_col(f"resv_allocated{k}", q)][i]) for k in range(2)],
                    "assigned": int(table[slot_col("resv_assigned", q)][i])})
    return out


def slot_class(slot, pod) -> int:
    """transformer.go:86-103: 1 matched, 2 unmatched with assigned pods, 0 untouched."""
    f = slot["flags"]
    if not f & abi.RESV_PRESENT:
        return 0
    if (f & abi.RESV_ALLOCATE_ONCE) and slot["assigned"] > 0:
        return 0
    if not (f & abi.RESV_UNSCHEDULABLE) and (pod["match"] >> slot["group"]) & 1:
        return 1
    return 2 if slot["assigned"] > 0 else 0


def node_state(table: NodeTable, i: int, pod):
    """(nrs, matched, d_requested [2], d_npods) of pod on node i: nodeRState as
    fits_node reads it, and what the whole restore adds to the loaded Requested
    cpu / memory and pod count."""
    slots = slots_of(table, i)
    cls = [slot_class(s, pod) for s in slots]
    requested = [int(table[f"requested{k}"][i]) for k in range(NRES)]
    matched, d = [], [0, 0]
    for q, s in enumerate(slots):
        if cls[q] == 2:      # restoreUnmatchedReservations: the reserve pod leaves, its remainder comes back
            rem = [max(0, s["ra"][k] - s["rd"][k]) if s["keys"][k] else 0 for k in range(2)]
            for k in range(2):
                d[k] += (rem[k] if any(rem) else 0) - s["ra"][k]
    touched = any(cls)
    pod_requested = [requested[k] + (d[k] if k < 2 else 0) for k in range(NRES)] if touched else [0] * NRES
    r_allocated = [0, 0]
    for q, s in enumerate(slots):
        if cls[q] == 1:
            matched.append((q, s))
            for k in range(2):
                d[k] -= s["ra"][k]
                r_allocated[k] += s["rd"][k]
    nrs = {"nmatch": len(matched), "pod_requested": pod_requested, "r_allocated": r_allocated}
    return nrs, matched, d, -len(matched)


def bound_slot(a) -> int:
    return ((int(a["flags"]) & abi.ASG_RESV_SLOT_MASK) >> abi.ASG_RESV_SLOT_SHIFT) - 1


def resv_verdicts(table: NodeTable, pod) -> np.ndarray:
    """[n] bool: the Reservation Filter fails with nothing preemptible (the oracle's ST_RESV_FAIL)."""
    p = pod_record(pod)
    out = np.zeros(table.n, bool)
    for i in range(table.n):
        nrs, matched, d, dn = node_state(table, i, p)
        node = {"alloc": [int(table[f"alloc{k}"][i]) for k in range(NRES)], "alloc_pods": int(table["alloc_pods"][i]),
                "npods": int(table["npods"][i]) + dn}
        out[i] = filter_with_reservations(p, node, nrs, matched, PreState()) is not None
    return out


def without_reservation(table: NodeTable, d_requested, d_npods) -> NodeTable:
    """The rows the walk of one preemptor starts from, on a table without reservation columns' content."""
    t = table.copy()
    for k in range(2):
        t[f"requested{k}"][:] = table[f"requested{k}"] + d_requested[:, k]
    t["npods"][:] = table["npods"] + d_npods
    for q in range(max(1, table.resv_slots)):
        t[slot_col("resv_flags", q)][:] = 0
    return t


class ResvRule(M.Rule):
    """The walk with the Reservation state of every node.  literal: add_pod's;
    base_cfg: the profile without the Reservation plugin (for the start rows'
    reasons).  Carried as functools.partial(ResvRule, literal=..., base_cfg=...)."""

    def __init__(self, cfg, table, pre, rows, literal=True, base_cfg=None):
        n = table.n
        self.rows, self.literal = rows, literal
        self.pod = pod_record(pre["pod"])
        self.info = [node_state(table, i, self.pod) for i in range(n)]
        self.alloc = [[int(table[f"alloc{k}"][i]) for k in range(NRES)] for i in range(n)]
        self.alloc_pods = [int(table["alloc_pods"][i]) for i in range(n)]
        self.state = [PreState() for _ in range(n)]
        self.resv_on = bool(int(cfg.filter_plugins) & abi.PLUGIN_RESERVATION)
        # the first failing plugin of the start row: Fit / LoadAware / NodeNUMAResource by their reasons, then Reservation
        start = without_reservation(table, np.array([x[2] for x in self.info], np.int64),
                                    np.array([x[3] for x in self.info], np.int32))
        mask = R.masks(oracle.Oracle(base_cfg if base_cfg is not None else cfg, start),
                       np.ascontiguousarray(pre["pod"].reshape(1)))[0]
        self.first = abi.first_reasons(mask)

    def resv_reason(self, i):
        if not self.resv_on:
            return None
        nrs, matched, _, dn = self.info[i]
        node = {"alloc": self.alloc[i], "alloc_pods": self.alloc_pods[i], "npods": int(self.rows.cols["npods"][i]) + dn}
        return filter_with_reservations(self.pod, node, nrs, matched, self.state[i])

    def unresolvable(self, i):
        if self.first[i]:
            return bool(self.first[i] & abi.REASON_UNRESOLVABLE_MASK)
        return self.resv_reason(i) == "affinity"

    def fits(self, status, i):
        """The oracle's status without its Reservation bit, and filter_with_reservations on the state the walk has reached."""
        return (status & ~abi.ST_RESV_FAIL) == 0 and self.resv_reason(i) is None

    def moved(self, i, a, sign):
        req = [int(x) for x in a["pod"]["req"]]
        if sign < 0:
            remove_pod(self.state[i], req, bound_slot(a))
        else:
            add_pod(self.state[i], req, bound_slot(a), self.literal)


def dry_run(cfg, table, assigned, pdb_allowed, pres, literal=True, base_cfg=None):
    return M.dry_run(cfg, table, assigned, pdb_allowed, pres, functools.partial(ResvRule, literal=literal, base_cfg=base_cfg))


# ---------------------------------------------------------------- generators
# name -> (n, n_pre, seed, slots, a node of 128 listed pods, NodeNUMAResource)
CASES = {
    "lane": (1, 1, M.SEED + 136, 1, False, False),
    "wave": (130, 5, M.SEED + 32, 1, False, False),
    "tiles": (257, 33, M.SEED + 34, 4, True, False),
    "numa": (130, 6, M.SEED + 36, 1, False, True),
    "numa4": (130, 4, M.SEED + 38, 4, False, True),
}
GROUPS = 4
BOUND_FRAC = 0.5


def resv_profile(numa=False):
    return shipped_profile(numa=numa, reservation=True)


def resv_spec(slots):
    return synth.ResvSpec(node_frac=0.7, groups=GROUPS, allocate_once_frac=0.3, aligned_frac=0.3, restricted_frac=0.3,
                          unschedulable_frac=0.05, cpu_only_frac=0.2, assigned_frac=0.5, slots=slots,
                          multi_frac=0.7 if slots > 1 else 0.0)


def inputs(n, n_pre, seed, slots, full, numa, base_per: int = 0) -> M.Inputs:
    """preempt_model.inputs (preempt_numa_model.inputs with `numa`) on a cluster
    with reservations: the reserve pods and their assigned pods' share are part
    of the rows before they are tightened; every other preemptor matches an
    owner group, every fourth carries a required reservation affinity, and
    about half of the listed pods of a node with reservations are bound to one."""
    make_cluster = synth.make_cluster

    def cluster(cs, p):
        return synth.add_reservations(make_cluster(cs, p), resv_spec(slots), seed)

    with mock.patch.object(synth, "make_cluster", cluster):
        inp = N.inputs(n, n_pre, seed, synth.NumaSpec(amp_frac=0.3), False, base_per) if numa else \
            M.inputs("base", n, n_pre, seed, full, base_per)
    table, a, pres = inp.table, inp.assigned, inp.pres
    m = len(a)
    # the bindings: one of the node's present slots
    on = np.stack([(table[slot_col("resv_flags", q)] & abi.RESV_PRESENT) != 0 for q in range(slots)], axis=1)
    first = np.argsort(~on, axis=1, kind="stable")            # a node's present slots, ascending, then the rest
    cnt = on.sum(axis=1)[a["node"]]
    pick = (synth.splitmix64(seed, m, 950) % np.maximum(cnt, 1).astype(np.uint64)).astype(np.int64)
    bind = (synth.uniform(seed, m, 951) < BOUND_FRAC) & (cnt > 0)
    slot = first[a["node"], pick]
    a["flags"] = a["flags"] | np.where(bind, (slot + 1) << abi.ASG_RESV_SLOT_SHIFT, 0).astype(a["flags"].dtype)
    # the preemptors: owner groups and affinities; a matched preemptor is an LS pod with both keys
    pod = pres["pod"]
    g = (synth.splitmix64(seed, n_pre, 952) % np.uint64(GROUPS)).astype(np.uint64)
    k = np.arange(n_pre)
    pod["resv_match"] = np.where(k % 2 == 0, np.uint64(1) << g, np.uint64(0))
    pod["flags"] |= np.where(k % 4 == 2, abi.POD_RESV_AFFINITY, 0).astype(pod["flags"].dtype)
    pod["flags"] |= np.where(k % 8 == 7, abi.POD_RESV_AFFINITY, 0).astype(pod["flags"].dtype)   # ... matching nothing
    pres["pod"] = pod
    return M.Inputs(resv_profile(numa), table, a, inp.pdb_allowed, pres)


# ------------------------------------------------------------ directed cases
def _slot(t: NodeTable, i, q, policy, ra, rd, assigned, group=0, once=False):
    """Reservation slot q of node i holding cpu only; its reserve pod (and nothing else) joins the row."""
    f = abi.RESV_PRESENT | abi.RESV_KEY_CPU | (policy << abi.RESV_POLICY_SHIFT) | (group << abi.RESV_GROUP_SHIFT)
    f |= abi.RESV_ALLOCATE_ONCE if once else 0
    t[slot_col("resv_flags", q)][i] = f
    t[slot_col("resv_alloc0", q)][i] = t[slot_col("resv_nz0", q)][i] = ra
    t[slot_col("resv_allocated0", q)][i] = rd
    t[slot_col("resv_assigned", q)][i] = assigned
    t["requested0"][i] += ra
    t["nz_cpu_m"][i] += ra
    t["npods"][i] += 1


def _bound(a, q):
    a["flags"] |= abi.asg_resv_slot(q)
    return a


def _pre(cpu, match=True, prio=1000):
    p = K.preemptor(cpu, prio=prio)
    p["pod"]["flags"] |= abi.POD_KEY_CPU
    p["pod"]["resv_match"] = 1 if match else 0
    return p


def _directed_profile():
    return Profile(filters=(PLUGIN_FIT, PLUGIN_RESERVATION), scores={PLUGIN_FIT: 1, PLUGIN_RESERVATION: 5000})


def without_plugin(prof):
    """The profile without the Reservation plugin."""
    return dataclasses.replace(prof, filters=tuple(f for f in prof.filters if f != PLUGIN_RESERVATION),
                               scores={k: v for k, v in prof.scores.items() if k != PLUGIN_RESERVATION})


def _table(a, extra=None):
    t = K.table(1, a, extra)
    t.set_resv_slots(1)
    return t


def _one(t, a, pres) -> M.Inputs:
    return M.Inputs(_directed_profile(), t, a, (), np.array(pres, abi.PREEMPTOR_DTYPE))


def _restricted() -> M.Inputs:
    """A Restricted slot that passes only because its bound pod is removed.
    Node of 10 CPUs.  A Restricted reservation of 4 CPUs (reusable), all 4
    allocated to its one assigned pod: pod 0, listed, bound, priority 10.  Pod 1
    (2 CPUs, priority 20) is not bound.  Requested = 4 (reserve pod) + 4 + 2 =
    10000.  The preemptor asks 4 CPUs and matches the reservation.

    Start row: 10000 - 4000 = 6000, podRequested 10000, rAllocated 4000,
    rRemained 0.  Fit: 4000 <= 10000 - 6000 passes.  Reservation: fitsNode 4000 >
    10000 - (10000 - 0 - 4000 - 0) = 4000 is false: fits; Restricted: 4000 >
    4000 - 4000 = 0: insufficient.  The node fails by Reservation alone.
    Both removed (list order: pod 1, pod 0): row 0, Pn = 2000, Pr[0] = 4000.
    fitsNode: 4000 > 10000 - (10000 - 4000 - 6000) = 10000: fits; Restricted:
    a = max(0, 4000 - 4000) = 0, 4000 <= 4000: passes.
    Pod 1 back: Pn = 0, row 2000: fitsNode 4000 > 10000 - (10000 - 4000 - 4000)
    = 8000: fits, Restricted as before: reprieved.
    Pod 0 back: Pr[0] - 4000 = 0: deleted.  Row 6000: Fit passes, fitsNode
    fits, Restricted: a = 4000, 4000 > 0: insufficient: pod 0 is the victim."""
    a = K.records([_bound(K.A(0, 4000, 10, start=1), 0), K.A(0, 2000, 20, start=2)])
    t = _table(a)
    _slot(t, 0, 0, abi.RESV_POLICY_RESTRICTED, 4000, 4000, 1)
    return _one(t, a, [_pre(4000)])


RESTRICTED_VICTIMS = [0]


def _default() -> M.Inputs:
    """A Default slot that is insufficient only once something is preemptible.
    Node of 10 CPUs with two Default reservations of 3 CPUs each, nothing
    allocated; pod 0 (1 CPU, priority 10, not bound) and 5 CPUs of pods that are
    not listed.  Requested = 3 + 3 + 1 + 5 = 12000.  The preemptor asks 3 CPUs
    and matches both.

    Start row: 12000 - 6000 = 6000, podRequested 12000.  Fit: 3000 <= 4000
    passes; nothing is preemptible, so no Default slot is tested: the node
    passes the whole Filter as it stands.
    Pod 0 removed: row 5000 (Fit passes), Pn = 1000.  Per slot fitsNode gives
    back that slot's remainder only: 3000 > 10000 - (12000 - 3000 - 0 - 1000) =
    2000: both slots insufficient, 2 of 2 Default: the node fails: UNFIT."""
    a = K.records([K.A(0, 1000, 10, start=1)])
    t = K.table(1, a, extra=[5000])
    t.set_resv_slots(2)
    _slot(t, 0, 0, abi.RESV_POLICY_DEFAULT, 3000, 0, 0)
    _slot(t, 0, 1, abi.RESV_POLICY_DEFAULT, 3000, 0, 0)
    return _one(t, a, [_pre(3000)])


def _unmatched() -> M.Inputs:
    """The branch without a matched reservation, on three nodes of 10 CPUs; the
    preemptor asks 3 CPUs and matches nothing.  Each node lists one pod of 4
    CPUs (priority 10) beside 4 CPUs of pods that are not listed.

    Node 0: a reservation of 4 CPUs, 4 allocated to its assigned pod, the
    listed pod, bound.  Requested = 4 + 4 + 4 = 12000; the unmatched restore
    takes the reserve pod out (remainder 0): start row and podRequested 8000.
    Fit: 3000 > 2000 fails.  Removed: row 4000, Fit passes; Pr[0] = 4000, Pn = 0.
    fitsNode(nil, Pn): 3000 > 10000 - (8000 - 0) = 2000: ErrReasonPreemptionFailed:
    UNFIT -- what a bound pod returns goes to its reservation, not to the node.
    Node 1: the same, the listed pod not bound: Pn = 4000: 3000 > 10000 - (8000
    - 4000) = 6000 is false: fits.  Back: Fit fails: the pod is the victim.
    Node 2: no reservation, Requested 8000, no nodeRState (podRequested 0):
    removed, Pn = 4000: 3000 > 10000 - (0 - 4000): fits.  Back: victim."""
    a = K.records([_bound(K.A(0, 4000, 10, start=1), 0), K.A(1, 4000, 10, start=1), K.A(2, 4000, 10, start=1)])
    t = K.table(3, a, extra=[4000, 4000, 4000])
    t.set_resv_slots(1)
    for i in (0, 1):
        _slot(t, i, 0, abi.RESV_POLICY_DEFAULT, 4000, 4000, 1, group=1)
    return _one(t, a, [_pre(3000, match=False)])


UNMATCHED_STATUS = [abi.PREEMPT_UNFIT, abi.PREEMPT_CANDIDATE, abi.PREEMPT_CANDIDATE]
UNMATCHED_VICTIMS = [[], [1], [2]]


def _quirk() -> M.Inputs:
    """The literal AddPod changes a victim list.  Node of 10 CPUs, a Restricted
    reservation of 4 CPUs (reusable), all allocated to its two assigned pods,
    both listed and bound: pod 0 (2 CPUs, priority 20), pod 1 (2 CPUs, priority
    10).  Requested = 4 + 2 + 2 = 8000.  The preemptor asks 2 CPUs and matches.

    Start row 4000, podRequested 8000, rAllocated 4000.  Restricted: 2000 > 4000
    - 4000: insufficient.  Both removed: Pr[0] = 4000: a = 0, passes.
    Pod 0 back: Pr[0] - 2000 = 2000 is not zero, so the reference leaves Pr[0]
    = 4000 (a fixed AddPod would store 2000; 2000 <= 4000 - 2000 passes too):
    reprieved.  Pod 1 back: Pr[0] - 2000 = 2000 again, Pr[0] stays 4000: a = 0,
    passes: reprieved, NO victim although the reservation is full again.  The
    fixed AddPod reaches Pr[0] = 0, a = 4000, insufficient: pod 1 is its victim."""
    a = K.records([_bound(K.A(0, 2000, 20, start=1), 0), _bound(K.A(0, 2000, 10, start=2), 0)])
    t = _table(a)
    _slot(t, 0, 0, abi.RESV_POLICY_RESTRICTED, 4000, 4000, 2)
    return _one(t, a, [_pre(2000)])


QUIRK_FIXED_VICTIMS = [1]

_DIRECTED = {"restricted": _restricted, "default": _default, "unmatched": _unmatched, "quirk": _quirk}
DIRECTED = tuple(_DIRECTED)
ALL_CASES = list(CASES) + list(DIRECTED)


class Model:
    pass


@functools.lru_cache(maxsize=None)
def case(name: str, literal: bool = True) -> Model:
    """The case's inputs and the expected answers of koordhip_preempt /
    koordhip_preempt_node_verdicts in the Reservation mode.  Computed once;
    callers must not modify it."""
    inp = _DIRECTED[name]() if name in _DIRECTED else inputs(*CASES[name])
    m = Model()
    m.name, m.prof, m.table, m.assigned, m.pdb_allowed, m.pres = name, inp.prof, inp.table, inp.assigned, inp.pdb_allowed, inp.pres
    m.cfg = to_c_config(inp.prof)
    m.base_cfg = to_c_config(without_plugin(inp.prof))
    m.res, m.verdicts, m.chosen, m.victims, m.potential = dry_run(m.cfg, m.table, m.assigned, m.pdb_allowed, m.pres,
                                                                  literal, m.base_cfg)
    return m
