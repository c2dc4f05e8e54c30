"""The preemption dry run under DeviceShare beside Reservation state
(koordhip_preempt_set_mode with KOORDHIP_PREEMPT_DEVICE | KOORDHIP_PREEMPT_RESV |
KOORDHIP_PREEMPT_DEVICE_RESV): a plain-Python restatement of both plugins'
preemptible cycle state on one node, independent of the device code, built from
preempt_resv_model (the restore, fitsNode over the five row resources, the
slots) and preempt_dev_model (the device maps, the allocator's free amounts).

What exists only where both states do:

    Reservation's maps    preemptible[node] and preemptibleInRRs[node][uid] are
                          whole ResourceLists (reservation/plugin.go:254-323):
                          literal dicts resource name -> amount here, the listed
                          pods' extended scalars included; fitsNode (:445-494)
                          also loops over the preemptor's ScalarResources
    DeviceShare's maps    preemptibleDevices[node] and preemptibleInRRs[node][uid]
                          (deviceshare/plugin.go:188-282): a victim bound to a
                          reservation goes to the second, which Filter (:284-323)
                          never hands to the node allocation and
                          tryAllocateFromReservation leaves alone without a
                          device-holding reservation (reservation.go:192)
    the Filter order      DeviceShare precedes Reservation (abi.FILTER_ORDER_EXT)

Beside the literal maps DevResvRule keeps the linear form the kernel keeps (Pn /
Pr[q] as vectors over the five resources and every KOORDHIP_NXRES scalar, Pd as
the plain sum of the removed pods that are NOT bound) and asserts after every
move and in every fit test that both agree.

Also the generated cases the GPU tests run (each on one and on four reservation
slots) and eight hand-worked ones.
"""
import functools
from unittest import mock

import numpy as np

import oracle
from koordinator_amd import abi, synth
from koordinator_amd.config import (PLUGIN_DEVICESHARE, PLUGIN_FIT, PLUGIN_RESERVATION, Profile, shipped_profile,
                                    to_c_config, with_deviceshare)
from koordinator_amd.deviceshare import GPU_CORE, NVIDIA_GPU, XRES, XRES_INDEX
from koordinator_amd.snapshot import slot_col

import preempt_cases as K
import preempt_dev_model as D
import preempt_model as M
import preempt_numa_model as N
import preempt_resv_model as V
import reasons_model as R

NRES, NX, DT, DR = abi.NRES, abi.NXRES, abi.DEV_TYPES, abi.DEV_RES
G = abi.DEV_GPU
NAMES = ["cpu", "memory", "ephemeral-storage", "kubernetes.io/batch-cpu", "kubernetes.io/batch-memory"] + \
    [XRES[j] if j < len(XRES) else f"scalar-{j}" for j in range(NX)]
BRANCHES = {}          # branch name -> times taken (the coverage condition reads it)
COVERAGE = ("bound_device", "scalar_term_decides", "affinity_device_fails", "no_rstate")


def _took(name):
    BRANCHES[name] = BRANCHES.get(name, 0) + 1


# ------------------------------------------------------- the plugin, restated
def requests_of(a, ax) -> dict:
    """PodRequestsAndLimits of a listed pod: the names it requests something of."""
    out = {NAMES[k]: int(a["pod"]["req"][k]) for k in range(NRES) if int(a["pod"]["req"][k])}
    if ax is not None:
        for j in range(NX):
            if (int(ax["xmask"]) >> j) & 1 and int(ax["xreq"][j]):
                out[NAMES[NRES + j]] = int(ax["xreq"][j])
    return out


def is_zero(rl) -> bool:
    """quotav1.IsZero."""
    return not rl or not any(rl.values())


def add(a, b) -> dict:
    """quotav1.Add."""
    out = dict(a or {})
    for k, v in b.items():
        out[k] = out.get(k, 0) + v
    return out


def subtract_non_negative(a, b) -> dict:
    """quotav1.SubtractWithNonNegativeResult."""
    out = {k: max(0, v - b.get(k, 0)) for k, v in (a or {}).items()}
    for k in b:
        out.setdefault(k, 0)
    return out


class Literal:
    """Both plugins' cycle state of one node, as the reference holds it."""

    def __init__(self):
        self.pn = {}           # Reservation: preemptible[node]
        self.pr = {}           # Reservation: preemptibleInRRs[node], slot -> ResourceList
        self.devices = {}      # DeviceShare: preemptibleDevices[node], type -> minor -> amounts
        self.dev_in_rrs = {}   # DeviceShare: preemptibleInRRs[node], slot -> type -> minor -> amounts


def resv_remove_pod(st: Literal, reqs: dict, slot: int):
    """reservation RemovePod (:292-323)."""
    if is_zero(reqs):
        return
    if slot < 0:
        st.pn = add(st.pn, reqs)
    else:
        st.pr[slot] = add(st.pr.get(slot), reqs)


def resv_add_pod(st: Literal, reqs: dict, slot: int):
    """reservation AddPod (:254-290): the bound branch never stores the difference."""
    if is_zero(reqs):
        return
    if slot < 0:
        left = subtract_non_negative(st.pn, reqs)
        st.pn = {} if is_zero(left) else left
        return
    left = subtract_non_negative(st.pr.get(slot), reqs)
    if is_zero(left):
        st.pr.pop(slot, None)


def dev_remove_pod(st: Literal, allocated: dict, slot: int):
    """deviceshare RemovePod (:238-282)."""
    if not allocated:
        return
    if slot < 0:
        D.append_allocated(st.devices, allocated)
    else:
        _took("bound_device")
        st.dev_in_rrs[slot] = D.append_allocated(st.dev_in_rrs.get(slot, {}), allocated)


def dev_add_pod(st: Literal, allocated: dict, slot: int):
    """deviceshare AddPod (:188-236)."""
    if not allocated:
        return
    if slot < 0:
        D.subtract_allocated(st.devices, allocated)
        return
    left = D.subtract_allocated(st.dev_in_rrs.get(slot, {}), allocated)
    if not left:
        st.dev_in_rrs.pop(slot, None)


def vector(rl) -> list:
    return [int((rl or {}).get(n, 0)) for n in NAMES]


def fits_node(pod, x, node, nrs, slot, pre, scalars=True) -> bool:
    """fitsNode: preempt_resv_model's over the five row resources, then the loop over the preemptor's
    ScalarResources.  node["xhead"][j] = Allocatable[j] - podRequested[j]; rRemained and allRAllocated hold no
    scalar (the reservations here hold cpu / memory); pre: amounts [NRES + NX]."""
    if not V.fits_node(pod, node, nrs, slot, pre[:NRES]):
        return False
    if not pod["has_req"] or not scalars:
        return True
    for j in range(NX):
        if (int(x["xmask"]) >> j) & 1 and int(x["xreq"][j]) > node["xhead"][j] + pre[NRES + j]:
            return False
    return True


def filter_with_reservations(pod, x, node, nrs, matched, pn, pr_of, scalars=True):
    """filterWithReservations (:373-440).  pn: amounts [NRES + NX]; pr_of(q): slot q's amounts or None.  None
    when the node passes, else the reason."""
    if not matched:
        if pod["affinity"]:
            return "affinity"
        if V.present(pn) or any(V.present(pr_of(q)) for q in range(node["slots"])):
            return None if fits_node(pod, x, node, nrs, None, pn, scalars) else "preemption_failed"
        return None
    pn_on = V.present(pn)
    tot, bad = [0, 0, 0], [0, 0, 0]
    for q, slot in matched:
        prq = pr_of(q)
        pr_on = V.present(prq)
        pre = [a + b for a, b in zip(prq or [0] * len(pn), pn)]
        pol = slot["policy"]
        tot[pol] += 1
        if pol == abi.RESV_POLICY_DEFAULT:
            if (pr_on or pn_on) and not fits_node(pod, x, node, nrs, slot, pre, scalars):
                bad[pol] += 1
            continue
        fits = fits_node(pod, x, node, nrs, slot, pre, scalars)
        if pol == abi.RESV_POLICY_ALIGNED:
            if fits:
                return None
            bad[pol] += 1
            continue
        le = True
        for k in range(2):         # Mask(allocated, ResourceNames): the reservation's own names, cpu / memory
            if not slot["keys"][k]:
                continue
            held = max(0, slot["rd"][k] - prq[k]) if pr_on else slot["rd"][k]
            if pod["keys"][k] and pod["req"][k] > max(0, slot["ra"][k] - held):
                le = False
        if le and fits:
            return None
        bad[pol] += 1
    if any(tot[g] > 0 and tot[g] == bad[g] for g in range(3)):
        return "insufficient"
    return None


class DevResvRule(M.Rule):
    """The walk with both plugins' state of every node.  Carried as
    functools.partial(DevResvRule, x=..., ax=..., assigned=..., base_cfg=...): x the preemptor's POD_EXT_DTYPE
    record, ax the listed pods' ASSIGNED_EXT_DTYPE records (None: none), base_cfg the profile without DeviceShare
    and without the Reservation plugin (the start rows' reasons)."""

    def __init__(self, cfg, table, pre, rows, x=None, ax=None, assigned=None, base_cfg=None):
        n = table.n
        self.rows = rows
        self.x = x if x is not None else abi.pod_ext_array(1)[0]
        self.device = bool(int(self.x["flags"]) & abi.PODX_DEVICE)
        self.ax, self.assigned = ax, assigned
        self.pod = V.pod_record(pre["pod"])
        self.resv_cols = slot_col("resv_flags", 0) in table.cols
        self.slots = max(1, table.resv_slots) if self.resv_cols else 1
        none = ({"nmatch": 0, "pod_requested": [0] * NRES, "r_allocated": [0, 0]}, [], [0, 0], 0)
        self.info = [V.node_state(table, i, self.pod) if self.resv_cols else none for i in range(n)]
        self.touched = [self.resv_cols and any(V.slot_class(s, self.pod) for s in V.slots_of(table, i)) for i in range(n)]
        self.alloc = [[int(table[f"alloc{k}"][i]) for k in range(NRES)] for i in range(n)]
        self.alloc_pods = [int(table["alloc_pods"][i]) for i in range(n)]
        ext = table.has_ext
        self.xalloc = table["xalloc"] if ext else np.zeros((n, NX), np.int64)
        self.xr = table["xrequested"].copy() if ext else np.zeros((n, NX), np.int64)
        # podRequested's scalars: the loaded ones (the restore of cpu / memory reservations moves none), 0 without a nodeRState
        self.xhead = [[int(self.xalloc[i, j]) - (int(self.xr[i, j]) if self.touched[i] else 0) for j in range(NX)]
                      for i in range(n)]
        self.nodes = [D.node_devices(table, i) if ext else None for i in range(n)]
        self.lit = [Literal() for _ in range(n)]
        # the linear form: Pn, Pr[q] over the five resources and every scalar; Pd of the pods that are not bound
        self.pn = np.zeros((n, NRES + NX), np.int64)
        self.pr = np.zeros((n, self.slots, NRES + NX), np.int64)
        self.pd = np.zeros((n, DT, max(1, table.dev_slots), DR), np.int64)
        self.resv_on = bool(int(cfg.filter_plugins) & abi.PLUGIN_RESERVATION)
        self.calls = [0] * n
        # the first failing plugin of the start row before DeviceShare and Reservation
        if self.resv_cols:
            start = V.without_reservation(table, np.array([v[2] for v in self.info], np.int64),
                                          np.array([v[3] for v in self.info], np.int32))
        else:
            start = table
        mask = R.masks(oracle.Oracle(base_cfg if base_cfg is not None else cfg, start),
                       np.ascontiguousarray(pre["pod"].reshape(1)))[0]
        self.first = abi.first_reasons(mask)

    def _ax_of(self, a):
        if self.ax is None:
            return None
        j = (a.__array_interface__["data"][0] - self.assigned.__array_interface__["data"][0]) // self.assigned.itemsize
        return self.ax[j]

    def _node(self, i):
        return {"alloc": self.alloc[i], "alloc_pods": self.alloc_pods[i],
                "npods": int(self.rows.cols["npods"][i]) + self.info[i][3], "xhead": self.xhead[i], "slots": self.slots}

    def _agree(self, i):
        """The literal maps are the linear form."""
        st = self.lit[i]
        assert vector(st.pn) == [int(v) for v in self.pn[i]], (i, st.pn, self.pn[i])
        for q in range(self.slots):
            assert vector(st.pr.get(q)) == [int(v) for v in self.pr[i, q]], (i, q, st.pr.get(q), self.pr[i, q])
        assert not any(q >= self.slots for q in st.pr)
        for t in range(DT):
            for s in range(self.pd.shape[2]):
                lit = st.devices.get(t, {}).get(s, [0] * DR)
                assert lit == [int(v) for v in self.pd[i, t, s]], (i, t, s, lit, self.pd[i, t, s])

    def resv_reason(self, i, scalars=True):
        if not self.resv_on:
            return None
        nrs, matched = self.info[i][0], self.info[i][1]
        st = self.lit[i]
        lit = filter_with_reservations(self.pod, self.x, self._node(i), nrs, matched, vector(st.pn),
                                       lambda q: vector(st.pr[q]) if q in st.pr else None, scalars)
        lin = filter_with_reservations(self.pod, self.x, self._node(i), nrs, matched, [int(v) for v in self.pn[i]],
                                       lambda q: [int(v) for v in self.pr[i, q]], scalars)
        assert lit == lin, f"node {i}: the literal maps say {lit}, the linear form {lin}"
        return lit

    def dev_ok(self, i) -> bool:
        if not self.device:
            return True
        lit = D.device_filter(self.x["dev_req"], self.nodes[i], self.lit[i].devices)
        lin = D.linear_filter(self.x["dev_req"], self.nodes[i], self.pd[i])
        assert lit == lin, f"node {i}: the literal device maps say {lit}, the linear form {lin}"
        return lit

    def unresolvable(self, i):
        """The first failing plugin of the start row in abi.FILTER_ORDER_EXT holds an UnschedulableAndUnresolvable
        reason: NodeResourcesFit with its scalars, LoadAware, NodeNUMAResource, DeviceShare, then Reservation."""
        f = int(self.first[i])
        fit = abi.REASONS_OF_BIT[abi.ST_STATIC_FAIL] | abi.REASONS_OF_BIT[abi.ST_FIT_FAIL]
        if f & fit:
            return bool(f & abi.REASON_UNRESOLVABLE_MASK)
        if not D.xfit(self.x, self.xalloc[i], self.xr[i]):
            return False
        if f:
            return bool(f & abi.REASON_UNRESOLVABLE_MASK)
        affinity = self.resv_reason(i) == "affinity"
        if not self.dev_ok(i):
            if affinity:
                _took("affinity_device_fails")
            return False
        return affinity

    def fits(self, status, i):
        self._agree(i)
        self.calls[i] += 1
        if (status & ~abi.ST_RESV_FAIL) != 0:
            return False
        if not D.xfit(self.x, self.xalloc[i], self.xr[i]) or not self.dev_ok(i):
            return False
        reason = self.resv_reason(i)
        if reason is not None and self.resv_reason(i, scalars=False) is None:
            _took("scalar_term_decides")
        if not self.touched[i] and (V.present(self.pn[i]) or self.pr[i].any()):
            _took("no_rstate")
        return reason is None

    def moved(self, i, a, sign):
        ax = self._ax_of(a)
        slot = V.bound_slot(a) if self.resv_cols else -1
        # NodeInfo.RemovePod / AddPod: Requested.ScalarResources, bound or not
        if ax is not None:
            for j in range(NX):
                if (int(ax["xmask"]) >> j) & 1:
                    self.xr[i, j] += sign * int(ax["xreq"][j])
        # the Reservation plugin
        reqs = requests_of(a, ax)
        st = self.lit[i]
        (resv_remove_pod if sign < 0 else resv_add_pod)(st, reqs, slot)
        v = np.array(vector(reqs), np.int64)
        if v.any():
            if slot < 0:
                self.pn[i] = self.pn[i] + v if sign < 0 else np.maximum(self.pn[i] - v, 0)
            elif sign < 0:
                self.pr[i, slot] += v
            elif not (self.pr[i, slot] > v).any():
                self.pr[i, slot] = 0
        # DeviceShare (state.skip for a preemptor without a device request; no nodeDevice entry: nothing)
        alloc = D.allocation_of(ax) if ax is not None else {}
        if self.device and self.nodes[i] is not None and alloc:
            (dev_remove_pod if sign < 0 else dev_add_pod)(st, alloc, slot)
            if slot < 0:
                for t, devs in alloc.items():
                    for s, res in devs.items():
                        self.pd[i, t, s] -= sign * np.array(res, np.int64)
        self._agree(i)


def dry_run(cfg, table, assigned, pdb_allowed, pres, ext=None, ax=None, base_cfg=None):
    """preempt_model.dry_run with every preemptor's own rule.  cfg: the profile WITHOUT DeviceShare (the rows'
    oracle, whose Reservation bit the rule replaces); base_cfg: without the Reservation plugin as well."""
    lists = M.node_lists(assigned, table.n)
    res = np.zeros(len(pres), abi.PREEMPT_RESULT_DTYPE)
    ver = np.zeros((len(pres), table.n), abi.PREEMPT_NODE_DTYPE)
    chosen, allv, allp = [], [], []
    for p in range(len(pres)):
        rule = functools.partial(DevResvRule, x=None if ext is None else ext[p], ax=ax, assigned=assigned,
                                 base_cfg=base_cfg)
        v, vic, pot = M.select_victims(cfg, table, assigned, pdb_allowed, pres[p], lists, rule)
        ver[p] = v
        res[p] = M.pick(v)
        chosen.append(vic[int(res[p]["node"])] if res[p]["node"] >= 0 else [])
        allv.append(vic)
        allp.append(pot)
    return res, ver, chosen, allv, allp


# ---------------------------------------------------------------- generators
# name -> (n, n_pre, seed, a node of 128 listed pods and eight GPUs, NodeNUMAResource); each on 1 and on 4 slots
SHAPES = {
    "lane": (1, 1, M.SEED + 150, False, False),
    "wave": (70, 5, M.SEED + 73, False, False),
    "tiles": (257, 33, M.SEED + 54, True, False),
    "numa": (70, 5, M.SEED + 64, False, True),
}
SLOTS = (1, abi.RESV_SLOTS)
CASES = {f"{name}{s}": shape + (s,) for name, shape in SHAPES.items() for s in SLOTS}


def devresv_profile(numa=False):
    return with_deviceshare(shipped_profile(numa=numa, reservation=True))


def inputs(n, n_pre, seed, full, numa, slots, base_per: int = 0, dev_every: int = 0, dev_spec=None,
           dev_pod_frac: float = D.DEV_POD_FRAC):
    """preempt_dev_model.inputs on a cluster with preempt_resv_model's reservations (the reserve pods and their
    assigned pods' share are part of the rows before they are tightened): about half of the listed pods of a
    node with reservations are bound to one of its slots, about half of a GPU node's listed pods hold a GPU share
    (so about half of the bound ones do); the preemptors carry preempt_resv_model's owner groups and
    affinities; base_per, dev_every, dev_spec, dev_pod_frac: preempt_dev_model.inputs' (the timing runs).  Returns
    (Inputs, ext, ax)."""
    make_cluster = synth.make_cluster

    def cluster(cs, p):
        return synth.add_reservations(make_cluster(cs, p), V.resv_spec(slots), seed)

    with mock.patch.object(synth, "make_cluster", cluster):
        inp, ext, ax = D.inputs(n, n_pre, seed, full, numa, base_per, dev_pod_frac=dev_pod_frac, dev_every=dev_every,
                                dev_spec=dev_spec)
    table, a, pres = inp.table, inp.assigned, inp.pres
    m = len(a)
    on = np.stack([(table[slot_col("resv_flags", q)] & abi.RESV_PRESENT) != 0 for q in range(slots)], axis=1)
    first = np.argsort(~on, axis=1, kind="stable")
    cnt = on.sum(axis=1)[a["node"]]
    pick = (synth.splitmix64(seed, m, 950) % np.maximum(cnt, 1).astype(np.uint64)).astype(np.int64)
    bind = (synth.uniform(seed, m, 951) < V.BOUND_FRAC) & (cnt > 0)
    slot = first[a["node"], pick]
    a["flags"] = a["flags"] | np.where(bind, (slot + 1) << abi.ASG_RESV_SLOT_SHIFT, 0).astype(a["flags"].dtype)
    pod = pres["pod"]
    g = (synth.splitmix64(seed, n_pre, 952) % np.uint64(V.GROUPS)).astype(np.uint64)
    k = np.arange(n_pre)
    pod["resv_match"] = np.where(k % 2 == 0, np.uint64(1) << g, np.uint64(0))
    pod["flags"] |= np.where(k % 4 == 2, abi.POD_RESV_AFFINITY, 0).astype(pod["flags"].dtype)
    pod["flags"] |= np.where(k % 8 == 7, abi.POD_RESV_AFFINITY, 0).astype(pod["flags"].dtype)
    pres["pod"] = pod
    return M.Inputs(devresv_profile(numa), table, a, inp.pdb_allowed, pres), ext, ax


# ------------------------------------------------------------ directed cases
CAND, NOV, UNFIT, UNRES = abi.PREEMPT_CANDIDATE, abi.PREEMPT_NO_VICTIMS, abi.PREEMPT_UNFIT, abi.PREEMPT_UNRESOLVABLE
KN, KC = XRES_INDEX[NVIDIA_GPU], XRES_INDEX[GPU_CORE]


def _profile():
    return Profile(filters=(PLUGIN_FIT, PLUGIN_DEVICESHARE, PLUGIN_RESERVATION),
                   scores={PLUGIN_FIT: 1, PLUGIN_DEVICESHARE: 1, PLUGIN_RESERVATION: 5000})


def _table(n, a, extra=None):
    t = D._table(n, a, extra)
    t.set_resv_slots(1)
    return t


def _one(t, a, ax, pres, x, prof=None):
    return M.Inputs(prof or _profile(), t, a, (), np.array(pres, abi.PREEMPTOR_DTYPE)), x, ax


def _scalar_ext(j, amount):
    """A preemptor without a device request that asks `amount` of extended scalar j."""
    x = abi.pod_ext_array(1)
    x["xreq"][0, j], x["xmask"] = amount, 1 << j
    return x


def _holds(ax, t, k, i, j, amount, requested=True):
    """Listed pod k of node i requests `amount` of extended scalar j."""
    ax["xreq"][k, j] = amount
    ax["xmask"][k] |= 1 << j
    if requested:
        t["xrequested"][i, j] += amount


def _bound_device():
    """Two nodes of 10 CPUs with one GPU each, held whole by the node's listed pod (1 CPU, priority 10), and a
    Default reservation of 1 CPU of owner group 1, its 1 CPU allocated to its one assigned pod.  P asks 1 CPU
    and a whole GPU and matches nothing (group 0).

    Node 0: the listed pod 0 is the reservation's, bound.  Requested = 1000 (reserve pod) + 1000 = 2000; the
    unmatched restore takes the reserve pod out, remainder 0: start row and podRequested 1000.  Fit passes,
    DeviceShare fails (the GPU is used).  Pod 0 removed: row 0, Pr[0] = {cpu: 1000}; its GPU goes to DeviceShare's
    preemptibleInRRs, preemptibleDevices stays empty: DeviceShare still fails: UNFIT.
    Node 1: the reservation's pod is not listed (1000 of extra Requested), pod 1 is not bound.  Requested 3000,
    start row and podRequested 2000.  Pod 1 removed: Pn = {cpu: 1000}, Pd = the GPU: DeviceShare passes,
    fitsNode(nil, Pn): 1000 > 10000 - (2000 - 1000) is false: fits.  Back: Pd empty: fails: the victim."""
    a, ax = D._pods(V._bound(K.A(0, 1000, 10, start=1), 0), K.A(1, 1000, 10, start=1))
    t = _table(2, a, extra=[0, 1000])
    for i in (0, 1):
        D._gpus(t, i, 1)
        D._hold(t, ax, i, i, G, 0, 100)
        V._slot(t, i, 0, abi.RESV_POLICY_DEFAULT, 1000, 1000, 1, group=1)
    return _one(t, a, ax, [V._pre(1000, match=False)], D._ext(100, 100))


def _bound_scalar(once=False, group=1):
    """One node of 10 CPUs, nvidia.com/gpu Allocatable 1, Requested 1: held by the listed pod 0 (1 CPU,
    priority 10), which is bound to a Default reservation of 1 CPU of owner group 1 (all allocated, one assigned
    pod).  P asks 1 CPU and nvidia.com/gpu 1, no device, and matches nothing.

    Requested = 2000, the unmatched restore takes the reserve pod out: start row and podRequested 1000,
    podRequested's nvidia.com/gpu 1.  NodeResourcesFit: 1 > 1 - 1 fails.  Pod 0 removed: the moved Requested
    holds 0: NodeResourcesFit passes.  Pr[0] = {cpu: 1000, nvidia.com/gpu: 1}, Pn empty; no matched reservation
    and something preemptible: fitsNode(nil, Pn): 1 > 1 - (1 - 0) = 0: ErrReasonPreemptionFailed: UNFIT -- what
    a bound pod returns goes to its reservation, scalars included."""
    a, ax = D._pods(V._bound(K.A(0, 1000, 10, start=1), 0))
    t = _table(1, a)
    V._slot(t, 0, 0, abi.RESV_POLICY_DEFAULT, 1000, 1000, 1, group=group, once=once)
    t["xalloc"][0, KN] = 1
    _holds(ax, t, 0, 0, KN, 1)
    return _one(t, a, ax, [V._pre(1000, match=group == 0)], _scalar_ext(KN, 1))


def _matched_scalar():
    """_bound_scalar with the reservation matched (owner group 0).  Requested 2000, podRequested 2000 (the
    clone before the matched restore), start row 1000, rAllocated 1000, rRemained 0.  Pod 0 removed: Pr[0] =
    {cpu: 1000, nvidia.com/gpu: 1}: the Default slot is tested with preemptible = Pr[0] + Pn: cpu 1000 > 10000 -
    (2000 - 0 - 1000 - 1000) is false, nvidia.com/gpu 1 > 1 - (1 - 1) = 1 is false: fits: CANDIDATE.  Back:
    Pr[0] - requests is zero everywhere: deleted; the moved Requested holds 1 again: NodeResourcesFit fails:
    pod 0 is the victim."""
    return _bound_scalar(group=0)


def _no_rstate():
    """_bound_scalar with an AllocateOnce reservation: it has an assigned pod, so it is neither matched nor
    restored (class 0) and the node has no nodeRState: podRequested counts as 0, in every resource.  The reserve
    pod stays on the row: start row 2000.  Pod 0 removed: Pr[0] = {cpu: 1000, nvidia.com/gpu: 1};
    fitsNode(nil, Pn): cpu 1000 > 10000 - (0 - 0), nvidia.com/gpu 1 > 1 - (0 - 0) = 1, both false: fits, where
    _bound_scalar's frozen podRequested failed: CANDIDATE.  Back: NodeResourcesFit fails: the victim."""
    return _bound_scalar(once=True)


def _quirk_scalar():
    """The literal AddPod with a scalar the preemptor does not request.  Node of 10 CPUs, a Restricted
    reservation of 2 CPUs (matched), all allocated, two assigned pods, both listed and bound: pod 0 (2 CPUs,
    priority 20) and pod 1 (no CPU, gpu-core 50, priority 10).  P asks 2 CPUs, no scalar, no device.

    Requested = 2000 + 2000 = 4000, start row 2000, podRequested 4000, rAllocated 2000.  Restricted: 2000 > 2000
    - 2000: insufficient.  Both removed: Pr[0] = {cpu: 2000, gpu-core: 50}: a = max0(2000 - 2000) = 0: passes.
    Pod 0 back: Pr[0] - requests = {cpu: 0, gpu-core: 50} is not zero, so Pr[0] KEEPS {cpu: 2000, gpu-core: 50}:
    a = 0, passes: reprieved.  Pod 1 back: the difference is {cpu: 2000, gpu-core: 0}: kept again: reprieved: no
    victim.  A state over cpu .. batch-memory alone would not move pod 1 at all and delete Pr[0] at pod 0: a =
    2000, insufficient, pod 0 the victim."""
    a, ax = D._pods(V._bound(K.A(0, 2000, 20, start=1), 0), V._bound(K.A(0, 0, 10, start=2), 0))
    t = _table(1, a)
    V._slot(t, 0, 0, abi.RESV_POLICY_RESTRICTED, 2000, 2000, 2)
    t["xalloc"][0, KC] = 100
    _holds(ax, t, 1, 0, KC, 50)
    return _one(t, a, ax, [V._pre(2000)], abi.pod_ext_array(1))


def _affinity_device():
    """A required reservation affinity that matches nothing, on three nodes of 10 CPUs with one GPU each and no
    reservation.  P asks 1 CPU and a whole GPU.  Node 0: the GPU is free, pod 0 (1 CPU) holds none: every plugin
    before Reservation passes on the start row, Reservation fails with ErrReasonReservationAffinity:
    UNRESOLVABLE.  Node 1: the GPU is held by the listed pod 1: DeviceShare, which precedes Reservation, is the
    first failing plugin and Unschedulable; no removal cures the affinity: UNFIT.  Node 2: the GPU is held by
    a pod that is not listed and nothing is listed: NO_VICTIMS."""
    a, ax = D._pods(K.A(0, 1000, 10, start=1), K.A(1, 1000, 10, start=1))
    t = _table(3, a)
    for i in range(3):
        D._gpus(t, i, 1)
    D._hold(t, ax, 1, 1, G, 0, 100)
    D._hold(t, ax, None, 2, G, 0, 100)
    pre = V._pre(1000, match=False)
    pre["pod"]["flags"] |= abi.POD_RESV_AFFINITY
    return _one(t, a, ax, [pre], D._ext(100, 100))


def _reprieve():
    """Two GPUs: pod 0 (priority 20, not bound) holds GPU 0, pod 1 (priority 10) holds GPU 1 and is bound to a
    Default reservation of owner group 1 (1 CPU, all allocated, one assigned pod).  P asks 1 CPU and a whole GPU
    and matches nothing.  Requested 3000, start row and podRequested 2000.  Both removed: Pd = {GPU 0} (GPU 1
    went to preemptibleInRRs), Pn = {cpu: 1000}, Pr[0] = {cpu: 1000}: DeviceShare passes, fitsNode(nil, Pn)
    fits.  Pod 0 back first (list order): Pd empty: DeviceShare fails: pod 0 is a victim although it is the more
    important pod.  Pod 1 back: Pd = {GPU 0} still: passes: reprieved.  Under DeviceShare alone pod 0 would be
    reprieved (GPU 1 free) and pod 1 the victim."""
    a, ax = D._pods(K.A(0, 1000, 20, start=1), V._bound(K.A(0, 1000, 10, start=2), 0))
    t = _table(1, a)
    D._gpus(t, 0, 2)
    D._hold(t, ax, 0, 0, G, 0, 100)
    D._hold(t, ax, 1, 0, G, 1, 100)
    V._slot(t, 0, 0, abi.RESV_POLICY_DEFAULT, 1000, 1000, 1, group=1)
    return _one(t, a, ax, [V._pre(1000, match=False)], D._ext(100, 100))


def _numa():
    """preempt_numa_model's `frozen` node beside both states: 16 CPUs, all held by four listed cpuset pods of 4
    CPUs (priorities 10 .. 40); pod 3 holds the node's one GPU and is bound to a Default reservation of owner
    group 1.  Preemptor 0, a cpuset pod with the required policy FullPCPUs, fails the frozen plane whatever is
    removed: UNFIT.  Preemptor 1, the same pod without a cpuset, asks no device: three pods fit back, pod 0
    (priority 10) is the victim."""
    inp = N._frozen()
    t, a = inp.table, inp.assigned
    ax = np.zeros(len(a), abi.ASSIGNED_EXT_DTYPE)
    t.enable_ext(dev_slots=4)
    t.set_resv_slots(1)
    D._gpus(t, 0, 1)
    D._hold(t, ax, 3, 0, G, 0, 100)
    a["flags"][3] |= abi.asg_resv_slot(0)
    f = abi.RESV_PRESENT | abi.RESV_KEY_CPU | (1 << abi.RESV_GROUP_SHIFT)
    t[slot_col("resv_flags", 0)][0] = f          # (its reserve pod's 0 CPUs are part of the row)
    t[slot_col("resv_assigned", 0)][0] = 1
    pres = inp.pres.copy()
    for p in pres:
        p["pod"]["flags"] |= abi.POD_KEY_CPU
    return M.Inputs(devresv_profile(numa=True), t, a, (), pres), abi.pod_ext_array(2), ax


_DIRECTED = {"bound_device": _bound_device, "bound_scalar": _bound_scalar, "matched_scalar": _matched_scalar,
             "no_rstate": _no_rstate, "quirk_scalar": _quirk_scalar, "affinity_device": _affinity_device,
             "reprieve": _reprieve, "numa": _numa}
DIRECTED = tuple(_DIRECTED)
ALL_CASES = list(CASES) + list(DIRECTED)
# by hand: per preemptor, per node (status, victims in append order)
EXPECTED = {
    "bound_device": [[(UNFIT, []), (CAND, [1])]],
    "bound_scalar": [[(UNFIT, [])]],
    "matched_scalar": [[(CAND, [0])]],
    "no_rstate": [[(CAND, [0])]],
    "quirk_scalar": [[(CAND, [])]],
    "affinity_device": [[(UNRES, []), (UNFIT, []), (NOV, [])]],
    "reprieve": [[(CAND, [0])]],
    "numa": [[(UNFIT, [])], [(CAND, [0])]],
}


def without(prof, *plugins):
    import dataclasses
    return dataclasses.replace(prof, filters=tuple(f for f in prof.filters if f not in plugins),
                               scores={k: v for k, v in prof.scores.items() if k not in plugins})


class Model:
    pass


@functools.lru_cache(maxsize=None)
def case(name: str) -> Model:
    """The case's inputs and the expected answers of koordhip_preempt_ext /
    koordhip_preempt_node_verdicts_ext in the DEVICE_RESV mode.  Computed once;
    callers must not modify it."""
    inp, ext, ax = _DIRECTED[name]() if name in _DIRECTED else inputs(*CASES[name])
    m = Model()
    m.name, m.prof, m.table, m.assigned, m.pdb_allowed, m.pres = name, inp.prof, inp.table, inp.assigned, inp.pdb_allowed, inp.pres
    m.ext, m.ax = ext, ax
    m.cfg = to_c_config(inp.prof)
    m.numa = bool(int(m.cfg.filter_plugins) & abi.PLUGIN_NUMA)
    m.resv_cfg = to_c_config(without(inp.prof, PLUGIN_DEVICESHARE))
    m.base_cfg = to_c_config(without(inp.prof, PLUGIN_DEVICESHARE, PLUGIN_RESERVATION))
    before = dict(BRANCHES)
    m.res, m.verdicts, m.chosen, m.victims, m.potential = dry_run(m.resv_cfg, m.table, m.assigned, m.pdb_allowed, m.pres,
                                                                  ext, ax, m.base_cfg)
    m.branches = {k: v - before.get(k, 0) for k, v in BRANCHES.items() if v - before.get(k, 0)}
    return m
