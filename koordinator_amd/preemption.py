"""Host side of the preemption dry run (koordhip_preempt*): the table of the
pods that sit on the nodes, the preemptor records and a view of the result.

    assigned_records   k8s pods on nodes -> abi.ASSIGNED_DTYPE (priority, start
                       time, non-preemptible label, quota name -> id, pdb_mask
                       from the PDB objects as preempt.go:222-267 matches them)
    preemptor_records  pending pods + their quotas' postFilterState -> abi.PREEMPTOR_DTYPE
    PreemptionResult   node name + victim pod keys of one preemptor
    assigned_ext_records / preemptor_ext_records
                       the dry run under DeviceShare (preempt_set_mode(device=True)):
                       what the listed pods hold of devices and extended scalars
                       (abi.ASSIGNED_EXT_DTYPE, beside assigned_records' records) and
                       the preemptors' koordhip_pod_ext records

With Reservation state (PlacementEngine.preempt_set_mode(resv=True)) pass
assigned_records the per-node slot order of the snapshot's reservation columns
(`reservation_slots`): a listed pod names the slot of the reservation it was
assumed into, and reserve pods are not listed.  In that mode the batch in
sequence is PlacementEngine.preempt_stream(pres, resv=True)
(koordhip_preempt_stream_resv): the earlier preemptors' victims have also left
their reservations (Allocated and the assigned count, by the slot a record
names), so the same records serve and nothing is to be pre-subtracted.

PodEligibleToPreemptOthers and nominated pods stay with the caller.

For a batch answered by PlacementEngine.preempt_stream (koordhip_preempt_stream)
the records are the same, and every QuotaState.used is the quota's used AS OF
THE START OF THE CALL: the engine itself lowers it for a later preemptor of the
same quota by what the earlier preemptors' victims held (floored at 0), and it
does not add the nominated preemptors to it.  Do not pre-subtract victims of
preemptors of the same batch, and do not reuse the records of one call for the
next without refreshing used, the table and the PDBs' DisruptionsAllowed.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import numpy as np

from . import abi, k8s
from .config import Profile
from .marshal import MarshalError, pod_record
from .reservation import Reservation, is_reserve_pod, reservation_allocated
from .topologyspread import LabelSelector

LABEL_QUOTA_NAME = "quota.scheduling.koordinator.sh/name"           # apis/extension/elastic_quota.go:37
LABEL_PREEMPTIBLE = "quota.scheduling.koordinator.sh/preemptible"   # :42
DEFAULT_QUOTA_NAME = "koordinator-default-quota"
QUOTA_RESOURCES = (k8s.CPU, k8s.MEMORY)                             # the default quota dimensions (<= PREEMPT_QRES)


@dataclass
class PodDisruptionBudget:
    """policy/v1 PodDisruptionBudget as filterPodsWithPDBViolation reads it."""
    namespace: str = "default"
    name: str = "pdb"
    selector: Optional[LabelSelector] = None     # None: LabelSelectorAsSelector(nil) matches nothing
    disruptions_allowed: int = 0                 # Status.DisruptionsAllowed
    disrupted_pods: Sequence[str] = ()           # Status.DisruptedPods keys (pod names)


@dataclass
class QuotaState:
    """postFilterState of a pending pod's quota (plugin.go PreFilter): used and
    runtime as resource lists; `skip` when the plugin's PreFilter skipped."""
    used: k8s.ResourceList = field(default_factory=dict)
    runtime: k8s.ResourceList = field(default_factory=dict)
    skip: bool = False


def is_non_preemptible(pod: k8s.Pod) -> bool:
    """extension.IsPodNonPreemptible (elastic_quota.go:79-81)."""
    return (pod.labels or {}).get(LABEL_PREEMPTIBLE) == "false"


def quota_name(pod: k8s.Pod) -> str:
    """The pod's quota label, else the default quota (the namespace fallback of
    getPodAssociateQuotaName needs the ElasticQuota lister: pass your own `quota_of`)."""
    return (pod.labels or {}).get(LABEL_QUOTA_NAME) or DEFAULT_QUOTA_NAME


def pdb_matches(pdb: PodDisruptionBudget, pod: k8s.Pod) -> bool:
    """preempt.go:231-250: same namespace, a non-empty selector that matches, the
    pod not among the PDB's DisruptedPods; a pod without labels matches no PDB."""
    if not pod.labels or pdb.namespace != pod.namespace or pdb.selector is None:
        return False
    sel = pdb.selector
    if not sel.match_labels and not sel.match_expressions:
        return False
    return sel.matches(pod.labels) and pod.name not in pdb.disrupted_pods


def _quantities(rlist: k8s.ResourceList, resources) -> List[int]:
    out = [0] * abi.PREEMPT_QRES
    for d, name in enumerate(resources):
        if name in rlist:
            out[d] = k8s.resource_value(name, rlist[name])
    return out


class QuotaIds:
    """quota name -> the id the records carry (host-assigned, dense from 0)."""

    def __init__(self):
        self.ids: Dict[str, int] = {}

    def of(self, name: str) -> int:
        return self.ids.setdefault(name, len(self.ids))


def assigned_records(pods: Iterable[k8s.Pod], profile: Profile, node_index: Dict[str, int], quotas: QuotaIds,
                     pdbs: Sequence[PodDisruptionBudget] = (), now_ns: int = 0,
                     start_time_ns: Optional[Dict[str, int]] = None, in_quota: Optional[Callable[[k8s.Pod], bool]] = None,
                     quota_of: Callable[[k8s.Pod], str] = quota_name, resources=QUOTA_RESOURCES, static_classes=None,
                     reservation_slots: Optional[Dict[int, List[Reservation]]] = None):
    """(abi.ASSIGNED_DTYPE records, DisruptionsAllowed per PDB, pod keys) of the
    pods bound to the snapshot's nodes (pod.node_name in `node_index`).
    `start_time_ns`: status.startTime by pod key (absent: `now_ns`, as
    GetPodStartTime).  `in_quota(pod)`: quotaInfo.IsPodExist (default: every pod).
    `reservation_slots`: node row -> its reservations in slot order, as
    reservation.available_by_node returned them for reservation_columns (the
    KOORDHIP_PREEMPT_RESV mode).  With it a pod's reservation-allocated
    annotation becomes abi.asg_resv_slot(slot) in its flags (matched by UID;
    MarshalError when its node holds no such reservation)
    and reserve pods are skipped: the plugin's AddPod / RemovePod skip them and
    the dry run never lists them as victims."""
    if len(pdbs) > abi.PREEMPT_PDBS:
        raise MarshalError(f"{len(pdbs)} PodDisruptionBudgets: the table takes {abi.PREEMPT_PDBS}")
    if len(resources) > abi.PREEMPT_QRES:
        raise MarshalError(f"{len(resources)} quota dimensions: the records take {abi.PREEMPT_QRES}")
    pods = [p for p in pods if p.node_name in node_index]
    if reservation_slots is not None:
        pods = [p for p in pods if not is_reserve_pod(p)]
    out = np.zeros(len(pods), abi.ASSIGNED_DTYPE)
    for j, pod in enumerate(pods):
        rec = out[j]
        pod_record(pod, profile, rec["pod"], static_classes=static_classes)
        rec["node"] = node_index[pod.node_name]
        rec["priority"] = pod.priority or 0
        rec["start_time"] = (start_time_ns or {}).get(pod.key, now_ns)
        rec["quota"] = quotas.of(quota_of(pod))
        rec["flags"] = ((abi.ASG_NONPREEMPTIBLE if is_non_preemptible(pod) else 0) |
                        (abi.ASG_IN_QUOTA if in_quota is None or in_quota(pod) else 0))
        rec["pdb_mask"] = sum(1 << i for i, pdb in enumerate(pdbs) if pdb_matches(pdb, pod))
        reqs, _ = k8s.pod_requests_and_limits(pod)
        rec["qreq"] = _quantities(reqs, resources)
        bound = reservation_allocated(pod) if reservation_slots is not None else None
        if bound is not None and bound[0]:             # (an empty UID counts as not bound, plugin.go:270,309)
            slots = reservation_slots.get(int(rec["node"]), [])
            q = next((k for k, r in enumerate(slots) if r.uid == bound[0]), None)
            if q is None:
                raise MarshalError(f"pod {pod.key}: bound to reservation {bound[1]!r} (uid {bound[0]}), which has no "
                                   f"slot on node {pod.node_name}")
            rec["flags"] = int(rec["flags"]) | abi.asg_resv_slot(q)
    return out, np.array([p.disruptions_allowed for p in pdbs], np.int32), [p.key for p in pods]


def preemptor_records(pods: Iterable[k8s.Pod], profile: Profile, quotas: QuotaIds, states: Dict[str, QuotaState],
                      quota_of: Callable[[k8s.Pod], str] = quota_name, resources=QUOTA_RESOURCES,
                      static_classes=None) -> np.ndarray:
    """abi.PREEMPTOR_DTYPE records; states: quota name -> its postFilterState
    (absent or skip: quota -1, no quota check and no victims)."""
    pods = list(pods)
    out = np.zeros(len(pods), abi.PREEMPTOR_DTYPE)
    for j, pod in enumerate(pods):
        rec = out[j]
        pod_record(pod, profile, rec["pod"], static_classes=static_classes)
        rec["priority"] = pod.priority or 0
        name = quota_of(pod)
        st = states.get(name)
        if st is None or st.skip:
            rec["quota"] = -1
            continue
        rec["quota"] = quotas.of(name)
        rec["q_used"] = _quantities(st.used, resources)
        rec["q_runtime"] = _quantities(st.runtime, resources)
        reqs, _ = k8s.pod_requests_and_limits(pod)
        rec["q_req"] = _quantities(reqs, resources)
        rec["q_mask"] = sum(1 << d for d, r in enumerate(resources) if r in st.runtime)
    return out


def assigned_ext_records(pods: Iterable[k8s.Pod], table, node_index: Dict[str, int],
                         reservation_slots: Optional[Dict[int, List[Reservation]]] = None) -> np.ndarray:
    """abi.ASSIGNED_EXT_DTYPE records beside assigned_records' (the same pods in
    the same order: those bound to a node of `node_index`), for the dry run
    under DeviceShare (PlacementEngine.preempt_set_mode(device=True)).
    `reservation_slots`: what assigned_records was given (only whether it is
    None is read): with it reserve pods are skipped here as well, so that the
    two tables stay parallel.  Under DeviceShare beside Reservation state
    (preempt_set_mode(numa_frozen=..., resv=True, device=True, device_resv=True)):

        slots = reservation.available_by_node(...)        # as for reservation_columns
        a, pdb, keys = assigned_records(pods, prof, node_index, quotas, pdbs, reservation_slots=slots)
        ax = assigned_ext_records(pods, table, node_index, reservation_slots=slots)
        engine.preempt_load_pods(a, pdb, ext=ax)

    A record's fields:

      xreq / xmask          deviceshare.fit_xreq: the extended scalars
                            NodeInfo.RemovePod / AddPod move
      dev_slots / dev_per   the device-allocated annotation
                            (deviceshare.parse_device_allocated), every minor as
                            the slot of the pod's node in `table`'s dev_minor

    A minor the node does not list is dropped (the reference frees nothing
    there either: total[minor] is nil).  MarshalError for a pod whose minors of
    one type hold different amounts: the records carry one per-card amount per
    type (plugin.go:465-478 allocates that way)."""
    from . import deviceshare as ds
    pods = [p for p in pods if p.node_name in node_index]
    if reservation_slots is not None:
        pods = [p for p in pods if not is_reserve_pod(p)]
    out = np.zeros(len(pods), abi.ASSIGNED_EXT_DTYPE)
    for j, pod in enumerate(pods):
        rec = out[j]
        for name, v in ds.fit_xreq(pod).items():
            k = ds.XRES_INDEX[name]
            rec["xreq"][k] = v
            rec["xmask"] |= 1 << k
        i = node_index[pod.node_name]
        for typ, items in ds.parse_device_allocated(pod.annotations).items():
            if typ not in ds.TYPE_INDEX:
                raise MarshalError(f"pod {pod.key}: device type {typ!r} is not supported (gpu, rdma, fpga)")
            t = ds.TYPE_INDEX[typ]
            per = None
            for minor, res in items:
                slots = [s for s in range(table.dev_slots) if int(table["dev_minor"][i, t, s]) == minor]
                if not slots:
                    continue
                amounts = [int(res.get(n, 0)) for n in ds.TYPE_RESOURCES[typ]]
                if per is not None and amounts != per:
                    raise MarshalError(f"pod {pod.key}: its {typ} minors hold different amounts ({per} and {amounts}); "
                                       "the dry run under DeviceShare takes one per-card amount per type")
                per = amounts
                rec["dev_slots"][t] |= 1 << slots[0]
            if per is not None:
                rec["dev_per"][t, :len(per)] = per
    return out


def preemptor_ext_records(pods: Iterable[k8s.Pod]) -> np.ndarray:
    """The preemptors' abi.POD_EXT_DTYPE records (deviceshare.pod_ext_records) for preempt(ext=...)."""
    from . import deviceshare as ds
    return ds.pod_ext_records(pods)


@dataclass
class PreemptionResult:
    """One preemptor's koordhip_preempt_result with names: the nominated node
    (None: no candidate), the victims' pod keys in the reference's order, the
    nodes per status."""
    node: Optional[str]
    victims: List[str]
    n_victims: int
    n_pdb_violations: int
    counts: Dict[str, int]

    STATUS_NAMES = ("candidate", "no_victims", "unfit", "error", "unresolvable")

    @classmethod
    def of(cls, result, victims, node_names: Sequence[str], pod_keys: Sequence[str]) -> "PreemptionResult":
        node = int(result["node"])
        return cls(node=node_names[node] if node >= 0 else None,
                   victims=[pod_keys[int(v)] for v in victims if v >= 0],
                   n_victims=int(result["best"]["n_victims"]),
                   n_pdb_violations=int(result["best"]["n_pdb_violations"]),
                   counts={s: int(result["count"][k]) for k, s in enumerate(cls.STATUS_NAMES)})
