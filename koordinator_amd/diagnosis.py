"""Reading koordhip_diag records (abi.DIAG_DTYPE): what the scheduler host
puts into a FitError's Diagnosis and the FailedScheduling event.

`first` counts each node under its FIRST failing Filter plugin in framework
order (upstream stops there), so it is what the reference's
Diagnosis.UnschedulablePlugins (frameworkext/eventhandlers/
reservation_handler.go:92-94) and the "0/N nodes are available" counts are
made of; `any` is koordhip_eval's no-short-circuit view.

Records of koordhip_diagnose_ext also fill the sequential cycle's slots
(DeviceShare, the extended scalars, PodTopologySpread, InterPodAffinity) and
count `first` in abi.FILTER_ORDER_EXT, which restricted to the five older bits
is abi.FILTER_ORDER: the functions below walk the extended order, and a record
without those slots reads as before.
"""
from __future__ import annotations

from . import abi

# The host resolves NodeUnschedulable / NodeAffinity / TaintToleration into one
# static filter bit (KOORDHIP_PLUGIN_NODE_STATIC), so the trio is one entry.
STATIC_PLUGINS = "NodeUnschedulable/NodeAffinity/TaintToleration"
PLUGIN_OF_BIT = {
    abi.ST_STATIC_FAIL: STATIC_PLUGINS,
    abi.ST_FIT_FAIL: "NodeResourcesFit",
    abi.ST_LA_FAIL: "LoadAwareScheduling",
    abi.ST_NUMA_FAIL: "NodeNUMAResource",
    abi.ST_RESV_FAIL: "Reservation",
    abi.ST_DEVICE_FAIL: "DeviceShare",
    abi.ST_XFIT_FAIL: "NodeResourcesFit",         # the extended scalars: the same plugin as ST_FIT_FAIL
    abi.ST_PTS_FAIL: "PodTopologySpread",
    abi.ST_IPA_FAIL: "InterPodAffinity",
}
REASON_OF_BIT = {
    abi.ST_STATIC_FAIL: "node(s) didn't match the pod's node affinity/selector, taints or were unschedulable",
    abi.ST_FIT_FAIL: "Insufficient resources",
    abi.ST_LA_FAIL: "node(s) usage exceed threshold",
    abi.ST_NUMA_FAIL: "node(s) failed NodeNUMAResource",
    abi.ST_RESV_FAIL: "node(s) failed Reservation",
    abi.ST_DEVICE_FAIL: "Insufficient Devices",   # deviceshare/plugin.go:52 ErrInsufficientDevices
    abi.ST_XFIT_FAIL: "Insufficient extended resources",
    # (upstream, k8s v1.24, not vendored in the reference: unpinned) podtopologyspread ErrReasonConstraintsNotMatch /
    # ErrReasonNodeLabelNotMatch and interpodaffinity ErrReasonAffinityRulesNotMatch and its two
    # anti-affinity siblings, one status bit each here
    abi.ST_PTS_FAIL: "node(s) didn't match pod topology spread constraints",
    abi.ST_IPA_FAIL: "node(s) didn't match pod affinity/anti-affinity rules",
}


# koordhip_reasons records (abi.REASONS_DTYPE): the reference's Status reason per slot.  The NodeResourcesFit
# strings are upstream's (k8s v1.24 fit.go InsufficientResource.Reason, not vendored: unpinned); the rest are the
# koordinator plugins' own (nodenumaresource/plugin.go:50-55, resource_manager.go:258,450, topology_hint.go:36,
# reservation/plugin.go:50,58).  Slots that collapse several reference strings say so in DESIGN.md 4.9.2.
REASON_TEXT = {
    abi.REASON_STATIC: REASON_OF_BIT[abi.ST_STATIC_FAIL],
    abi.REASON_FIT_PODS: "Too many pods",
    abi.REASON_FIT_CPU: "Insufficient cpu",
    abi.REASON_FIT_MEM: "Insufficient memory",
    abi.REASON_FIT_EPH: "Insufficient ephemeral-storage",
    abi.REASON_FIT_BCPU: "Insufficient kubernetes.io/batch-cpu",
    abi.REASON_FIT_BMEM: "Insufficient kubernetes.io/batch-memory",
    abi.REASON_LA_USAGE: REASON_OF_BIT[abi.ST_LA_FAIL],       # load_aware.go:45-46 without the resource name
    abi.REASON_NUMA_POD_ERROR: "the requested CPUs must be integer",
    abi.REASON_NUMA_AMP_CPU: "Insufficient amplified cpu",
    abi.REASON_NUMA_NO_TOPOLOGY: "node(s) CPU Topology not found",
    abi.REASON_NUMA_SMT_ALIGN: "node(s) requested cpus not multiple cpus per core",
    abi.REASON_NUMA_FULL_PCPUS_ONLY: "node(s) required FullPCPUs policy",
    abi.REASON_NUMA_CPUS: "not enough cpus available to satisfy request",
    abi.REASON_NUMA_REQUIRED_POLICY: "insufficient CPUs to satisfy required cpu bind policy",
    abi.REASON_NUMA_NO_ZONES: "node(s) missing NUMA resources",
    abi.REASON_NUMA_POLICY: "node(s) NUMA Topology affinity error",
    abi.REASON_RESV_AFFINITY: "node(s) no reservations match reservation affinity",
    abi.REASON_RESV_INSUFFICIENT: "node(s) reservations insufficient resources",
}
assert sorted(REASON_TEXT) == list(range(abi.REASON_COUNT))
# ... and slots 27-31 of koordhip_diagnose_reasons_ext's records (slots 19-26 are "Insufficient " + the extended
# scalar's name, deviceshare.XRES): deviceshare/plugin.go:52, and upstream's (k8s v1.24, not vendored: unpinned)
# podtopologyspread / interpodaffinity strings.  Two slots collapse two reference strings:
# DEVICE_INSUFFICIENT also stands for "node(s) reservations insufficient devices" (deviceshare/reservation.go:280),
# IPA_ANTI for "node(s) didn't satisfy existing pods anti-affinity rules".
REASON_TEXT_EXT = {
    abi.REASON_DEVICE_INSUFFICIENT: REASON_OF_BIT[abi.ST_DEVICE_FAIL],
    abi.REASON_PTS_MISSING_LABEL: "node(s) didn't match pod topology spread constraints (missing required label)",
    abi.REASON_PTS_SKEW: REASON_OF_BIT[abi.ST_PTS_FAIL],
    abi.REASON_IPA_AFFINITY: "node(s) didn't match pod affinity rules",
    abi.REASON_IPA_ANTI: "node(s) didn't match pod anti-affinity rules",
}
assert sorted(REASON_TEXT_EXT) == list(range(abi.REASON_FIT_X0 + abi.NXRES, abi.REASON_EXT_COUNT))


def reason_text(r: int) -> str:
    """The Status reason string of slot r (0 .. abi.REASON_EXT_COUNT - 1)."""
    if r < abi.REASON_COUNT:
        return REASON_TEXT[r]
    if r < abi.REASON_FIT_X0 + abi.NXRES:
        from .deviceshare import XRES
        return "Insufficient " + XRES[r - abi.REASON_FIT_X0]
    return REASON_TEXT_EXT[r]


def fit_error_message(rec, n: int) -> str:
    """Upstream FitError.Error() (k8s v1.24 framework/types.go, not vendored:
    unpinned) over a koordhip_reasons record: '0/N nodes are available: ' + the
    '<count> <reason>' strings of `first`, sorted as strings, joined with ', ',
    then '.'.  A node that fails NodeResourcesFit on several resources counts
    under each, as upstream's per-reason histogram does.  Slots 19-31 (records
    of koordhip_diagnose_reasons_ext) print alike; a record with zeros there
    reads as before."""
    parts = sorted(f"{int(rec['first'][r])} {reason_text(r)}" for r in range(abi.REASON_EXT_COUNT)
                   if int(rec["first"][r]) > 0)
    return f"0/{int(n)} nodes are available: " + ", ".join(parts) + "."


def preemption_might_help(rec, n: int) -> bool:
    """Whether nodesWherePreemptionMightHelp leaves PostFilter any node: some
    failing node's status is not UnschedulableAndUnresolvable."""
    return int(n) - int(rec["feasible"]) - int(rec["unresolvable"]) > 0


def _slot(bit: int) -> int:
    return bit.bit_length() - 1


def unschedulable_plugins(rec) -> set:
    """The reference plugin names that rejected some node first (first > 0)."""
    return {PLUGIN_OF_BIT[b] for b in abi.FILTER_ORDER_EXT if int(rec["first"][_slot(b)]) > 0}


def summary(rec, n: int) -> str:
    """'F/N nodes are available: <count> <reason>, ...' in Filter order, the
    counts from `first` (they and `feasible` add up to N)."""
    parts = [f"{int(rec['first'][_slot(b)])} {REASON_OF_BIT[b]}" for b in abi.FILTER_ORDER_EXT
             if int(rec["first"][_slot(b)]) > 0]
    head = f"{int(rec['feasible'])}/{int(n)} nodes are available"
    return head + (": " + ", ".join(parts) + "." if parts else ".")
