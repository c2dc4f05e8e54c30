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
