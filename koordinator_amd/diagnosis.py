"""Reading koordhip_diag records (abi.DIAG_DTYPE): what the scheduler host
puts into a FitError's Diagnosis and the FailedScheduling event.

`first` counts each node under its FIRST failing Filter plugin in framework
order (upstream stops there), so it is what the reference's
Diagnosis.UnschedulablePlugins (frameworkext/eventhandlers/
reservation_handler.go:92-94) and the "0/N nodes are available" counts are
made of; `any` is koordhip_eval's no-short-circuit view.
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
}
REASON_OF_BIT = {
    abi.ST_STATIC_FAIL: "node(s) didn't match the pod's node affinity/selector, taints or were unschedulable",
    abi.ST_FIT_FAIL: "Insufficient resources",
    abi.ST_LA_FAIL: "node(s) usage exceed threshold",
    abi.ST_NUMA_FAIL: "node(s) failed NodeNUMAResource",
    abi.ST_RESV_FAIL: "node(s) failed Reservation",
}


def _slot(bit: int) -> int:
    return bit.bit_length() - 1


def unschedulable_plugins(rec) -> set:
    """The reference plugin names that rejected some node first (first > 0)."""
    return {PLUGIN_OF_BIT[b] for b in abi.FILTER_ORDER if int(rec["first"][_slot(b)]) > 0}


def summary(rec, n: int) -> str:
    """'F/N nodes are available: <count> <reason>, ...' in Filter order, the
    counts from `first` (they and `feasible` add up to N)."""
    parts = [f"{int(rec['first'][_slot(b)])} {REASON_OF_BIT[b]}" for b in abi.FILTER_ORDER
             if int(rec["first"][_slot(b)]) > 0]
    head = f"{int(rec['feasible'])}/{int(n)} nodes are available"
    return head + (": " + ", ".join(parts) + "." if parts else ".")
