"""Writes filter_reasons.json: the Status each Filter case of the reference's
table tests wants, transcribed as data (code and reason string).  The cases
themselves are the ones numa_plugin_cases.json and reservation_cases.json
already hold under the same names; this file adds what their boolean `want`
leaves out.

  plugins/nodenumaresource/plugin_test.go:544-812   TestPlugin_Filter
  plugins/nodenumaresource/plugin_test.go:814-925   TestFilterWithAmplifiedCPUs
  plugins/reservation/plugin_test.go:527-1202       Test_filterWithReservations (the four
                                                    rows of reservation_cases.json)
  plugins/reservation/plugin_test.go:261-269        TestPreFilter "failed to reservation affinity"

code: "Success", "Unschedulable", "UnschedulableAndUnresolvable" or "Error";
reason: the Status' one reason (the plugins' Err* constants spelled out), ""
for Success.
"""
import json
import os

U, UU = "Unschedulable", "UnschedulableAndUnresolvable"
# nodenumaresource/plugin.go:50-55, reservation/plugin.go:50,58
NOT_FOUND_TOPOLOGY = "node(s) CPU Topology not found"
INVALID_TOPOLOGY = "node(s) invalid CPU Topology"
SMT_ALIGNMENT = "node(s) requested cpus not multiple cpus per core"
REQUIRED_FULL_PCPUS = "node(s) required FullPCPUs policy"
INSUFFICIENT_AMPLIFIED_CPU = "Insufficient amplified cpu"
RESV_AFFINITY = "node(s) no reservations match reservation affinity"
RESV_INSUFFICIENT = "node(s) reservations insufficient resources"


def row(name, source, code="Success", reason=""):
    return {"name": name, "source": source, "code": code, "reason": reason}


F = "plugin_test.go:"
NUMA_FILTER = [
    row("error with missing CPUTopology", F + "560-565", UU, NOT_FOUND_TOPOLOGY),
    row("error with invalid cpu topology", F + "566-574", UU, INVALID_TOPOLOGY),
    row("succeed with valid cpu topology", F + "575-583"),
    row("succeed with skip", F + "584-590"),
    row("verify FullPCPUsOnly with SMTAlignmentError", F + "591-604", UU, SMT_ALIGNMENT),
    row("verify required FullPCPUs SMTAlignmentError", F + "605-616", UU, SMT_ALIGNMENT),
    row("verify FullPCPUsOnly with preferred SpreadByPCPUs", F + "617-630", UU, REQUIRED_FULL_PCPUS),
    row("verify FullPCPUsOnly with required SpreadByPCPUs", F + "631-645", UU, REQUIRED_FULL_PCPUS),
    row("verify Kubelet FullPCPUsOnly with SMTAlignmentError", F + "646-662", UU, SMT_ALIGNMENT),
    row("verify Kubelet FullPCPUsOnly with RequiredFullPCPUsPolicy", F + "663-679", UU, REQUIRED_FULL_PCPUS),
    row("verify required FullPCPUs with none NUMA topology policy", F + "680-690"),
    row("verify FullPCPUs with NUMA Topology Policy", F + "691-704"),
]

NUMA_FILTER_AMP = [
    row("no resources requested always fits", F + "825-830"),
    row("no filtering without node cpu amplification", F + "831-837"),
    row("cpu fits on no NRT node", F + "838-844"),
    row("insufficient cpu", F + "845-852", U, INSUFFICIENT_AMPLIFIED_CPU),
    row("insufficient cpu with cpuset pod on node", F + "853-861", U, INSUFFICIENT_AMPLIFIED_CPU),
    row("insufficient cpu when scheduling cpuset pod", F + "862-870", U, INSUFFICIENT_AMPLIFIED_CPU),
    row("insufficient cpu when scheduling cpuset pod with cpuset pod on node", F + "871-879", U,
        INSUFFICIENT_AMPLIFIED_CPU),
]

RESV_FILTER = [
    row("filter aligned reservation with nodeInfo", F + "546-589"),
    row("failed to filter aligned reservation with nodeInfo", F + "590-634", U, RESV_INSUFFICIENT),
    row("filter restricted reservation with nodeInfo", F + "635-679"),
    row("failed to filter restricted reservation with nodeInfo", F + "680-724", U, RESV_INSUFFICIENT),
]

# the pod has a required reservation affinity and no reservation matches it
RESV_AFFINITY_CASE = row("failed to reservation affinity", F + "261-269", UU, RESV_AFFINITY)


def main():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "filter_reasons.json")
    with open(path, "w") as f:
        json.dump({"numa_filter": NUMA_FILTER, "numa_filter_amp": NUMA_FILTER_AMP, "resv_filter": RESV_FILTER,
                   "resv_affinity": RESV_AFFINITY_CASE}, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
