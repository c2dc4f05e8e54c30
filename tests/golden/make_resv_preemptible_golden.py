"""Writes resv_preemptible_cases.json: the reference-held vectors of the
Reservation plugin's preemptible cycle state (data only).

  filter       the twelve rows of Test_filterWithReservations that carry
               preemption state (reservation/plugin_test.go:725-1202): four
               without a matched reservation, eight with one Default or
               Restricted reservation and preemption from the node
               (`preemptible`), from the reservation (`in_rr`, keyed by the
               reservation's UID) or both.  want: null passes, else the status
               reason.
  add / remove the rows of TestPreFilterExtensionAddPod / RemovePod (:1222-1440):
               the state before, the pod (its cpu request, whether its
               reservation-allocated annotation names the reservation) and the
               state after.

The test node: allocatable cpu 32, memory 32Gi, pods 100 (:528-539), no pods on
the NodeInfo.  Quantities in milli-CPU and bytes; an absent key is absent in
the reference's map too.
"""
import json
import os

S = "reservation/plugin_test.go:"
GI = 2**30
PREEMPTION_FAILED = "ErrReasonPreemptionFailed"
INSUFFICIENT = "ErrReasonReservationInsufficientResources"


def resv(policy, names=None):
    """The rows' one matched reservation: UID 123456, Allocatable = Allocated = cpu 6."""
    return {"policy": policy, "allocatable": {"cpu": 6000}, "allocated": {"cpu": 6000}, "resource_names": names}


FILTER = [
    {"name": "filter non-reservations with preemption", "source": S + "725-745", "pod": {"cpu": 4000},
     "preemptible": {"cpu": 4000}, "in_rr": None, "pod_requested": {"cpu": 32000}, "r_allocated": None,
     "reservation": None, "want": None},
    {"name": "filter non-reservations with preemption but no preemptible resources", "source": S + "746-762",
     "pod": {"cpu": 4000}, "preemptible": None, "in_rr": None, "pod_requested": {"cpu": 32000}, "r_allocated": None,
     "reservation": None, "want": None},
    {"name": "filter non-reservations with preemption but no preemptible resources and have preemptibleInRR",
     "source": S + "763-786", "pod": {"cpu": 4000}, "preemptible": None, "in_rr": {"cpu": 4000},
     "pod_requested": {"cpu": 32000}, "r_allocated": None, "reservation": None, "want": PREEMPTION_FAILED},
    {"name": "filter non-reservations with preemption", "source": S + "787-807", "pod": {"cpu": 4000},
     "preemptible": {"cpu": 2000}, "in_rr": None, "pod_requested": {"cpu": 32000}, "r_allocated": None,
     "reservation": None, "want": PREEMPTION_FAILED},
    {"name": "filter default reservations with preemption", "source": S + "808-852", "pod": {"cpu": 4000},
     "preemptible": None, "in_rr": {"cpu": 4000}, "pod_requested": {"cpu": 36000}, "r_allocated": {"cpu": 6000},
     "reservation": resv("Default"), "want": None},
    {"name": "filter default reservations with preempt from reservation and node", "source": S + "853-902",
     "pod": {"cpu": 4000}, "preemptible": {"cpu": 2000}, "in_rr": {"cpu": 2000}, "pod_requested": {"cpu": 38000},
     "r_allocated": {"cpu": 6000}, "reservation": resv("Default"), "want": None},
    {"name": "failed to filter default reservations with preempt from reservation", "source": S + "903-947",
     "pod": {"cpu": 4000}, "preemptible": None, "in_rr": {"cpu": 2000}, "pod_requested": {"cpu": 38000},
     "r_allocated": {"cpu": 6000}, "reservation": resv("Default"), "want": INSUFFICIENT},
    {"name": "failed to filter default reservations with preempt from node", "source": S + "948-990",
     "pod": {"cpu": 4000}, "preemptible": {"cpu": 2000}, "in_rr": None, "pod_requested": {"cpu": 38000},
     "r_allocated": {"cpu": 6000}, "reservation": resv("Default"), "want": INSUFFICIENT},
    {"name": "filter restricted reservations with preempt from reservation", "source": S + "991-1039",
     "pod": {"cpu": 4000}, "preemptible": None, "in_rr": {"cpu": 4000}, "pod_requested": {"cpu": 38000},
     "r_allocated": {"cpu": 6000}, "reservation": resv("Restricted"), "want": None},
    {"name": "failed to filter restricted reservations with preempt from node", "source": S + "1040-1087",
     "pod": {"cpu": 4000}, "preemptible": {"cpu": 4000}, "in_rr": None, "pod_requested": {"cpu": 38000},
     "r_allocated": {"cpu": 6000}, "reservation": resv("Restricted"), "want": INSUFFICIENT},
    {"name": "failed to filter restricted reservations with preempt from reservation and node",
     "source": S + "1088-1144", "pod": {"cpu": 4000}, "preemptible": {"cpu": 2000}, "in_rr": {"cpu": 2000},
     "pod_requested": {"cpu": 38000}, "r_allocated": {"cpu": 6000}, "reservation": resv("Restricted", ["cpu"]),
     "want": INSUFFICIENT},
    {"name": "filter restricted reservations with preempt from reservation and node", "source": S + "1145-1203",
     "pod": {"cpu": 4000, "memory": 4 * GI}, "preemptible": {"memory": 32 * GI}, "in_rr": {"cpu": 4000},
     "pod_requested": {"cpu": 38000}, "r_allocated": {"cpu": 6000}, "reservation": resv("Restricted", ["cpu"]),
     "want": None},
]

NONE = {"preemptible": None, "in_rr": None}
ADD = [
    {"name": "with BestEffort Pod", "source": S + "1236-1245", "pod_cpu": 0, "bound": False, "state": NONE, "want": NONE},
    {"name": "preempt normal pod", "source": S + "1246-1276", "pod_cpu": 4000, "bound": False,
     "state": {"preemptible": {"cpu": 4000}, "in_rr": None}, "want": NONE},
    {"name": "preempt pod allocated in reservation", "source": S + "1277-1310", "pod_cpu": 4000, "bound": True,
     "state": {"preemptible": None, "in_rr": {"cpu": 4000}}, "want": NONE},
]
REMOVE = [
    {"name": "with BestEffort Pod", "source": S + "1350-1355", "pod_cpu": 0, "bound": False, "state": NONE, "want": NONE},
    {"name": "preempt normal pod", "source": S + "1356-1382", "pod_cpu": 4000, "bound": False, "state": NONE,
     "want": {"preemptible": {"cpu": 4000}, "in_rr": None}},
    {"name": "preempt pod allocated in reservation", "source": S + "1383-1412", "pod_cpu": 4000, "bound": True,
     "state": NONE, "want": {"preemptible": None, "in_rr": {"cpu": 4000}}},
]


def main():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resv_preemptible_cases.json")
    with open(path, "w") as f:
        json.dump({"node": {"alloc_cpu": 32000, "alloc_memory": 32 * GI, "alloc_pods": 100, "pods": 0},
                   "filter": FILTER, "add": ADD, "remove": REMOVE}, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
