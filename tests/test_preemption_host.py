"""koordinator_amd/preemption.py: the assigned-pod table and the preemptor
records from k8s objects (priority, start time, non-preemptible label, quota
ids, pdb_mask as preempt.go:222-267 matches PDBs), and the result view.  No GPU."""
import numpy as np
import pytest

from koordinator_amd import abi, k8s, preemption as pre
from koordinator_amd.config import shipped_profile
from koordinator_amd.marshal import MarshalError, pod_record
from koordinator_amd.topologyspread import LabelSelector

PROF = shipped_profile()


def pod(name, node="", cpu="1", mem="1Gi", prio=None, labels=None, ns="default"):
    return k8s.Pod(namespace=ns, name=name, priority=prio, labels=dict(labels or {}), node_name=node,
                   containers=[k8s.Container(requests=k8s.rl(cpu=cpu, memory=mem))])


def test_assigned_records():
    web = LabelSelector(match_labels=(("app", "web"),))
    pdbs = [pre.PodDisruptionBudget("default", "web", web, 1, disrupted_pods=("w2",)),
            pre.PodDisruptionBudget("other", "web", web, 0),
            pre.PodDisruptionBudget("default", "empty", LabelSelector(), 0),
            pre.PodDisruptionBudget("default", "nil", None, 0)]
    pods = [pod("w1", "n1", prio=100, labels={"app": "web", pre.LABEL_QUOTA_NAME: "team-a"}),
            pod("w2", "n0", "500m", labels={"app": "web", pre.LABEL_PREEMPTIBLE: "false"}),
            pod("w3", "n1", labels={"app": "web"}, ns="other"),
            pod("x", "gone", labels={"app": "web"}),       # not on a snapshot node
            pod("bare", "n0")]
    q = pre.QuotaIds()
    rec, allowed, keys = pre.assigned_records(pods, PROF, {"n0": 0, "n1": 1}, q, pdbs, now_ns=77,
                                              start_time_ns={"default/w1": 5},
                                              in_quota=lambda p: p.name != "bare")
    assert keys == ["default/w1", "default/w2", "other/w3", "default/bare"]
    assert rec["node"].tolist() == [1, 0, 1, 0]
    assert rec["priority"].tolist() == [100, 0, 0, 0]
    assert rec["start_time"].tolist() == [5, 77, 77, 77]
    assert rec["quota"].tolist() == [q.of("team-a"), q.of(pre.DEFAULT_QUOTA_NAME)] + [q.of(pre.DEFAULT_QUOTA_NAME)] * 2
    assert rec["flags"].tolist() == [abi.ASG_IN_QUOTA, abi.ASG_IN_QUOTA | abi.ASG_NONPREEMPTIBLE, abi.ASG_IN_QUOTA, 0]
    # w1: PDB 0; w2 is among PDB 0's DisruptedPods; w3 (namespace other): PDB 1; empty / nil selectors match nothing
    assert rec["pdb_mask"].tolist() == [1, 0, 2, 0]
    assert allowed.tolist() == [1, 0, 0, 0]
    assert rec["qreq"][:, 0].tolist() == [1000, 500, 1000, 1000] and rec["qreq"][0, 1] == 1 << 30
    assert not rec["qreq"][:, 2:].any()
    want = pod_record(pods[1], PROF)
    assert rec["pod"][1].tobytes() == want.tobytes()
    with pytest.raises(MarshalError):
        pre.assigned_records(pods, PROF, {"n0": 0}, q, pdbs * 3)


def test_preemptor_records_and_result_view():
    q = pre.QuotaIds()
    a = q.of("team-a")
    states = {"team-a": pre.QuotaState(used=k8s.rl(cpu="10", memory="4Gi"), runtime=k8s.rl(cpu="12")),
              "team-b": pre.QuotaState(skip=True)}
    pods = [pod("p0", cpu="2", prio=9, labels={pre.LABEL_QUOTA_NAME: "team-a"}),
            pod("p1", labels={pre.LABEL_QUOTA_NAME: "team-b"}),
            pod("p2")]
    rec = pre.preemptor_records(pods, PROF, q, states)
    assert rec["quota"].tolist() == [a, -1, -1]
    assert rec["priority"].tolist() == [9, 0, 0]
    assert rec["q_used"][0].tolist() == [10000, 4 << 30, 0, 0]
    assert rec["q_runtime"][0].tolist() == [12000, 0, 0, 0] and rec["q_mask"][0] == 1   # runtime has cpu only
    assert rec["q_req"][0].tolist() == [2000, 1 << 30, 0, 0]
    assert rec["pod"][0].tobytes() == pod_record(pods[0], PROF).tobytes()
    res = np.zeros((), abi.PREEMPT_RESULT_DTYPE)
    res["node"], res["count"], res["best"]["n_victims"], res["best"]["n_pdb_violations"] = 1, [3, 1, 0, 0, 2], 3, 1
    view = pre.PreemptionResult.of(res, np.array([2, 0, -1], np.int32), ["n0", "n1"], ["a", "b", "c"])
    assert (view.node, view.victims, view.n_victims, view.n_pdb_violations) == ("n1", ["c", "a"], 3, 1)
    assert view.counts == {"candidate": 3, "no_victims": 1, "unfit": 0, "error": 0, "unresolvable": 2}
    res["node"] = -1
    assert pre.PreemptionResult.of(res, np.array([], np.int32), ["n0"], []).node is None
