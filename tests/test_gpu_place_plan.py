"""The shape a place call takes (csrc/place_plan.hpp plan_place), seen from
outside: pods per round, pipeline depth, rounds, the shard-local flag and the
evaluation / resolve kernels of the last call, for every knob and profile that
changes a decision -- and the placements equal the oracle's every time.  The
expected values are worked out from the rules: lag 2 with two evaluation
streams unless the kernels keep side rows without reservations, 3P <= 128 and
2P <= 64 for lag 2, the class lists where (2048 - K) / P >= 50."""
import functools

import numpy as np
import pytest

import oracle
from koordinator_amd import abi, synth
from koordinator_amd.config import shipped_profile, to_c_config, with_deviceshare

pytestmark = pytest.mark.gpu

N_NODES, N_PODS = 400, 600
# the evaluation where the class lists do not run: k_scan (+ select) on the plain profile, the fused k_eval_topk
# with NodeNUMAResource (whose stream of this size does not take the class lists)
CLS, SCAN, TOPK, RES, SEQ = "kh::k_cls_run", "kh::k_scan", "kh::k_eval_topk", "kh::k_resolve", "kh::k_seq"


def _profile(kind):
    if kind == "device":
        return with_deviceshare(shipped_profile())
    return shipped_profile(numa=kind == "numa")


@functools.lru_cache(maxsize=None)
def _workload(kind):
    """Cluster, pods, ext records and the oracle's placements of one profile
    kind (they depend on neither the round size nor a knob): computed once."""
    prof = _profile(kind)
    t = synth.make_cluster(synth.ClusterSpec(N_NODES), prof)
    ext = None
    if kind == "numa":
        synth.add_numa(t, synth.NumaSpec(), prof)
    if kind == "device":
        synth.add_devices(t, synth.DevSpec())
        ext = synth.make_device_ext(N_PODS, synth.DevStreamSpec(frac=0.1))
    pods = synth.make_pods(synth.StreamSpec(N_PODS, be_frac=0.3, cpuset_frac=0.4 if kind == "numa" else 0.0), prof)
    o = oracle.Oracle(to_c_config(prof), t)
    ref = o.place_stream_ext(pods, ext) if kind == "device" else o.place_stream(pods)
    ref.setflags(write=False)
    return t, pods, ext, ref


# id: (profile kind, batch_pods, knob, one-rank communicator) -> round_pods, lag, rounds, local, eval, resolve
CASES = {
    "default_b16": (("plain", 16, None, False), (16, 2, 38, False, CLS, RES)),
    "b32": (("plain", 32, None, False), (32, 2, 19, False, CLS, RES)),
    "b40": (("plain", 40, None, False), (40, 1, 15, False, SCAN, RES)),  # 2P > 64: lag 1; amax 49: no class lists
    "numa": (("numa", 16, None, False), (16, 1, 38, False, TOPK, RES)),  # side rows, no reservations: lag 1
    "numa_lag2": (("numa", 16, "KOORDHIP_LAG2", False), (16, 2, 38, False, TOPK, RES)),
    "lag1": (("plain", 16, "KOORDHIP_LAG1", False), (16, 1, 38, False, CLS, RES)),
    "cls_off": (("plain", 16, "KOORDHIP_CLS_OFF", False), (16, 2, 38, False, SCAN, RES)),
    "one_eval_stream": (("plain", 16, "KOORDHIP_ONE_EVAL_STREAM", False), (16, 1, 38, False, SCAN, RES)),
    "serial": (("plain", 16, "KOORDHIP_SERIAL", False), (16, 1, 38, False, SCAN, RES)),
    "round_launch": (("plain", 16, "KOORDHIP_ROUND_LAUNCH", False), (16, 1, 38, False, SCAN, RES)),
    "shard_local_sim": (("plain", 16, "KOORDHIP_SHARD_LOCAL_SIM", False), (16, 2, 38, True, CLS, RES)),
    "one_rank_comm": (("plain", 16, None, True), (16, 2, 38, False, SCAN, RES)),  # the exchange: no class lists
    "device_pipe": (("device", 16, None, False), (16, 2, 38, False, CLS, RES)),
    "device_ext_seq": (("device", 16, "KOORDHIP_EXT_SEQ", False), (1, 0, 600, False, SEQ, SEQ)),
}


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_place_call_shape(case, monkeypatch):
    import torch  # noqa: F401  (device discovery only; the engine is plain HIP)
    from koordinator_amd.engine import PlacementEngine
    (kind, batch, knob, comm), (round_pods, lag, rounds, local, ev, rs) = CASES[case]
    if knob:
        monkeypatch.setenv(knob, "1")
    t, pods, ext, ref = _workload(kind)
    prof = _profile(kind)
    prof.batch_pods = batch
    with PlacementEngine(prof, device=0) as e:
        if comm:
            e.comm_init(PlacementEngine.comm_unique_id(), 1, 0)
        e.load_snapshot(t)
        got = e.place_stream_ext(pods, ext) if kind == "device" else e.place_stream(pods)
        ks = e.kernel_stats()
        names = e.kernel_names()
    seen = (int(ks["round_pods"]), int(ks["lag"]), int(ks["rounds"]), bool(int(ks["flags"]) & abi.KSTAT_LOCAL))
    print(f"{case}: round_pods, lag, rounds, local = {seen}; kernels {names}")
    assert seen == (round_pods, lag, rounds, local)
    assert names["eval"].startswith(ev) and names["resolve"].startswith(rs), names
    assert np.array_equal(got, ref), int(np.flatnonzero(got != ref)[0])
