"""The unschedulable-pod diagnosis, computed with the CPU oracle alone: the
inputs whose streams leave interleaved unplaced pods, and for each unplaced
pod the koordhip_diag record at the state it was decided on (the commits of
the pods before it) and, for comparison, at the state the stream ends in.

    Oracle.place_stream on a prefix   -> the decision state
    Oracle.eval(status)               -> the status bits at that state
"""
import functools

import numpy as np

import oracle
from koordinator_amd import abi, synth
from koordinator_amd.config import shipped_profile, to_c_config

SEED = synth.SEED

# name -> (numa, n, n_pods, be, slack_m, cf)
CASES = {
    "A": (False, 203, 900, 0.3, 3000, 0.0),
    "B": (False, 77, 500, 0.5, 3000, 0.0),
    "C": (True, 301, 800, 0.2, 6000, 0.5),
}
# batch_pods the engine runs each case at
BATCHES = {"A": (0, 17), "B": (1,), "C": (0, 17)}


def inputs(numa, n, n_pods, be, slack_m, cf):
    """A cluster tightened to `slack_m` milli-CPU of free capacity at most, and a stream over it."""
    prof = shipped_profile(numa=numa)
    table = synth.make_cluster(synth.ClusterSpec(n, seed=SEED), prof)
    if numa:
        synth.add_numa(table, synth.NumaSpec(), prof)
    free = (synth.uniform(SEED, n, 901) * slack_m).astype(np.int64)
    table["requested0"][:] = np.maximum(table["requested0"], table["alloc0"] - free)
    pods = synth.make_pods(synth.StreamSpec(n_pods, be_frac=be, seed=SEED, cpuset_frac=cf), prof)
    pods["flags"][::3] |= abi.POD_DAEMONSET
    return prof, table, pods


def records(status: np.ndarray) -> np.ndarray:
    """koordhip_diag records of [p][n] status bytes."""
    st = np.atleast_2d(status).astype(np.uint32)
    rec = np.zeros(len(st), abi.DIAG_DTYPE)
    rec["feasible"] = (st == 0).sum(axis=1)
    left = np.ones(st.shape, bool)          # nodes no earlier plugin of the Filter order failed
    for bit in abi.FILTER_ORDER:
        b = bit.bit_length() - 1
        has = (st & bit) != 0
        rec["any"][:, b] = has.sum(axis=1)
        rec["first"][:, b] = (has & left).sum(axis=1)
        left &= ~has
    assert not (st & ~np.uint32(sum(abi.FILTER_ORDER))).any(), "a status bit outside the Filter order"
    return rec


class Model:
    pass


@functools.lru_cache(maxsize=None)
def case(name: str) -> Model:
    """The case's inputs, the oracle's placements and, per unplaced pod, its
    decision-state status / record and final-state record.  Computed once;
    callers must not modify it."""
    prof, table, pods = inputs(*CASES[name])
    cfg = to_c_config(prof)
    m = Model()
    m.name, m.prof, m.table, m.pods, m.cfg = name, prof, table, pods, cfg
    whole = oracle.Oracle(cfg, table)
    m.out, m.cpusets = whole.place_stream(pods, cpusets=True)
    m.unplaced = np.flatnonzero(m.out < 0)
    m.final_rec = np.zeros(len(pods), abi.DIAG_DTYPE)
    if len(m.unplaced):
        m.final_rec[m.unplaced] = records(whole.eval(pods[m.unplaced], status=True, scores=False)["status"])
    m.final_state, m.final_numa = whole.state(), whole.numa_state()
    seg = oracle.Oracle(cfg, table)
    m.status = {}
    m.rec = np.zeros(len(pods), abi.DIAG_DTYPE)
    prev = 0
    for u in m.unplaced:
        u = int(u)
        got = seg.place_stream(pods[prev:u])
        assert np.array_equal(got, m.out[prev:u])
        st = seg.eval(pods[u:u + 1], status=True, scores=False)["status"][0].copy()
        m.status[u] = st
        m.rec[u] = records(st)[0]
        prev = u + 1  # pod u itself commits nothing
    m.differ = np.array([u for u in m.unplaced if m.rec[u] != m.final_rec[u]], np.int64)
    return m
