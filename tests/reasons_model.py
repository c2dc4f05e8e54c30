"""The FitError reasons (abi.REASON_*) of a pod's nodes, computed on the CPU
from the oracle's state: a numpy restatement of the reference's exits.

    NodeResourcesFit   every failing term of upstream fitsRequest over
                       Oracle.state() (one InsufficientResource each)
    NodeNUMAResource   the branch order of nodenumaresource/plugin.go:266-324
                       over the pod record (numa.py's PreFilter state) and
                       Oracle.numa_state(); where the exit is inside Allocate
                       or the topology-policy Admit, the oracle's NUMA status
                       bit is the verdict and the model only names the reason
    the one-reason plugins (static, LoadAware, Reservation affinity) from the
    oracle's status bit

Reservation snapshots are outside the model (Fit on the restored rows has no
model here): masks() refuses them.
"""
import functools

import numpy as np

import diag_model
import oracle
from koordinator_amd import abi

R = abi


def bit(r: int) -> np.uint32:
    return np.uint32(1 << r)


def popcount(words: np.ndarray) -> np.ndarray:
    """[W][n] uint64 -> [n] set bits"""
    b = np.unpackbits(np.ascontiguousarray(words.T).view(np.uint8), axis=1)
    return b.sum(axis=1).astype(np.int64)


def fit_mask(pod, table, state) -> np.ndarray:
    """fitsRequest: 'Too many pods', then podRequest > Allocatable - Requested
    per resource (a zero cpu / memory / ephemeral request still fails an
    over-committed node: 0 > a negative remainder); nothing past the pod count
    for a pod without requests."""
    n = table.n
    m = np.where(state["npods"] + 1 > table["alloc_pods"], bit(R.REASON_FIT_PODS), np.uint32(0))
    fl = int(pod["flags"])
    if not fl & abi.POD_HAS_REQ:
        return m
    slots = [(abi.RES_CPU, R.REASON_FIT_CPU, True), (abi.RES_MEM, R.REASON_FIT_MEM, True),
             (abi.RES_EPH, R.REASON_FIT_EPH, True), (abi.RES_BCPU, R.REASON_FIT_BCPU, bool(fl & abi.POD_REQ_BCPU)),
             (abi.RES_BMEM, R.REASON_FIT_BMEM, bool(fl & abi.POD_REQ_BMEM))]
    for res, slot, on in slots:
        if not on:
            continue
        over = int(pod["req"][res]) > table[f"alloc{res}"].astype(np.int64) - state["requested"][res]
        m = m | np.where(over, bit(slot), np.uint32(0))
    assert m.shape == (n,)
    return m


def amplify(v, ratio):
    return np.where(ratio <= 1.0, v, np.ceil(v * ratio))


def numa_mask(pod, table, state, numa_state, numa_bit: np.ndarray) -> np.ndarray:
    """One reason per node: the first exit of Filter.  numa_bit: the oracle's
    NUMA status bit per node, the verdict of the Allocate / Admit tails."""
    n = table.n
    fl, pol = int(pod["flags"]), int(pod["numa_policy"])
    out = np.zeros(n, np.uint32)
    if fl & abi.POD_NUMA_ERROR:                                     # PreFilter, plugin.go:244
        return out | bit(R.REASON_NUMA_POD_ERROR)
    open_ = np.ones(n, bool)                                        # nodes with no exit taken yet

    def leave(cond, slot=None):
        nonlocal out, open_
        take = open_ & cond
        if slot is not None:
            out = np.where(take, bit(slot), out)
        open_ = open_ & ~cond

    cs = bool(fl & abi.POD_CPUSET)
    skip = bool(fl & abi.POD_NUMA_SKIP)
    cls = table["numa_class"].astype(np.int64)
    nflags = table["numa_flags"].astype(np.int64)
    # filterAmplifiedCPUs, plugin.go:326-363
    cpu = float(pod["req"][abi.RES_CPU])
    ratio = table["numa_amp_cpu"].astype(np.float64)
    if cpu != 0.0:
        req = amplify(np.full(n, cpu), ratio) if (cs and not skip) else np.full(n, cpu)
        allocm = np.where(cls >= 0, numa_state["alloc_cnt"].astype(np.float64) * 1000.0, 0.0)
        requested = state["requested"][abi.RES_CPU].astype(np.float64)
        requested = np.where((requested >= allocm) & (allocm > 0), requested - allocm + amplify(allocm, ratio), requested)
        leave((ratio > 1.0) & (req > table["alloc0"].astype(np.float64) - requested), R.REASON_NUMA_AMP_CPU)
    tp = (nflags >> abi.NODE_NUMA_POLICY_SHIFT) & 3
    if skip:
        return out
    leave(np.full(n, not cs) & (tp == 0))                           # skipTheNode
    leave(cls < 0, R.REASON_NUMA_NO_TOPOLOGY if cs else R.REASON_NUMA_NO_ZONES)
    classes = table.numa_classes
    cpc = np.where(cls >= 0, classes["cpus_per_core"][np.maximum(cls, 0)] if len(classes) else 1, 1).astype(np.int64)
    failing = (numa_bit != 0)
    if not cs:                                                      # a policy node: FilterByNUMANode
        leave(failing, R.REASON_NUMA_POLICY)
        return out
    req_pol, pref = pol & 3, (pol >> 2) & 3
    need = int(pod["numa_cpus"])
    full_only = (nflags & 3) == abi.NODE_CPUBIND_FULL_PCPUS_ONLY
    gate = full_only | (req_pol == abi.CPUBIND_FULL_PCPUS)
    leave(gate & (need % cpc != 0), R.REASON_NUMA_SMT_ALIGN)
    leave(full_only & np.full(n, req_pol != abi.CPUBIND_FULL_PCPUS or pref != abi.CPUBIND_FULL_PCPUS),
          R.REASON_NUMA_FULL_PCPUS_ONLY)
    leave((tp != 0) & failing, R.REASON_NUMA_POLICY)
    leave(tp != 0)
    if req_pol != abi.CPUBIND_NONE:                                 # Allocate, resource_manager.go:257-259 / :442-453
        free = popcount(numa_state["free"])
        leave(failing & (free < need), R.REASON_NUMA_CPUS)
        leave(failing, R.REASON_NUMA_REQUIRED_POLICY)
    return out


def resv_mask(orc: "oracle.Oracle", pod, resv_bit: np.ndarray) -> np.ndarray:
    """filterWithReservations' two exits (reservation/plugin.go:378-381,437),
    told apart by whether the node has a matched reservation (transformer.go:
    86-103); the oracle's Reservation status bit is the verdict."""
    from koordinator_amd.snapshot import slot_col
    table = orc.table
    n, slots = table.n, max(1, table.resv_slots)
    assigned = orc.resv_state()["assigned"].reshape(slots, n)
    matched = np.zeros(n, bool)
    for s in range(slots):
        rf = table[slot_col("resv_flags", s)].astype(np.uint64)
        live = ((rf & abi.RESV_PRESENT) != 0) & ~(((rf & abi.RESV_ALLOCATE_ONCE) != 0) & (assigned[s] > 0))
        group = (rf >> np.uint64(abi.RESV_GROUP_SHIFT)) & np.uint64(abi.RESV_MAX_GROUPS - 1)
        owner = ((np.uint64(pod["resv_match"]) >> group) & np.uint64(1)) != 0
        matched |= live & owner & ((rf & abi.RESV_UNSCHEDULABLE) == 0)
    fail = resv_bit != 0
    assert not (fail & ~matched).any() or int(pod["flags"]) & abi.POD_RESV_AFFINITY
    return np.where(fail, np.where(matched, bit(R.REASON_RESV_INSUFFICIENT), bit(R.REASON_RESV_AFFINITY)), np.uint32(0))


def masks(orc: "oracle.Oracle", pods: np.ndarray) -> np.ndarray:
    """[p][n] reason masks of `pods` on the oracle's current state."""
    table, cfg = orc.table, orc.cfg
    if table["resv_flags"].any():
        raise ValueError("Reservation snapshots are outside the model")
    filt = int(cfg.filter_plugins)
    st = orc.eval(pods, status=True, scores=False)["status"].astype(np.uint32)
    state, numa_state = orc.state(), orc.numa_state()
    out = np.zeros((len(pods), table.n), np.uint32)
    for p, pod in enumerate(pods):
        m = np.zeros(table.n, np.uint32)
        m |= np.where(st[p] & abi.ST_STATIC_FAIL, bit(R.REASON_STATIC), np.uint32(0))
        if filt & abi.PLUGIN_FIT:
            m |= fit_mask(pod, table, state)
        m |= np.where(st[p] & abi.ST_LA_FAIL, bit(R.REASON_LA_USAGE), np.uint32(0))
        if filt & abi.PLUGIN_NUMA:
            m |= numa_mask(pod, table, state, numa_state, st[p] & abi.ST_NUMA_FAIL)
        # no node holds a reservation: the affinity exit is the only one (reservation/plugin.go:378-381)
        m |= np.where(st[p] & abi.ST_RESV_FAIL, bit(R.REASON_RESV_AFFINITY), np.uint32(0))
        out[p] = m
    return out


def records(mask: np.ndarray) -> np.ndarray:
    """koordhip_reasons records of [p][n] reason masks."""
    m = np.atleast_2d(mask).astype(np.uint32)
    rec = np.zeros(len(m), abi.REASONS_DTYPE)
    first = abi.first_reasons(m)
    rec["feasible"] = (m == 0).sum(axis=1)
    rec["unresolvable"] = ((first & np.uint32(abi.REASON_UNRESOLVABLE_MASK)) != 0).sum(axis=1)
    for r in range(abi.REASON_SLOTS):
        rec["any"][:, r] = ((m >> np.uint32(r)) & 1).sum(axis=1)
        rec["first"][:, r] = ((first >> np.uint32(r)) & 1).sum(axis=1)
    return rec


def possible_slots(cfg, table) -> int:
    """The slots the profile and snapshot can produce (reasons.hip reason_slots)."""
    filt = int(cfg.filter_plugins)
    numa = abi.REASONS_OF_BIT[abi.ST_NUMA_FAIL]
    if not (table["numa_amp_cpu"] > 1.0).any():
        numa &= ~(1 << R.REASON_NUMA_AMP_CPU)
    if not ((table["numa_flags"] >> abi.NODE_NUMA_POLICY_SHIFT) & 3).any():
        numa &= ~((1 << R.REASON_NUMA_NO_ZONES) | (1 << R.REASON_NUMA_POLICY))
    s = 0
    if filt & abi.PLUGIN_NODE_STATIC:
        s |= abi.REASONS_OF_BIT[abi.ST_STATIC_FAIL]
    if filt & abi.PLUGIN_FIT:
        s |= abi.REASONS_OF_BIT[abi.ST_FIT_FAIL]
    if filt & abi.PLUGIN_LOADAWARE:
        s |= abi.REASONS_OF_BIT[abi.ST_LA_FAIL]
    if filt & abi.PLUGIN_NUMA:
        s |= numa
    if filt & abi.PLUGIN_RESERVATION:
        s |= 1 << R.REASON_RESV_AFFINITY
    return s


class Model:
    pass


@functools.lru_cache(maxsize=None)
def case(name: str) -> Model:
    """diag_model's case `name` with, per unplaced pod, the reason masks and
    record at the state it was decided on, and the record at the final state.
    Computed once; callers must not modify it."""
    d = diag_model.case(name)
    m = Model()
    m.d = d
    m.mask, m.status = {}, {}
    m.rec = np.zeros(len(d.pods), abi.REASONS_DTYPE)
    m.final_rec = np.zeros(len(d.pods), abi.REASONS_DTYPE)
    seg = oracle.Oracle(d.cfg, d.table)
    prev = 0
    for u in d.unplaced:
        u = int(u)
        seg.place_stream(d.pods[prev:u])
        m.mask[u] = masks(seg, d.pods[u:u + 1])[0]
        m.rec[u] = records(m.mask[u])[0]
        prev = u + 1
    seg.place_stream(d.pods[prev:])
    if len(d.unplaced):
        m.final_rec[d.unplaced] = records(masks(seg, d.pods[d.unplaced]))
    m.differ = np.array([u for u in d.unplaced if m.rec[u] != m.final_rec[u]], np.int64)
    return m


# ------------------------------------------------------------------ the reference's Filter rows
CODE_U, CODE_UU, CODE_E = "Unschedulable", "UnschedulableAndUnresolvable", "Error"
# the engine has one "no class" state for a missing and an invalid CPUTopology
SLOT_OF_TEXT = {"node(s) invalid CPU Topology": R.REASON_NUMA_NO_TOPOLOGY}


def code_of(slot: int) -> str:
    if (abi.REASON_UNRESOLVABLE_MASK >> slot) & 1:
        return CODE_UU
    return CODE_E if (abi.REASON_ERROR_MASK >> slot) & 1 else CODE_U


def slot_of(text: str) -> int:
    from koordinator_amd.diagnosis import REASON_TEXT
    if text in SLOT_OF_TEXT:
        return SLOT_OF_TEXT[text]
    (slot,) = [r for r, s in REASON_TEXT.items() if s == text]
    return slot


def fixture_rows():
    """[(id, fixture row, plugin status bit, profile, table, pod)] for every row of
    tests/golden/filter_reasons.json, built as the plugins' own known-answer tests
    build them (golden_cases.py)."""
    import golden_cases as G
    from koordinator_amd import marshal
    from koordinator_amd import reservation as rv
    want = G.load("filter_reasons.json")
    rows = []
    cases = dict(G.numa_plugin_cases("filter"))
    for w in want["numa_filter"]:
        prof, t, pod, _ = G.build_numa_plugin_case(cases[w["name"]])
        rows.append(("numa:" + w["name"], w, abi.ST_NUMA_FAIL, prof, t, pod))
    cases = dict(G.numa_plugin_cases("filter_amp"))
    for w in want["numa_filter_amp"]:
        prof, t, pod = G.build_numa_filter_amp_case(cases[w["name"]])
        rows.append(("amp:" + w["name"], w, abi.ST_NUMA_FAIL, prof, t, pod))
    cases = {c["name"]: c for c in G.reservation_cases()["filter"]}
    node = ("test-node", {"cpu": "32", "memory": "32Gi", "pods": "100"})
    zero = G.rlist({"x": "0"})["x"]
    for w in want["resv_filter"]:
        c = cases[w["name"]]
        # NodeInfo pods: the reserve pod (its Allocatable) and a pod holding the rest of podRequested
        req = c["pod_requested"]
        rest = {k: str(G.rlist(req)[k].v - G.rlist(c["reservation"]["allocatable"]).get(k, zero).v) for k in req}
        prof = G.resv_profile()
        r = rv.Reservation(name="r", node_name=node[0], allocatable=G.rlist(c["reservation"]["allocatable"]),
                           allocated=G.rlist(c["reservation"].get("allocated") or {}), owners=G.match_all_owner(),
                           labels={}, allocate_policy=c["policy"], allocate_once=None, assigned=0)
        t, idx = G.build_resv_nodes([node], [r], prof, {node[0]: [G.resv_pod(rest, name="filler")]})
        pod = marshal.pod_records([G.resv_pod(c["pod"])], prof, idx)
        rows.append(("resv:" + w["name"], w, abi.ST_RESV_FAIL, prof, t, pod))
    # a required reservation affinity and no reservation to match
    w = want["resv_affinity"]
    prof = G.resv_profile()
    t, idx = G.build_resv_nodes([node], [], prof)
    pod = marshal.pod_records([G.resv_pod({"cpu": "1"})], prof, idx)
    pod["flags"] |= abi.POD_RESV_AFFINITY
    rows.append(("resv:" + w["name"], w, abi.ST_RESV_FAIL, prof, t, pod))
    return rows


def check_fixture_row(w, status_bit: int, mask: int):
    """The plugin's part of a node's reason mask against the fixture row."""
    got = int(mask) & abi.REASONS_OF_BIT[status_bit]
    if w["code"] == "Success":
        assert got == 0, (w["source"], hex(got))
        return
    slot = slot_of(w["reason"])
    assert got == 1 << slot, (w["source"], hex(got), slot)
    assert code_of(slot) == w["code"], w["source"]


# ------------------------------------------------------------------ the random cases
GI = 2**30


def tighten(table, pods, seed=diag_model.SEED):
    """Node rows and pods that reach every NodeResourcesFit term: nodes full of
    pods, nodes out of cpu / memory / ephemeral-storage (overlapping, so several
    terms fail on one node), over-committed nodes (the zero-request branch) and
    pods that request ephemeral-storage."""
    from koordinator_amd import synth
    n = table.n
    u = [synth.uniform(seed, n, 920 + k) for k in range(6)]
    if n == 1:
        u = [np.zeros(1)] * 4 + [np.ones(1), np.zeros(1)]
    full, cpu, mem, eph, over = (u[0] < 0.25), (u[1] < 0.4), (u[2] < 0.4), (u[3] < 0.4), (u[4] < 0.1)
    batch = u[5] < 0.4
    table["requested3"][batch] = table["alloc3"][batch]
    table["requested4"][batch] = table["alloc4"][batch]
    table["npods"][full] = table["alloc_pods"][full]
    table["requested0"][cpu] = table["alloc0"][cpu] - 100
    table["requested1"][mem] = table["alloc1"][mem] - 64 * 2**20
    table["alloc2"][:] = 100 * GI
    table["requested2"][eph] = 99 * GI
    table["requested0"][over] = table["alloc0"][over] + 1000
    table["requested1"][over] = table["alloc1"][over] + GI
    req = pods["req"]
    has = (pods["flags"] & abi.POD_HAS_REQ) != 0
    req[has & (np.arange(len(pods)) % 2 == 0), abi.RES_EPH] = 2 * GI
    return table, pods


@functools.lru_cache(maxsize=None)
def current_case(name: str):
    """(profile, table, pods) of a current-state case.  Computed once; callers
    must not modify it.
      base-<n>-<pods>  the shipped Fit + LoadAware profile on a tightened cluster
      numa             diag_model's case C (70 pods) with PreFilter-error and skipped pods
      numa-ext         ... with amplified nodes, topology-policy nodes and the static filters"""
    from koordinator_amd import synth
    from koordinator_amd.config import shipped_profile, with_upstream
    if name.startswith("base-"):
        n, n_pods = (int(x) for x in name.split("-")[1:])
        prof = shipped_profile()
        table = synth.make_cluster(synth.ClusterSpec(n), prof)
        pods = synth.make_pods(synth.StreamSpec(n_pods, be_frac=0.3), prof)
        pods["flags"][::3] |= abi.POD_DAEMONSET
        tighten(table, pods)
        return prof, table, pods
    if name == "numa":
        d = diag_model.case("C")
        pods = d.pods[:70].copy()
        cs = np.flatnonzero(pods["flags"] & abi.POD_CPUSET)
        pods["flags"][cs[0]] |= abi.POD_NUMA_ERROR
        pods["flags"][cs[1]] |= abi.POD_NUMA_SKIP
        return d.prof, d.table, pods
    if name == "numa-ext":
        prof = with_upstream(shipped_profile(numa=True))
        n = 301
        table = synth.make_cluster(synth.ClusterSpec(n), prof)
        synth.add_numa(table, synth.NumaSpec(policy_frac=0.25, amp_frac=0.25, no_topology_frac=0.1), prof)
        pods = synth.make_pods(synth.StreamSpec(70, be_frac=0.2, cpuset_frac=0.5), prof)
        synth.add_static(table, pods, synth.StaticSpec(), prof)
        free = (synth.uniform(diag_model.SEED, n, 901) * 6000).astype(np.int64)
        table["requested0"][:] = np.maximum(table["requested0"], table["alloc0"] - free)
        tighten(table, pods)
        cs = np.flatnonzero(pods["flags"] & abi.POD_CPUSET)
        pods["flags"][cs[0]] |= abi.POD_NUMA_ERROR
        # nodes with two free CPUs left (Allocate's "not enough cpus"), and topology-policy nodes
        # without a CPU topology ("missing NUMA resources" for a pod without a cpuset)
        few = (synth.uniform(diag_model.SEED, n, 931) < 0.2) & (table["numa_class"] >= 0)
        ncpu = table.numa_classes["num_cpus"][np.maximum(table["numa_class"], 0)]
        for w in range(abi.NUMA_WORDS):
            table[f"numa_free{w}"][few] &= np.uint64(3 if w == 0 else 0)
        left = popcount(np.stack([table[f"numa_free{w}"] for w in range(abi.NUMA_WORDS)]))
        table["numa_alloc_cnt"][few] = (ncpu - left)[few]
        bare = np.flatnonzero(table["numa_class"] < 0)[::2]
        table["numa_flags"][bare] |= abi.NUMA_TOPO_SINGLE_NUMA_NODE << abi.NODE_NUMA_POLICY_SHIFT
        return prof, table, pods
    raise KeyError(name)


def resv_case():
    """The 400-node Reservation snapshot of the GPU test, some pods with a required reservation affinity."""
    from koordinator_amd import synth
    from koordinator_amd.config import shipped_profile
    prof = shipped_profile(numa=True, reservation=True)
    table = synth.make_cluster(synth.ClusterSpec(400), prof)
    synth.add_numa(table, synth.NumaSpec(), prof)
    synth.add_reservations(table, synth.ResvSpec(aligned_frac=0.3, restricted_frac=0.3))
    pods = synth.make_pods(synth.StreamSpec(40, be_frac=0.3, cpuset_frac=0.3, resv_match_frac=0.5,
                                            resv_affinity_frac=0.3), prof)
    return prof, table, pods


CURRENT_CASES = ("base-1-3", "base-63-7", "base-1003-70", "numa", "numa-ext")
