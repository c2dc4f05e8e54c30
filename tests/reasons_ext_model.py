"""The FitError reasons of the sequential cycle's plugins (abi.REASON_FIT_X0 ..
REASON_IPA_ANTI, koordhip_diagnose_reasons_ext / koordhip_node_reasons_ext),
computed on the CPU from the oracle's state: a numpy restatement of the four
groups, ORed with reasons_model's masks of the base plugins.

    NodeResourcesFit    the extended scalars: one reason per failing scalar of
                        upstream fitsRequest over the xalloc column and
                        Oracle.dev_state()'s Requested; on a node whose
                        reservation holds devices, over the restored scalars
                        (the reservation's Allocatable leaves, an unmatched
                        one's remainder comes back: Oracle.resv_scalar_state())
    DeviceShare         one slot; the oracle's DEVICE status bit is the verdict
    PodTopologySpread   calPreFilterState over Oracle.pts_counts() and the
                        pts_dom / pts_elig columns, then Filter's loop over the
                        pod's DoNotSchedule constraints in record order: the
                        first failing one says missing label or skew
    InterPodAffinity    the pair sums of Oracle.ipa_counts(); satisfyPodAffinity
                        before the anti-affinity checks

Reservation snapshots: NodeResourcesFit's FIT_* slots and NodeNUMAResource on
the restored rows have no model (reasons_model.py); masks() leaves those two
groups out there and says so in its second result, and the callers compare them
at the level of the status bit.

CASES are diag_ext_model's, resv-scalars (its resv case made to depend on the
restored scalars) and "directed": a small table written by hand, with
hand-written expected masks, for the exits the synthetic streams never reach.
"""
import copy
import functools

import numpy as np

import diag_ext_model as X
import oracle
import reasons_model as RM
from koordinator_amd import abi, synth
from koordinator_amd.config import (shipped_profile, to_c_config, with_deviceshare, with_interpod_affinity,
                                    with_topology_spread)
from koordinator_amd.snapshot import IpaMeta, PtsMeta, slot_col

bit = RM.bit
OF = abi.REASONS_OF_BIT_EXT
FIT_ALL = OF[abi.ST_FIT_FAIL] | OF[abi.ST_XFIT_FAIL]
EXT_GROUPS = OF[abi.ST_XFIT_FAIL] | OF[abi.ST_DEVICE_FAIL] | OF[abi.ST_PTS_FAIL] | OF[abi.ST_IPA_FAIL]
# the groups without a model on a Reservation snapshot
RESTORED_ROW_GROUPS = OF[abi.ST_FIT_FAIL] | OF[abi.ST_NUMA_FAIL]


# ------------------------------------------------------------------ NodeResourcesFit, the extended scalars
def resv_class(orc, pod, h: np.ndarray) -> np.ndarray:
    """[n] the restore class of each node's reservation slot h[i] for the pod
    (1 matched, 2 unmatched with assigned pods, 0 neither / h < 0)."""
    table = orc.table
    n, slots = table.n, max(1, table.resv_slots)
    assigned = orc.resv_state()["assigned"].reshape(slots, n)
    out = np.zeros(n, np.int64)
    for s in range(slots):
        rf = table[slot_col("resv_flags", s)].astype(np.uint64)
        rn = assigned[s]
        present = ((rf & abi.RESV_PRESENT) != 0) & ~(((rf & abi.RESV_ALLOCATE_ONCE) != 0) & (rn > 0))
        group = (rf >> np.uint64(abi.RESV_GROUP_SHIFT)) & np.uint64(abi.RESV_MAX_GROUPS - 1)
        match = ((np.uint64(pod["resv_match"]) >> group) & np.uint64(1)) != 0
        cls = np.where(present, np.where(match & ((rf & abi.RESV_UNSCHEDULABLE) == 0), 1, np.where(rn > 0, 2, 0)), 0)
        out = np.where(h == s, cls, out)
    return out


def xfit_mask(orc, pod, x) -> np.ndarray:
    table = orc.table
    n = table.n
    m = np.zeros(n, np.uint32)
    if x is None or not int(x["xmask"]) or not table.has_ext:
        return m
    alloc = table["xalloc"].astype(np.int64)
    req = orc.dev_state()["xrequested"]
    restored = np.zeros(n, bool)
    if table.has_resv_dev and table["resv_xalloc"].any() and table["resv_flags"].any():
        h = table["resv_dev_slot"].astype(np.int64)
        restored = (h >= 0) & (h < max(1, table.resv_slots))
        cls = resv_class(orc, pod, np.where(restored, h, -1))
        A = table["resv_xalloc"].astype(np.int64)
        D = orc.resv_scalar_state()
        rem = np.maximum(A - D, 0)
    for j in range(abi.NXRES):
        if not (int(x["xmask"]) >> j) & 1:
            continue
        px = int(x["xreq"][j])
        over = px > alloc[:, j] - req[:, j]
        if restored.any():
            back = req[:, j] - np.where(cls != 0, A[:, j], 0) + np.where(cls == 2, rem[:, j], 0)
            over = np.where(restored, px > alloc[:, j] - back, over)
        m |= np.where(over, bit(abi.REASON_FIT_X0 + j), np.uint32(0))
    return m


# ------------------------------------------------------------------ PodTopologySpread
def pts_mask(orc, x, filt: bool) -> np.ndarray:
    table = orc.table
    n = table.n
    out = np.zeros(n, np.uint32)
    meta = table.pts
    if not filt or x is None or meta is None or meta.keys <= 0 or int(x["pts_n"]) == 0:
        return out
    dom = table["pts_dom"].astype(np.int64)
    cnt = orc.pts_counts().astype(np.int64)
    elig = ((table["pts_elig"].astype(np.int64) >> (2 * int(x["pts_class"]))) & 1) != 0
    hard = [j for j in range(int(x["pts_n"])) if int(x["pts_fl"][j]) & abi.PTS_HARD]
    key_of = lambda j: meta.cons_key[int(x["pts_c"][j])]
    # TpPairToMatchNum: the pairs of the eligible nodes, summed over every node of such a pair
    pres, match, mn = {}, {}, {}
    for k in {key_of(j) for j in hard}:
        D = n if (meta.hostname >> k) & 1 else meta.ndom[k]
        pres[k] = np.zeros(max(D, 1), bool)
        d = dom[:, k]
        pres[k][d[elig & (d >= 0)]] = True
        match[k] = np.zeros(max(D, 1), np.int64)
    for j in hard:
        k = key_of(j)
        d = dom[:, k]
        ok = (d >= 0) & pres[k][np.maximum(d, 0)]
        np.add.at(match[k], d[ok], cnt[ok, int(x["pts_c"][j])])
    for k in pres:
        mn[k] = match[k][pres[k]].min() if pres[k].any() else np.iinfo(np.int32).max
    open_ = np.ones(n, bool)
    for j in hard:
        k = key_of(j)
        d = dom[:, k]
        missing = open_ & (d < 0)
        out = np.where(missing, bit(abi.REASON_PTS_MISSING_LABEL), out)
        open_ &= ~missing
        self_ = 1 if int(x["pts_fl"][j]) & abi.PTS_SELF else 0
        m = np.where(pres[k][np.maximum(d, 0)], match[k][np.maximum(d, 0)], 0)
        skew = open_ & (m + self_ - mn[k] > int(x["pts_skew"][j]))
        out = np.where(skew, bit(abi.REASON_PTS_SKEW), out)
        open_ &= ~skew
    return out


# ------------------------------------------------------------------ InterPodAffinity
def ipa_mask(orc, x, filt: bool) -> np.ndarray:
    table = orc.table
    n = table.n
    out = np.zeros(n, np.uint32)
    if not filt or x is None or table.ipa is None or table.pts is None or not table.ipa.ent_key:
        return out
    aff, anti = int(x["ipa_aff"]), int(x["ipa_anti"])
    if not (aff | anti):
        return out
    dom = table["pts_dom"].astype(np.int64)
    cnt = orc.ipa_counts().astype(np.int64)
    meta = table.pts

    def pair_maps(mask):
        maps = {}
        for e, k in enumerate(table.ipa.ent_key):
            if not (mask >> e) & 1:
                continue
            D = n if (meta.hostname >> k) & 1 else meta.ndom[k]
            m = maps.setdefault(k, np.zeros(max(D, 1), np.int64))
            d = dom[:, k]
            np.add.at(m, d[d >= 0], cnt[d >= 0, e])
        return maps

    fail_aff = np.zeros(n, bool)
    if aff:
        maps = pair_maps(aff)
        empty = not any(m.any() for m in maps.values())
        exist = np.ones(n, bool)
        for e, k in enumerate(table.ipa.ent_key):
            if not (aff >> e) & 1:
                continue
            d = dom[:, k]
            fail_aff |= d < 0                                           # all topology labels must exist on the node
            exist &= np.where(d >= 0, maps[k][np.maximum(d, 0)] > 0, False)
        first_of_series = empty and bool(int(x["ipa_flags"]) & abi.IPA_SELF)
        fail_aff |= ~exist & (not first_of_series)
    fail_anti = np.zeros(n, bool)
    for k, m in pair_maps(anti).items():
        d = dom[:, k]
        fail_anti |= (d >= 0) & (m[np.maximum(d, 0)] > 0)
    out = np.where(fail_anti, bit(abi.REASON_IPA_ANTI), out)
    return np.where(fail_aff, bit(abi.REASON_IPA_AFFINITY), out)          # satisfyPodAffinity runs first


# ------------------------------------------------------------------ the masks and records
def masks(orc: "oracle.Oracle", pods: np.ndarray, ext):
    """([p][n] reason masks of (pods, ext) on the oracle's current state, the
    groups left out of them: RESTORED_ROW_GROUPS on a Reservation snapshot, else 0)."""
    table, cfg = orc.table, orc.cfg
    filt = int(cfg.filter_plugins)
    st = orc.eval_ext(pods, ext, status=True, scores=False)["status"].astype(np.uint32)
    resv = bool(table["resv_flags"].any())
    out = np.zeros((len(pods), table.n), np.uint32)
    if not resv:
        out |= RM.masks(orc, pods)
    for p, pod in enumerate(pods):
        x = None if ext is None else ext[p]
        m = out[p]
        if resv:
            m |= np.where(st[p] & abi.ST_STATIC_FAIL, bit(abi.REASON_STATIC), np.uint32(0))
            m |= np.where(st[p] & abi.ST_LA_FAIL, bit(abi.REASON_LA_USAGE), np.uint32(0))
            m |= RM.resv_mask(orc, pod, st[p] & abi.ST_RESV_FAIL)
        if filt & abi.PLUGIN_FIT:
            m |= xfit_mask(orc, pod, x)
        m |= np.where(st[p] & abi.ST_DEVICE_FAIL, bit(abi.REASON_DEVICE_INSUFFICIENT), np.uint32(0))
        m |= pts_mask(orc, x, bool(filt & abi.PLUGIN_PTS))
        m |= ipa_mask(orc, x, bool(filt & abi.PLUGIN_IPA))
    return out, (RESTORED_ROW_GROUPS if resv else 0)


def records(mask: np.ndarray) -> np.ndarray:
    """koordhip_reasons records of [p][n] reason masks, `first` in abi.FILTER_ORDER_EXT."""
    m = np.atleast_2d(mask).astype(np.uint32)
    rec = np.zeros(len(m), abi.REASONS_DTYPE)
    first = abi.first_reasons_ext(m)
    rec["feasible"] = (m == 0).sum(axis=1)
    rec["unresolvable"] = ((first & np.uint32(abi.REASON_EXT_UNRESOLVABLE_MASK)) != 0).sum(axis=1)
    for r in range(abi.REASON_SLOTS):
        rec["any"][:, r] = ((m >> np.uint32(r)) & 1).sum(axis=1)
        rec["first"][:, r] = ((first >> np.uint32(r)) & 1).sum(axis=1)
    return rec


class Model:
    pass


@functools.lru_cache(maxsize=None)
def case(name: str) -> Model:
    """diag_ext_model's case `name` (or "directed") with its reason masks and
    records on the loaded state and, where the case has a stream, after it.
    Computed once; callers must not modify it."""
    m = Model()
    m.x = directed() if name == "directed" else resv_scalars() if name == "resv-scalars" else X.CASES[name]()
    x = m.x
    o = oracle.Oracle(x.cfg, x.table)
    m.mask, m.loose = masks(o, x.pods, x.ext)
    m.rec = records(m.mask)
    if hasattr(x, "out"):
        o.place_stream_ext(x.pods, x.ext)
        m.mask_after, _ = masks(o, x.pods, x.ext)
        m.rec_after = records(m.mask_after)
    return m


@functools.lru_cache(maxsize=None)
def resv_scalars():
    """diag_ext_model's resv case with the nodes whose reservation holds extended
    scalars used up in them, the reservation's own Allocatable counted: a
    scalar fits there only on the restored NodeInfo (a matched reservation's
    Allocatable leaves), so the restored terms and xfit_filter's disagree."""
    src = X.resv()
    m = X.Model()
    m.prof, m.pods, m.ext = src.prof, src.pods, src.ext
    t = m.table = copy.deepcopy(src.table)
    held = (t["resv_dev_slot"] >= 0)[:, None] & (t["resv_xalloc"] > 0)
    t["xalloc"][held] = t["xrequested"][held]
    return X._finish(m)


def restored_differs(m: Model) -> int:
    """(pod, node) pairs of a Reservation case whose extended-scalar reasons on
    the restored scalars are not xfit_filter's on the node's own."""
    x = m.x
    o = oracle.Oracle(x.cfg, x.table)
    own = copy.deepcopy(x.table)
    own.cols["resv_xalloc"] = np.zeros_like(own.cols["resv_xalloc"])
    o2 = oracle.Oracle(x.cfg, own)
    return sum(int((xfit_mask(o, x.pods[p], x.ext[p]) != xfit_mask(o2, x.pods[p], x.ext[p])).sum())
               for p in range(len(x.pods)))


CASES = tuple(sorted(X.CASES)) + ("resv-scalars", "directed")

# ------------------------------------------------------------------ the directed table
# 13 nodes, topology keys zone (0), rack (1), hostname (2); every base plugin
# passes everywhere except NodeResourcesFit's cpu on nodes 9 and 12.
#
#   node   0  1  2  3  4  5  6  7  8  9 10 11 12
#   zone   0  0  0  0  0  0  1  -  1  1  1  1  0
#   rack   -  1  1  0  1  0  -  0  0  1  1  1  1
#   extended scalar j is used up on node j (j = 0..7); scalars 0, 3, 5 on node 8; scalar 2 on node 9
#   spread constraint 0 (zone): 5 matching pods on node 0; constraint 1 (rack): 3 on node 3
#   affinity entry 0 (zone): 2 matching pods on node 8; anti-affinity entry 1 (hostname): 1 pod on nodes 1 and 9
D_N = 13
D_ZONE = [0, 0, 0, 0, 0, 0, 1, -1, 1, 1, 1, 1, 0]
D_RACK = [-1, 1, 1, 0, 1, 0, -1, 0, 0, 1, 1, 1, 1]
D_CPU_FULL = (9, 12)
_X = lambda *js: sum(1 << (abi.REASON_FIT_X0 + j) for j in js)
_CPU = 1 << abi.REASON_FIT_CPU
_LABEL, _SKEW = 1 << abi.REASON_PTS_MISSING_LABEL, 1 << abi.REASON_PTS_SKEW
_AFF, _ANTI = 1 << abi.REASON_IPA_AFFINITY, 1 << abi.REASON_IPA_ANTI
# pod: what it asks for -> the expected mask per node, written by hand
D_WANT = {
    # 0: every extended scalar, 1 each: alone on nodes 0-7, three together on node 8, with cpu on node 9
    0: [_X(0), _X(1), _X(2), _X(3), _X(4), _X(5), _X(6), _X(7), _X(0, 3, 5), _CPU | _X(2), 0, 0, _CPU],
    # 1: DoNotSchedule zone (maxSkew 1) then rack (maxSkew 1): zone 0 holds 5 pods against 0, rack 0 holds 3 against 0.
    #    Node 0: zone skew, rack label missing -> the zone constraint comes first: skew.  Node 7: zone label
    #    missing, rack skew -> missing label.  Node 12: cpu failed earlier.
    1: [_SKEW, _SKEW, _SKEW, _SKEW, _SKEW, _SKEW, _LABEL, _LABEL, _SKEW, _CPU, 0, 0, _CPU | _SKEW],
    # 2: no requests, DoNotSchedule rack with maxSkew 100: only the nodes without the label fail, all UU
    2: [_LABEL, 0, 0, 0, 0, 0, _LABEL, 0, 0, 0, 0, 0, 0],
    # 3: required affinity to entry 0 (pods in zone 1 only) and anti-affinity to entry 1 (hosts 1 and 9):
    #    node 1 fails both -> affinity; node 9 fails anti-affinity after cpu
    3: [_AFF, _AFF, _AFF, _AFF, _AFF, _AFF, 0, _AFF, 0, _CPU | _ANTI, 0, 0, _CPU | _AFF],
    # 4: no requests, the required affinity alone: every failing node is UU
    4: [_AFF, _AFF, _AFF, _AFF, _AFF, _AFF, 0, _AFF, 0, 0, 0, 0, _AFF],
}
D_PODS = len(D_WANT)
D_PREEMPTION_HELPS = {0: True, 1: True, 2: False, 3: True, 4: False}


@functools.lru_cache(maxsize=None)
def directed():
    """The directed table as a diag_ext_model-style case (prof, table, pods, ext, cfg, status, rec)."""
    m = X.Model()
    m.prof = with_interpod_affinity(with_topology_spread(with_deviceshare(shipped_profile())))
    t = m.table = synth.make_cluster(synth.ClusterSpec(D_N, seed=X.SEED + 7), m.prof)
    synth.add_devices(t, synth.DevSpec())
    # every base plugin passes: empty nodes without a NodeMetric
    for r in range(abi.NRES):
        t[f"requested{r}"][:] = 0
    t["alloc0"][:], t["alloc1"][:] = 64000, 256 * 2**30
    t["nz_cpu_m"][:] = t["nz_mem"][:] = 0
    t["npods"][:] = 0
    t["alloc_pods"][:] = 110
    t["la_flags"][:] = 0
    t["requested0"][list(D_CPU_FULL)] = 64000
    t["xalloc"][:], t["xrequested"][:] = 10, 0
    for j in range(abi.NXRES):
        t["xrequested"][j, j] = 10
    t["xrequested"][8, [0, 3, 5]] = 10
    t["xrequested"][9, 2] = 10
    t.enable_pts(PtsMeta(keys=3, hostname=0b100, ndom=[2, 2, 0, 0], cons_key=[0, 1], classes=1))
    dom = t["pts_dom"]
    dom[:, 0], dom[:, 1], dom[:, 2] = D_ZONE, D_RACK, np.arange(D_N)
    t["pts_cnt"][0, 0] = 5
    t["pts_cnt"][3, 1] = 3
    both = (dom[:, 0] >= 0) & (dom[:, 1] >= 0)
    t["pts_elig"][:] = np.where(both, 0b11, 0)
    # pod 2's class 1 would need its own bits: one class, eligible = carries every hard key of the pod; pod 2's
    # only hard key is the rack, so its class is 1
    t.pts.classes = 2
    t["pts_elig"][:] |= np.where(dom[:, 1] >= 0, 0b1100, 0).astype(np.uint16)
    t.enable_ipa(IpaMeta(ent_key=[0, 2]))
    t["ipa_cnt"][8, 0] = 2
    t["ipa_cnt"][[1, 9], 1] = 1
    pods = m.pods = synth.make_pods(synth.StreamSpec(D_PODS), m.prof)
    pods["flags"][:] = abi.POD_PROD | abi.POD_HAS_REQ
    pods["req"][:] = 0
    pods["req"][:, abi.RES_CPU], pods["req"][:, abi.RES_MEM] = 1000, 2**30
    pods["nz_cpu_m"][:], pods["nz_mem"][:] = 1000, 2**30
    pods["est_cpu"][:], pods["est_mem"][:] = 1000, 2**30
    for p in (2, 4):
        pods["flags"][p] = abi.POD_PROD
        pods["req"][p] = 0
    x = m.ext = abi.pod_ext_array(D_PODS)
    x["xmask"][0] = 0xFF
    x["xreq"][0, :] = 1
    x["pts_n"][1], x["pts_class"][1] = 2, 0
    x["pts_c"][1, :2], x["pts_fl"][1, :2], x["pts_skew"][1, :2] = [0, 1], abi.PTS_HARD | abi.PTS_SELF, [1, 1]
    x["pts_n"][2], x["pts_class"][2] = 1, 1
    x["pts_c"][2, 0], x["pts_fl"][2, 0], x["pts_skew"][2, 0] = 1, abi.PTS_HARD | abi.PTS_SELF, 100
    x["ipa_aff"][3], x["ipa_anti"][3] = 0b01, 0b10
    x["ipa_aff"][4] = 0b01
    return X._finish(m)
