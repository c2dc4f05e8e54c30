"""The edge tables of exact_model projected onto node snapshots, one case per
node, and the model's evaluation of a snapshot (status bits, score planes,
top-k).  Shared by test_exact_model.py (model against the CPU oracle) and
test_gpu_exact_arith.py (the device against both), so a projection mistake
shows on the CPU before it reaches the GPU.  Imports neither the oracle nor
the engine."""
from __future__ import annotations

import functools

import numpy as np

from koordinator_amd import abi, k8s
from koordinator_amd.config import PLUGIN_NUMA, Profile, shipped_profile, with_upstream
from koordinator_amd.snapshot import NodeTable, pod_array

import exact_model as M

BIG = M.LIMIT - 1


# ------------------------------------------------------------------ the model's eval
def _ints(table, col):
    return [int(v) for v in table[col]]


def model_la_flags(table):
    """(non-prod passes, prod passes, score is zero) per node: load_aware.go:123-254, :278-289."""
    n = table.n
    f = _ints(table, "la_flags")
    used = [_ints(table, f"laf_used_m{r}") for r in range(2)]
    total = [_ints(table, f"laf_total_m{r}") for r in range(2)]
    pused = [_ints(table, f"laf_prod_used_m{r}") for r in range(2)]
    thr = [_ints(table, f"laf_thr{r}") for r in range(2)]
    pthr = [_ints(table, f"laf_prod_thr{r}") for r in range(2)]
    out = []
    for i in range(n):
        if not f[i] & abi.LA_HAS_METRIC or f[i] & abi.LA_FILTER_SKIP:
            np_ok = p_ok = True
        else:
            np_ok = True
            if f[i] & abi.LA_FILTER_USAGE:
                np_ok = all(M.usage_ok(used[r][i], total[r][i], thr[r][i]) for r in range(2))
            p_ok = np_ok
            if f[i] & abi.LA_PROD_MODE:
                p_ok = True
                if f[i] & abi.LA_HAS_PODS_METRIC:
                    p_ok = all(M.usage_ok(pused[r][i], total[r][i], pthr[r][i]) for r in range(2))
        zero = not f[i] & abi.LA_HAS_METRIC or bool(f[i] & abi.LA_SCORE_EXPIRED)
        out.append((np_ok, p_ok, zero))
    return out


def model_eval(cfg, table, pods, k=0):
    """Status bits [p][n], score planes [p][NPLUGINS][n] (plane order
    abi.SCORE_PLUGIN_BITS) and the top-k of the weighted totals over the
    feasible nodes (ties: ascending node), by the model's rules.  Covers Fit,
    LoadAware, NodeResourcesBalancedAllocation and NodeNUMAResource on nodes
    without a topology policy (for a cpuset pod the Filter only)."""
    n, p = table.n, len(pods)
    alloc = [_ints(table, f"alloc{r}") for r in range(abi.NRES)]
    reqd = [_ints(table, f"requested{r}") for r in range(abi.NRES)]
    nzc, nzm = _ints(table, "nz_cpu_m"), _ints(table, "nz_mem")
    apods, npods = _ints(table, "alloc_pods"), _ints(table, "npods")
    laa = [_ints(table, "la_alloc_cpu_m"), _ints(table, "la_alloc_mem")]
    lau = [_ints(table, "la_used_cpu_m"), _ints(table, "la_used_mem")]
    laup = [_ints(table, "la_used_prod_cpu_m"), _ints(table, "la_used_prod_mem")]
    ncls, ncnt = _ints(table, "numa_class"), _ints(table, "numa_alloc_cnt")
    nflags = _ints(table, "numa_flags")
    amp = [float(v) for v in table["numa_amp_cpu"]]
    laf = model_la_flags(table)
    fw = [int(cfg.fit_weight[r]) for r in range(abi.NRES)]
    pw = [int(cfg.plugin_weight[q]) for q in range(abi.NPLUGINS)]
    filt, score = int(cfg.filter_plugins), int(cfg.score_plugins)
    assert not (filt | score) & ~(abi.PLUGIN_FIT | abi.PLUGIN_LOADAWARE | abi.PLUGIN_NUMA | abi.PLUGIN_BALANCED
                                  | abi.PLUGIN_NODE_STATIC), "plugin outside the model"
    status = np.zeros((p, n), np.uint8)
    scores = np.zeros((p, abi.NPLUGINS, n), np.int32)
    topk = np.zeros((p, k), abi.TOPK_DTYPE) if k else None
    scorer = M.most_requested if cfg.numa_most_allocated else M.least_requested
    for j in range(p):
        pod = pods[j]
        fl = int(pod["flags"])
        preq = [int(v) for v in pod["req"]]
        pnzc, pnzm, ec, em = int(pod["nz_cpu_m"]), int(pod["nz_mem"]), int(pod["est_cpu"]), int(pod["est_mem"])
        cpuset = bool(fl & abi.POD_CPUSET) and not fl & abi.POD_NUMA_SKIP
        prod_score = bool(fl & abi.POD_PROD) and bool(cfg.la_score_according_prod_usage)
        keys = []
        for i in range(n):
            a = [alloc[r][i] for r in range(abi.NRES)]
            q = [reqd[r][i] for r in range(abi.NRES)]
            b = 0
            if filt & abi.PLUGIN_FIT and not M.fits_request(npods[i], apods[i], q, a, preq, bool(fl & abi.POD_HAS_REQ),
                                                            bool(fl & abi.POD_REQ_BCPU), bool(fl & abi.POD_REQ_BMEM)):
                b |= abi.ST_FIT_FAIL
            if filt & abi.PLUGIN_LOADAWARE and not fl & abi.POD_DAEMONSET:
                if not (laf[i][1] if fl & abi.POD_PROD else laf[i][0]):
                    b |= abi.ST_LA_FAIL
            if filt & abi.PLUGIN_NUMA:
                assert nflags[i] >> abi.NODE_NUMA_POLICY_SHIFT == 0 and nflags[i] & 3 == 0, "node outside the model"
                assert not fl & abi.POD_NUMA_ERROR and abi.numa_policy(3) & int(pod["numa_policy"]) == 0
                ok = M.amplified_cpu_fits(preq[0], cpuset, amp[i], ncnt[i], ncls[i] >= 0, q[0], a[0])
                if cpuset and ncls[i] < 0:
                    ok = False
                if not ok:
                    b |= abi.ST_NUMA_FAIL
            status[j, i] = b
            s = [0, 0, 0, 0]
            if score & abi.PLUGIN_FIT:
                s[0] = M.fit_score(nzc[i], nzm[i], q, a, pnzc, pnzm, preq, fw)
            if score & abi.PLUGIN_LOADAWARE:
                u = laup if prod_score else lau
                s[1] = M.loadaware_score(u[0][i], u[1][i], laa[0][i], laa[1][i], ec, em, int(cfg.la_weight_cpu),
                                         int(cfg.la_weight_mem), laf[i][2])
            if score & abi.PLUGIN_NUMA and not fl & (abi.POD_NUMA_SKIP | abi.POD_NUMA_ERROR) and ncls[i] >= 0:
                assert not cpuset, "cpuset Score is outside the model"
                rc = q[0]
                if preq[0] != 0 and amp[i] > 1:
                    rc = rc - ncnt[i] * 1000 + M.amplify(ncnt[i] * 1000, amp[i])
                terms = []
                if cfg.numa_weight_cpu:
                    terms.append((rc + preq[0], a[0], int(cfg.numa_weight_cpu)))
                if cfg.numa_weight_mem:
                    terms.append((q[1] + preq[1], a[1], int(cfg.numa_weight_mem)))
                s[2] = M.weighted_average(terms, scorer)
            if score & abi.PLUGIN_BALANCED:
                s[3] = M.balanced_score(q[0] + preq[0], a[0], q[1] + preq[1], a[1])
            for w in range(4):
                scores[j, w, i] = s[w]
            if k and b == 0:
                keys.append((-sum(pw[w] * s[w] for w in range(4)), i))
        if k:
            keys.sort()
            for t in range(k):
                topk[j, t] = (keys[t][1], -keys[t][0]) if t < len(keys) else (-1, 0)
    return {"status": status, "scores": scores, "topk": topk}


def first_diff(got, want):
    """Index tuple of the first differing element of two arrays, or None."""
    if np.array_equal(got, want):
        return None
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.dtype.names:
        bad = np.zeros(got.shape, bool)
        for f in got.dtype.names:
            bad |= got[f] != want[f]
    else:
        bad = got != want
    return tuple(int(x) for x in np.argwhere(bad)[0])


# ------------------------------------------------------------------ cluster pieces
def base_table(n, cls=False):
    """n roomy nodes: every Filter passes for a modest pod until a case column is written."""
    t = NodeTable.empty(n)
    t["alloc_pods"][:] = 110
    t["la_flags"][:] = abi.LA_HAS_METRIC
    if cls:
        from koordinator_amd.numa import ClassTable, reference_test_topology
        topo = reference_test_topology(2, 1, 8, 2)
        ct = ClassTable()
        t["numa_class"][:] = ct.add(topo)
        t.numa_classes = ct.records()
        free = topo.mask(list(topo.cpu_of))
        for w in range(abi.NUMA_WORDS):
            t[f"numa_free{w}"][:] = free[w]
    return t


def _pair(n, seed):
    """A seeded pairing of one case column with another (the tables themselves hold no randomness)."""
    return np.random.default_rng(seed).permutation(n)


@functools.lru_cache(maxsize=None)
def _qe(most=False):
    c = M.loadable(M.quotient_edges(most))
    return np.array([x[0] for x in c], np.int64), np.array([x[1] for x in c], np.int64)


def lrs_profile():
    prof = shipped_profile()
    prof.loadaware.score_according_prod_usage = True
    return prof


def lrs_pods():
    """A non-prod pod with zero quantities, a prod pod with zero quantities (its
    LoadAware Score reads the prod usage columns) and a pod adding 1 to every
    quantity (each case moves by one)."""
    p = pod_array(3)
    p["flags"][1] = abi.POD_PROD
    p["nz_cpu_m"][2] = p["nz_mem"][2] = p["est_cpu"][2] = p["est_mem"][2] = 1
    return p


def lrs_cluster(alias: bool):
    """The quotient-edge table (the cases the loader admits) on the Fit cpu column, a second pairing of it on
    the memory column, two more on LoadAware's usage columns (non-prod and
    prod).  alias: LoadAware's allocatable equals Allocatable (the loader reads
    them once); else LoadAware's caps are a further pairing of the table."""
    req, cap = _qe()
    n = len(req)
    t = base_table(n)
    pm = _pair(n, 1)
    t["nz_cpu_m"][:], t["alloc0"][:] = req, cap
    t["nz_mem"][:], t["alloc1"][:] = req[pm], cap[pm]
    if alias:
        t["la_alloc_cpu_m"][:], t["la_alloc_mem"][:] = t["alloc0"], t["alloc1"]
        t["la_used_cpu_m"][:], t["la_used_mem"][:] = req, req[pm]
        # prod usage: the same caps with the boundary of the neighbouring quotient
        t["la_used_prod_cpu_m"][:] = np.maximum(req - cap // 100, 0)
        t["la_used_prod_mem"][:] = np.maximum(req[pm] - cap[pm] // 100, 0)
    else:
        pc, pq = _pair(n, 2), _pair(n, 3)
        t["la_alloc_cpu_m"][:], t["la_used_cpu_m"][:] = cap[pc], req[pc]
        t["la_alloc_mem"][:], t["la_used_mem"][:] = cap[pq], req[pq]
        t["la_used_prod_cpu_m"][:] = np.maximum(req[pc] - cap[pc] // 100, 0)
        t["la_used_prod_mem"][:] = np.maximum(req[pq] - 1, 0)
    return t


def lrs_label(alias: bool):
    req, cap = _qe()
    pm = _pair(len(req), 1)
    return lambda i: f"fit cpu (req, cap) = ({req[i]}, {cap[i]}), fit memory ({req[pm[i]]}, {cap[pm[i]]})"


def mrs_profile():
    prof = Profile(filters=(PLUGIN_NUMA,), scores={PLUGIN_NUMA: 1})
    prof.numa.scoring_type = "MostAllocated"
    prof.numa.resources = {k8s.CPU: 1, k8s.MEMORY: 3}
    return prof


def mrs_cluster():
    """mostRequestedScore: the most-requested edge table of the caps >= 2^31 on
    memory, the small caps' table on cpu (Requested columns; NodeNUMAResource
    Score of a pod without a cpuset on nodes with a CPU topology)."""
    big = [c for c in M.CAPS if c >= 1 << 31]
    small = [c for c in M.CAPS if c < 1 << 31]
    cm = [x for x in M.loadable(M.quotient_edges(True, big)) if x[1] != 0]
    cc = M.loadable(M.quotient_edges(True, small))
    n = len(cm)
    t = base_table(n, cls=True)
    t["requested1"][:] = [x[0] for x in cm]
    t["alloc1"][:] = [x[1] for x in cm]
    idx = np.arange(n) % len(cc)
    t["requested0"][:] = np.array([x[0] for x in cc], np.int64)[idx]
    t["alloc0"][:] = np.array([x[1] for x in cc], np.int64)[idx]
    p = pod_array(2)
    p["req"][1, abi.RES_MEM] = 1
    p["flags"][1] = abi.POD_HAS_REQ
    return t, p, (lambda i: f"memory (req, cap) = {cm[i]}, cpu {cc[idx[i]]}")


AVERAGE_ENGINES = [
    # (Fit weights cpu, memory[, ephemeral, batch-cpu, batch-memory]), LoadAware weights
    ((1, 1), (1, 1)),        # LoadAware (1, 1): the power-of-two shift
    ((1, 2), (3, 4)),
    ((99, 1), (1, 1)),
    ((100, 100, 100, 100, 100), (3, 4)),   # weight sum 500, the pod requests both batch resources
    ((7, 13), (1, 1)),
]


def average_profile(fit_w, la_w):
    prof = shipped_profile()
    names = [k8s.CPU, k8s.MEMORY, k8s.EPHEMERAL, k8s.BATCH_CPU, k8s.BATCH_MEMORY]
    prof.fit.resources = {names[r]: w for r, w in enumerate(fit_w)}
    prof.loadaware.resource_weights = {k8s.CPU: la_w[0], k8s.MEMORY: la_w[1]}
    return prof


def average_cluster():
    """The 101 x 101 grid: caps of 100, so the cpu / memory scores of Fit and of
    LoadAware are 100 - req; the other three Fit resources sweep 0..100 on
    strides coprime with 101."""
    g = M.average_grid()
    n = len(g)
    t = base_table(n)
    sc = np.array([x[0] for x in g], np.int64)
    sm = np.array([x[1] for x in g], np.int64)
    for r in range(abi.NRES):
        t[f"alloc{r}"][:] = 100
    t["la_alloc_cpu_m"][:] = t["la_alloc_mem"][:] = 100
    t["nz_cpu_m"][:], t["nz_mem"][:] = 100 - sc, 100 - sm
    t["la_used_cpu_m"][:], t["la_used_mem"][:] = 100 - sm, 100 - sc
    i = np.arange(n, dtype=np.int64)
    t["requested2"][:], t["requested3"][:], t["requested4"][:] = (i * 7) % 101, (i * 13) % 101, (i * 29) % 101
    p = pod_array(2)
    p["flags"][1] = abi.POD_HAS_REQ | abi.POD_REQ_BCPU | abi.POD_REQ_BMEM
    p["req"][1, abi.RES_BCPU] = p["req"][1, abi.RES_BMEM] = 1
    return t, p, (lambda q: f"(s_cpu, s_mem) = {g[q]}")


def usage_profile():
    prof = shipped_profile()
    prof.loadaware.prod_usage_thresholds = {k8s.CPU: 40, k8s.MEMORY: 90}
    return prof


def usage_pods():
    p = pod_array(3)
    p["flags"][0] = abi.POD_PROD
    p["flags"][2] = abi.POD_DAEMONSET
    return p


def usage_cluster():
    """Every rounding edge twice, on the threshold (fails) and one under it
    (passes): even nodes carry it on cpu, odd nodes on memory, the other
    resource's threshold 0 (skipped); the prod columns carry a second pairing
    the same way.  -> (table, cases, node -> (case, resource, prod case))."""
    cases = M.usage_edges()
    m = len(cases)
    n = 2 * m
    t = base_table(n)
    t["la_flags"][:] = abi.LA_HAS_METRIC | abi.LA_FILTER_USAGE | abi.LA_PROD_MODE | abi.LA_HAS_PODS_METRIC
    group = {}
    for c, (_, total) in enumerate(cases):
        group.setdefault(total, []).append(c)
    where = []
    for i in range(n):
        c, var = divmod(i, 2)
        r = c & 1
        used, total = cases[c]
        # one total column serves both usages: the prod case is another case of the same total
        g = group[total]
        pc = g[(g.index(c) + 7) % len(g)]
        pused = cases[pc][0]
        t[f"laf_used_m{r}"][i], t[f"laf_total_m{r}"][i] = used, total
        t[f"laf_thr{r}"][i] = M.usage_percent(used, total) + var
        t[f"laf_prod_used_m{r}"][i] = pused
        t[f"laf_prod_thr{r}"][i] = M.usage_percent(pused, total) + (1 - var)
        where.append((c, r, pc))
    return t, cases, where


def usage_update(t):
    """Rows 0, 3, 6, ... with every non-zero threshold moved by one toward the other verdict."""
    idx = np.arange(0, t.n, 3, dtype=np.int32)
    rows = t.rows(idx)
    for r in range(2):
        for col, used in ((f"laf_thr{r}", f"laf_used_m{r}"), (f"laf_prod_thr{r}", f"laf_prod_used_m{r}")):
            for q in range(len(idx)):
                thr, total = int(rows[col][q]), int(rows[f"laf_total_m{r}"][q])
                if thr == 0 or total == 0:
                    continue
                u = M.usage_percent(int(rows[used][q]), total)
                rows[col][q] = thr + 1 if u >= thr else thr - 1
    t2 = t.copy()
    for c in rows.cols:
        t2[c][idx] = rows[c]
    return idx, rows, t2


FILTER_POD_REQ = (7, (1 << 33) + 5, 1000, 333, (1 << 20) + 1)


def filter_pods():
    """A pod requesting all five resources, a pod with requests but none of cpu
    / memory / ephemeral storage (the over-commit bits decide), a pod without
    requests (only the pod count)."""
    p = pod_array(3)
    p["req"][0] = FILTER_POD_REQ
    p["flags"][0] = abi.POD_HAS_REQ | abi.POD_REQ_BCPU | abi.POD_REQ_BMEM
    p["req"][1, abi.RES_BCPU] = 1
    p["flags"][1] = abi.POD_HAS_REQ | abi.POD_REQ_BCPU
    return p


def filter_cluster():
    """Per resource and Allocatable (2^45 - 1 and small ones): Requested such that
    the free amount is one under, on and one over the first pod's request; then
    Requested on and one over Allocatable (the zero-request path); then the pod
    count one under and on its limit."""
    rows = []   # (resource, alloc, requested) with the others roomy; resource -1: pod count (npods, alloc_pods)
    for r in range(abi.NRES):
        for a in (BIG, FILTER_POD_REQ[r] + 3, 1 << 40):
            for d in (-1, 0, 1):
                rows.append((r, a, a - FILTER_POD_REQ[r] + d))
        for a in (BIG - 1, 10, 0):
            for d in (-1, 0, 1):
                if a + d >= 0:
                    rows.append((r, a, a + d))
    for a in (1, 110, 2**31 - 1):
        rows += [(-1, a - 1, a), (-1, a, a), (-1, 0, a)]
    n = len(rows)
    t = base_table(n)
    for r in range(abi.NRES):
        t[f"alloc{r}"][:] = 1 << 42
    for i, (r, a, q) in enumerate(rows):
        if r < 0:
            t["npods"][i], t["alloc_pods"][i] = a, q
        else:
            t[f"alloc{r}"][i], t[f"requested{r}"][i] = a, q
    return t, rows


def balanced_profile():
    return with_upstream(shipped_profile(), balanced_weight=1)


def balanced_cluster():
    c = M.balanced_edges()
    t = base_table(len(c))
    t["requested0"][:] = [x[0] for x in c]
    t["alloc0"][:] = [x[1] for x in c]
    t["requested1"][:] = [x[2] for x in c]
    t["alloc1"][:] = [x[3] for x in c]
    t["la_alloc_cpu_m"][:], t["la_alloc_mem"][:] = t["alloc0"], t["alloc1"]
    p = pod_array(2)
    p["req"][1, abi.RES_CPU] = p["req"][1, abi.RES_MEM] = 1
    p["flags"][1] = abi.POD_HAS_REQ
    return t, p, c


AMP_POD_CPU = (1000, 50, 3000, 7)


def amp_pods():
    """Cpuset pods (their request is amplified) and the last one again without a cpuset."""
    p = pod_array(len(AMP_POD_CPU) + 1)
    for j, cpu in enumerate(AMP_POD_CPU + (AMP_POD_CPU[-1],)):
        p["req"][j, abi.RES_CPU] = p["nz_cpu_m"][j] = cpu
        p["flags"][j] = abi.POD_HAS_REQ
        if j < len(AMP_POD_CPU):
            p["flags"][j] |= abi.POD_CPUSET
            p["numa_cpus"][j] = max(1, cpu // 1000)
            p["numa_policy"][j] = abi.numa_policy(0, abi.CPUBIND_FULL_PCPUS, 0)
    return p


def amp_cluster():
    """Per (ratio, CPUs held by cpusets, other Requested, pod, slack): Allocatable
    = the amplified Requested + the pod's amplified request + slack."""
    c = M.amplify_edges(AMP_POD_CPU)
    t = base_table(len(c), cls=True)
    for i, (ratio, cnt, other, cpu, d) in enumerate(c):
        held = cnt * 1000
        t["numa_amp_cpu"][i] = ratio
        t["numa_alloc_cnt"][i] = cnt
        t["requested0"][i] = held + other
        t["alloc0"][i] = other + M.amplify(held, ratio) + M.amplify(cpu, ratio) + d
    t["alloc1"][:] = 1 << 40
    return t, c


# ------------------------------------------------------------------ the stream
STREAM_CLASSES = [(1, 1), (7, (1 << 20) + 1), (333, (1 << 33) + 5), (1000, (1 << 36) - 1), (17, (1 << 41) + 9),
                  (4001, 123456789)]


def stream_pods(n=1500, resv=False):
    """Six classes of awkward sizes; resv: every fourth pod matches the cluster's reservations (owner group 0)."""
    p = pod_array(n)
    if resv:
        p["resv_match"][::4] = 1
    for j in range(n):
        cpu, mem = STREAM_CLASSES[(j * 5 + j // 7) % len(STREAM_CLASSES)]
        p["req"][j, abi.RES_CPU], p["req"][j, abi.RES_MEM] = cpu, mem
        p["nz_cpu_m"][j], p["nz_mem"][j] = cpu, mem
        p["est_cpu"][j], p["est_mem"][j] = (cpu * 85 + 99) // 100, (mem * 70 + 99) // 100
        p["flags"][j] = abi.POD_HAS_REQ | (abi.POD_PROD if j % 3 == 0 else 0)
    return p


def stream_cluster(numa=False, resv=False):
    """Nodes whose cpu / memory Allocatable come from the edge tables' caps
    (memory up to 2^45 - 1) with Requested, NonZeroRequested and LoadAware usage
    on the quotient boundaries, so that the 1500 placements walk the scores
    across them."""
    caps_c = [c for c in M.CAPS if 32000 <= c < 1 << 38]
    caps_m = [c for c in M.CAPS if c >= 1 << 38]
    n = 211
    t = base_table(n, cls=numa)
    i = np.arange(n, dtype=np.int64)
    ac = np.array(caps_c, np.int64)[i % len(caps_c)]
    am = np.array(caps_m, np.int64)[(i // 3) % len(caps_m)]
    qc, qm = (i * 37) % 16, (i * 53) % 18
    rc = ac - (-((-(100 - qc) * ac) // 100))      # on the boundary: score 100 - qc exactly
    rm = np.maximum(am - (-((-(100 - qm) * am) // 100)) + (i % 3 - 1), 0)     # ... one under, on, one over
    t["alloc0"][:], t["alloc1"][:] = ac, am
    t["requested0"][:], t["requested1"][:] = rc, rm
    t["nz_cpu_m"][:], t["nz_mem"][:] = rc, rm
    t["la_alloc_cpu_m"][:], t["la_alloc_mem"][:] = ac, am
    t["la_used_cpu_m"][:], t["la_used_mem"][:] = rc // 2, rm // 3
    t["la_used_prod_cpu_m"][:], t["la_used_prod_mem"][:] = rc // 4, rm // 5
    t["npods"][:] = (i % 40).astype(np.int32)
    t["la_flags"][:] = abi.LA_HAS_METRIC | abi.LA_FILTER_USAGE
    t["laf_total_m0"][:], t["laf_used_m0"][:] = 200, 129 + (i % 3)     # 64.5 % (rounds up: 65 fails), 65 %, 65.5 %
    t["laf_thr0"][:] = np.where(i % 10 == 0, 65, 66)
    if resv:
        t["resv_flags"][::5] = abi.RESV_PRESENT | abi.RESV_KEY_CPU | abi.RESV_KEY_MEM
        t["resv_alloc0"][::5], t["resv_alloc1"][::5] = 8000, (1 << 41) + 9
        t["resv_nz0"][::5], t["resv_nz1"][::5] = 8000, (1 << 41) + 9
        t["requested0"][::5] += 8000
        t["requested1"][::5] += (1 << 41) + 9
        t["nz_cpu_m"][::5] += 8000
        t["nz_mem"][::5] += (1 << 41) + 9
        t["npods"][::5] += 1
    return t


def stream_profile(numa=False, resv=False):
    prof = shipped_profile(numa=numa or resv, reservation=resv)
    prof.batch_pods = 32
    return prof


def check_stream_not_vacuous(placed):
    """On the oracle's placements: >= 90 % placed, >= 100 distinct nodes, at
    least half on a node already chosen earlier in the stream."""
    ok = placed[placed >= 0]
    seen, again = set(), 0
    for v in ok.tolist():
        again += v in seen
        seen.add(v)
    assert len(ok) >= 0.9 * len(placed), (len(ok), len(placed))
    assert len(seen) >= 100, len(seen)
    assert again >= 0.5 * len(ok), (again, len(ok))
    return len(ok), len(seen), again
