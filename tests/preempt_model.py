"""The preemption dry run, computed with the CPU oracle alone: a plain-Python
restatement of elasticquota's SelectVictimsOnNode (preempt.go:111-215) per
(preemptor, node) and of the candidate pick, as include/koordhip.h states them.

Every "does the preemptor fit this hypothetical row" is one status byte of
oracle.Oracle(cfg, table).eval(status=True) on a table whose rows are the
hypothetical states: the snapshot's rows with requested*, nz_* and npods moved
by the removed / re-added pods.  One preemptor's walk advances all nodes in
lock step, so a step of the walk is one oracle call over n hypothetical rows.

Also the generators of the inputs the GPU tests run: clusters tightened so
that the preemptors are unschedulable, 0-12 assigned pods per node with tied
priorities, duplicate start times, three quotas, some non-preemptible pods and
three PDBs with budgets 0 and 1.
"""
import functools
from dataclasses import dataclass

import numpy as np

import oracle
from koordinator_amd import abi, k8s, synth
from koordinator_amd.config import shipped_profile, to_c_config, with_upstream
from koordinator_amd.snapshot import NodeTable

SEED = synth.SEED
NRES = abi.NRES
ROW_COLS = [f"requested{r}" for r in range(NRES)] + ["nz_cpu_m", "nz_mem", "npods"]


# --------------------------------------------------------------------- model
def node_lists(assigned: np.ndarray, n: int):
    """Per node the indices of its assigned pods in list order: priority
    descending, start_time ascending, input index ascending."""
    lists = [[] for _ in range(n)]
    order = sorted(range(len(assigned)), key=lambda j: (-int(assigned["priority"][j]), int(assigned["start_time"][j]), j))
    for j in order:
        lists[int(assigned["node"][j])].append(j)
    return lists


class _Rows:
    """The hypothetical rows of all nodes for one preemptor."""

    def __init__(self, cfg, table: NodeTable, pod: np.ndarray):
        self.cfg, self.table, self.pod = cfg, table, np.ascontiguousarray(pod.reshape(1))
        self.cols = {c: table[c].copy() for c in ROW_COLS}

    def move(self, i: int, pod, sign: int):
        for r in range(NRES):
            self.cols[f"requested{r}"][i] += sign * int(pod["req"][r])
        self.cols["nz_cpu_m"][i] += sign * int(pod["nz_cpu_m"])
        self.cols["nz_mem"][i] += sign * int(pod["nz_mem"])
        self.cols["npods"][i] += sign

    def status(self) -> np.ndarray:
        t = self.table.copy()
        for c in ROW_COLS:
            t[c][:] = self.cols[c]
        return oracle.Oracle(self.cfg, t).eval(self.pod, status=True, scores=False)["status"][0].copy()


def _verdict(status, nv=0, npdb=0, top=0, sump=0, es=0):
    v = np.zeros((), abi.PREEMPT_NODE_DTYPE)
    v["status"], v["n_victims"], v["n_pdb_violations"], v["top_priority"] = status, nv, npdb, top
    v["sum_priority"], v["earliest_start"] = sump, es
    return v


class Rule:
    """What a mode of the dry run adds to the walk, for one preemptor: made by
    select_victims as rule(cfg, table, pre, rows), where `table` holds the rows
    the walk starts from and `rows` the hypothetical ones it moves.  This one is
    the base dry run; preempt_numa_model and preempt_resv_model define theirs."""

    def __init__(self, cfg, table, pre, rows):
        pass

    def unresolvable(self, i: int) -> bool:
        """Node i's start row is UNRESOLVABLE although no static filter fails."""
        return False

    def fits(self, status: int, i: int) -> bool:
        """The preemptor fits node i's hypothetical row, whose oracle status is `status`."""
        return status == 0

    def moved(self, i: int, a, sign: int):
        """Listed pod `a` left (-1) or rejoined (+1) node i's row: what else moves with it."""


def select_victims(cfg, table: NodeTable, assigned: np.ndarray, pdb_allowed, pre: np.ndarray, lists=None, rule=Rule):
    """One preemptor on every node: (verdicts [n] PREEMPT_NODE_DTYPE, victims
    per node as lists of table indices in append order, potential victims per
    node; [] where the start row is UNRESOLVABLE)."""
    n = table.n
    lists = lists if lists is not None else node_lists(assigned, n)
    rows = _Rows(cfg, table, pre["pod"])
    mode = rule(cfg, table, pre, rows)
    verdicts = np.zeros(n, abi.PREEMPT_NODE_DTYPE)
    P_prio, P_quota = int(pre["priority"]), int(pre["quota"])
    st0 = rows.status()
    used = [[int(x) for x in pre["q_used"]] for _ in range(n)]
    done = np.zeros(n, bool)
    pot = [[] for _ in range(n)]
    order = [[] for _ in range(n)]
    nviol = [0] * n

    def take(i, j, sign):
        a = assigned[j]
        rows.move(i, a["pod"], sign)
        mode.moved(i, a, sign)
        if int(a["flags"]) & abi.ASG_IN_QUOTA:
            for d in range(abi.PREEMPT_QRES):
                used[i][d] = used[i][d] + int(a["qreq"][d]) if sign > 0 else max(0, used[i][d] - int(a["qreq"][d]))

    for i in range(n):
        unresolvable = mode.unresolvable(i)
        if (st0[i] & abi.ST_STATIC_FAIL) or unresolvable:
            verdicts[i] = _verdict(abi.PREEMPT_UNRESOLVABLE)
            done[i] = True
            continue
        allowed = [int(x) for x in pdb_allowed]
        viol, rest = [], []
        for j in lists[i]:
            a = assigned[j]
            if (int(a["flags"]) & abi.ASG_NONPREEMPTIBLE) or not int(a["priority"]) < P_prio or int(a["quota"]) != P_quota:
                continue
            pot[i].append(j)
            take(i, j, -1)
            bad = False
            for b in range(len(allowed)):
                if (int(a["pdb_mask"]) >> b) & 1:
                    allowed[b] -= 1
                    bad = bad or allowed[b] < 0
            (viol if bad else rest).append(j)
        if not pot[i]:
            verdicts[i] = _verdict(abi.PREEMPT_NO_VICTIMS)
            done[i] = True
        order[i], nviol[i] = viol + rest, len(viol)
    st1 = rows.status()
    for i in range(n):
        if not done[i] and not mode.fits(int(st1[i]), i):
            verdicts[i] = _verdict(abi.PREEMPT_UNFIT)
            done[i] = True
    victims = [[] for _ in range(n)]
    npdb = [0] * n
    step = 0
    while True:
        live = [i for i in range(n) if not done[i] and step < len(order[i])]
        if not live:
            break
        for i in live:
            take(i, order[i][step], +1)
        st = rows.status()
        for i in live:
            j = order[i][step]
            fits = mode.fits(int(st[i]), i)
            if not fits:
                take(i, j, -1)
                victims[i].append(j)
                if step < nviol[i]:
                    npdb[i] += 1
            over = P_quota >= 0 and any((int(pre["q_mask"]) >> d) & 1 and
                                        used[i][d] + int(pre["q_req"][d]) > int(pre["q_runtime"][d])
                                        for d in range(abi.PREEMPT_QRES))
            if over:
                if not fits:  # NodeInfo.RemovePod of a pod that is gone: the evaluator drops the node
                    verdicts[i] = _verdict(abi.PREEMPT_ERROR)
                    victims[i] = []
                    done[i] = True
                    continue
                take(i, j, -1)
                victims[i].append(j)
        step += 1
    for i in range(n):
        if done[i]:
            continue
        v = victims[i]
        if not v:
            verdicts[i] = _verdict(abi.PREEMPT_CANDIDATE)
            continue
        pr = [int(assigned["priority"][j]) for j in v]
        top = max(pr)
        es = min(int(assigned["start_time"][j]) for j in v if int(assigned["priority"][j]) == top)
        verdicts[i] = _verdict(abi.PREEMPT_CANDIDATE, len(v), npdb[i], pr[0], sum(p + (1 << 31) for p in pr), es)
    return verdicts, victims, pot


def pick_key(v, node: int):
    """The pick's key of a CANDIDATE verdict: the smallest wins."""
    return (int(v["n_victims"]) != 0, int(v["n_pdb_violations"]), int(v["top_priority"]), int(v["sum_priority"]),
            int(v["n_victims"]), -int(v["earliest_start"]), node)


def pick(verdicts: np.ndarray):
    """koordhip_preempt_result of one preemptor's verdicts."""
    res = np.zeros((), abi.PREEMPT_RESULT_DTYPE)
    res["node"] = -1
    for s in range(abi.PREEMPT_STATUSES):
        res["count"][s] = int((verdicts["status"] == s).sum())
    cand = [i for i in range(len(verdicts)) if verdicts["status"][i] == abi.PREEMPT_CANDIDATE]
    if cand:
        best = min(cand, key=lambda i: pick_key(verdicts[i], i))
        res["node"] = best
        res["best"] = verdicts[best]
    return res


def dry_run(cfg, table, assigned, pdb_allowed, pres, rule=Rule):
    """All preemptors: (results [p], verdicts [p][n], chosen victims per preemptor, victims / potential per (p, node))."""
    lists = node_lists(assigned, table.n)
    res = np.zeros(len(pres), abi.PREEMPT_RESULT_DTYPE)
    ver = np.zeros((len(pres), table.n), abi.PREEMPT_NODE_DTYPE)
    chosen, allv, allp = [], [], []
    for p in range(len(pres)):
        v, vic, pot = select_victims(cfg, table, assigned, pdb_allowed, pres[p], lists, rule)
        ver[p] = v
        res[p] = pick(v)
        chosen.append(vic[int(res[p]["node"])] if res[p]["node"] >= 0 else [])
        allv.append(vic)
        allp.append(pot)
    return res, ver, chosen, allv, allp


def victims_array(chosen, max_victims: int) -> np.ndarray:
    out = np.full((len(chosen), max_victims), -1, np.int32)
    for p, v in enumerate(chosen):
        k = min(len(v), max_victims)
        out[p, :k] = v[:k]
    return out


# ---------------------------------------------------------------- generators
# name -> (profile kind, n, n_pre, seed, a node holding exactly 128 pods)
CASES = {
    "one": ("base", 1, 1, SEED + 1, False),
    "wave": ("la", 63, 3, SEED + 1, False),
    "tiles": ("base", 257, 33, SEED + 2, False),
    "la257": ("la", 257, 3, SEED + 3, False),
    "full": ("base", 63, 3, SEED + 5, True),
    "static": ("static", 130, 3, SEED + 6, False),
}
FULL_NODE = 5
N_PDB = 3
PDB_ALLOWED = (0, 1, 1)
PRIORITIES = [0, 100, 100, 1000, 5000]
PRE_PRIORITIES = [100, 1000, 5000, 9000]
PRE_CPU = [3000, 4000, 6000, 8000]
STARTS = [1_700_000_000_000_000_000 + k * 3_600_000_000_000 for k in range(6)]


def profile_of(kind: str):
    prof = shipped_profile()
    if kind == "la":  # usage thresholds that fail on many nodes (usage is U[0, 0.8] of the allocatable)
        prof.loadaware.usage_thresholds = {k8s.CPU: 45, k8s.MEMORY: 60}
    if kind == "static":
        prof = with_upstream(prof)
    return prof


@dataclass
class Inputs:
    prof: object
    table: NodeTable
    assigned: np.ndarray
    pdb_allowed: tuple
    pres: np.ndarray


def inputs(kind, n, n_pre, seed, full, base_per: int = 0) -> Inputs:
    """base_per: assigned pods every node holds besides its 0-12 (the timing runs' ~30 per node)."""
    prof = profile_of(kind)
    table = synth.make_cluster(synth.ClusterSpec(n, seed=seed), prof)
    per = (synth.splitmix64(seed, n, 700) % np.uint64(13)).astype(np.int64) + base_per
    if full:
        per[FULL_NODE] = abi.PREEMPT_NODE_PODS
        table["alloc_pods"][FULL_NODE] = 400
        table["alloc0"][FULL_NODE] = table["la_alloc_cpu_m"][FULL_NODE] = 128000
        table["alloc1"][FULL_NODE] = table["la_alloc_mem"][FULL_NODE] = 1024 * synth.GI
    m = int(per.sum())
    a = np.zeros(m, abi.ASSIGNED_DTYPE)
    a["pod"] = synth.make_pods(synth.StreamSpec(m, be_frac=0.2, seed=seed + 3), prof)
    node = np.repeat(np.arange(n), per)
    node = node[np.argsort(synth.splitmix64(seed, m, 701), kind="stable")]  # the input order is not the nodes'
    a["node"] = node
    if full:  # small pods, so that the node's 128 fit its allocatable
        on = node == FULL_NODE
        pod = a["pod"]
        pod["req"][on] = pod["req"][on] // 4
        for f in ("nz_cpu_m", "nz_mem", "est_cpu", "est_mem"):
            pod[f][on] = pod[f][on] // 4
        a["pod"] = pod
    a["priority"] = synth.choice(seed, m, 702, PRIORITIES)
    a["start_time"] = synth.choice(seed, m, 703, STARTS)
    a["quota"] = (synth.splitmix64(seed, m, 704) % np.uint64(3)).astype(np.int32)
    fl = np.where(synth.uniform(seed, m, 705) < 0.1, abi.ASG_NONPREEMPTIBLE, 0)
    fl |= np.where(synth.uniform(seed, m, 706) < 0.85, abi.ASG_IN_QUOTA, 0)
    a["flags"] = fl
    mask = np.zeros(m, np.uint32)
    for b in range(N_PDB):
        mask |= np.where(synth.uniform(seed, m, 710 + b) < 0.2, 1 << b, 0).astype(np.uint32)
    a["pdb_mask"] = mask
    req = a["pod"]["req"]
    a["qreq"][:, 0] = req[:, abi.RES_CPU] + req[:, abi.RES_BCPU]
    a["qreq"][:, 1] = req[:, abi.RES_MEM] + req[:, abi.RES_BMEM]
    # the rows: at most 2.5 CPUs free, and every assigned pod is part of its node's row
    free = (synth.uniform(seed, n, 901) * 2500).astype(np.int64)
    table["requested0"][:] = np.maximum(table["requested0"], table["alloc0"] - free)
    for r in range(NRES):
        s = np.bincount(node, weights=req[:, r].astype(np.float64), minlength=n).astype(np.int64)
        table[f"requested{r}"][:] = np.maximum(table[f"requested{r}"], s)
    for f in ("nz_cpu_m", "nz_mem"):
        s = np.bincount(node, weights=a["pod"][f].astype(np.float64), minlength=n).astype(np.int64)
        table[f][:] = np.maximum(table[f], s)
    table["npods"][:] = table["npods"] + per.astype(np.int32)
    # the preemptors: LS pods of 3 CPUs and more, unschedulable on every node as the rows stand
    pres = np.zeros(n_pre, abi.PREEMPTOR_DTYPE)
    pod = synth.make_pods(synth.StreamSpec(n_pre, be_frac=0.0, seed=seed + 5), prof)
    cpu = synth.choice(seed, n_pre, 720, PRE_CPU).astype(np.int64)
    pod["req"][:, abi.RES_CPU] = cpu
    pod["nz_cpu_m"] = cpu
    if kind == "static":
        synth.add_static(table, pod, synth.StaticSpec(), prof, seed)
    pres["pod"] = pod
    pres["priority"] = synth.choice(seed, n_pre, 721, PRE_PRIORITIES)
    pres["quota"] = (synth.splitmix64(seed, n_pre, 722) % np.uint64(3)).astype(np.int32)
    pres["q_mask"] = 3
    inq = (a["flags"] & abi.ASG_IN_QUOTA) != 0
    used = [a["qreq"][inq & (a["quota"] == k)].sum(axis=0) for k in range(3)]   # what the quota's pods hold
    for p in range(n_pre):
        pres["q_used"][p] = used[int(pres["quota"][p])]
        pres["q_req"][p, 0] = pod["req"][p, abi.RES_CPU]
        pres["q_req"][p, 1] = pod["req"][p, abi.RES_MEM]
        # the quota's runtime: ample, or short by the preemptor's CPUs + 2 / by 1.5 CPUs, so that the quota asks
        # for more room than the node does (victims by quota alone) or for room the node lacks (ERROR nodes)
        short = (1 << 40, -int(cpu[p]) - 2000, 1 << 40, -1500)[p % 4]
        pres["q_runtime"][p] = pres["q_used"][p] + pres["q_req"][p]
        pres["q_runtime"][p, 0] += short
        pres["q_runtime"][p, 1] += 1 << 40
    if n_pre >= 3:
        pres["quota"][2] = -1  # postFilterState.skip
    return Inputs(prof, table, a, PDB_ALLOWED, pres)


class Model:
    pass


@functools.lru_cache(maxsize=None)
def case(name: str) -> Model:
    """The case's inputs and the oracle-only expected answers.  Computed once;
    callers must not modify it."""
    inp = inputs(*CASES[name])
    m = Model()
    m.name, m.prof, m.table, m.assigned, m.pdb_allowed, m.pres = name, inp.prof, inp.table, inp.assigned, inp.pdb_allowed, inp.pres
    m.cfg = to_c_config(inp.prof)
    m.res, m.verdicts, m.chosen, m.victims, m.potential = dry_run(m.cfg, m.table, m.assigned, m.pdb_allowed, m.pres)
    return m
