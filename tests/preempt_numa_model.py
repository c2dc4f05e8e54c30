"""The preemption dry run under NodeNUMAResource with the frozen NUMA verdict
(koordhip_preempt_set_mode(KOORDHIP_PREEMPT_NUMA_FROZEN)), computed with the
CPU oracle alone.

preempt_model.select_victims already evaluates every hypothetical row with the
full oracle, the NodeNUMAResource Filter and filterAmplifiedCPUs included, and
moves only the row columns: the free-CPU masks, the allocated cpuset count and
the zone amounts stay as loaded, which is the plugin without
PreFilterExtensions.  What this module adds is step 1, as the walk's NumaRule:
a node whose FIRST failing plugin on the row the walk starts from holds an
UnschedulableAndUnresolvable reason is UNRESOLVABLE (upstream
nodesWherePreemptionMightHelp reads that plugin's code), found with
reasons_model.masks and abi.first_reasons.

Also the generated cases (preempt_model.inputs on a cluster with NUMA columns,
two of three preemptors cpuset pods, ~15 % of the nodes with room beside their
listed pods so that NodeResourcesFit passes and NodeNUMAResource decides) and
two hand-worked cases, `amp` and `frozen`.
"""
import functools
from unittest import mock

import numpy as np

import oracle
from koordinator_amd import abi, synth
from koordinator_amd import numa as nm
from koordinator_amd.config import shipped_profile, to_c_config, with_upstream
from koordinator_amd.snapshot import NodeTable

import preempt_cases as K
import preempt_model as M
import preempt_stream_model as S
import reasons_model as R

LOOSE_FRAC = 0.15


# --------------------------------------------------------------------- model
def unresolvable(cfg, table: NodeTable, pod: np.ndarray) -> np.ndarray:
    """[n] bool: the first failing plugin of `pod` on the rows of `table` gives an UnschedulableAndUnresolvable reason."""
    mask = R.masks(oracle.Oracle(cfg, table), np.ascontiguousarray(pod.reshape(1)))[0]
    return (abi.first_reasons(mask) & np.uint32(abi.REASON_UNRESOLVABLE_MASK)) != 0


class NumaRule(M.Rule):
    """Step 1 of the NUMA mode; the fit test and a move are the base walk's."""

    def __init__(self, cfg, table, pre, rows):
        self.unres = unresolvable(cfg, table, pre["pod"])

    def unresolvable(self, i):
        return bool(self.unres[i])


def dry_run(cfg, table, assigned, pdb_allowed, pres):
    return M.dry_run(cfg, table, assigned, pdb_allowed, pres, NumaRule)


def stream(cfg, table, assigned, pdb_allowed, pres):
    """preempt_stream_model.stream under NumaRule."""
    return S.stream(cfg, table, assigned, pdb_allowed, pres, rule=NumaRule)


# ---------------------------------------------------------------- generators
# name -> (n, n_pre, seed, NumaSpec, static filters)
CASES = {
    "one": (1, 1, M.SEED + 21, synth.NumaSpec(), False),
    "wave": (63, 3, M.SEED + 22, synth.NumaSpec(amp_frac=0.4, no_topology_frac=0.1, full_only_frac=0.15), False),
    "tiles": (257, 33, M.SEED + 23, synth.NumaSpec(policy_frac=0.4, no_topology_frac=0.05, full_only_frac=0.1), False),
    "zones8": (130, 3, M.SEED + 24, synth.NumaSpec(policy_frac=0.5, nodes_per_socket=4), False),
    "static": (130, 3, M.SEED + 25, synth.NumaSpec(), True),
}
DIRECTED = ("amp", "frozen")


def numa_profile(static=False):
    prof = shipped_profile(numa=True)
    return with_upstream(prof) if static else prof


def inputs(n, n_pre, seed, spec, static, base_per: int = 0, cpuset_of: int = 3) -> M.Inputs:
    """cpuset_of: all but the last of every `cpuset_of` preemptors are cpuset pods; base_per: preempt_model.inputs'."""
    prof = numa_profile(static)
    make_cluster = synth.make_cluster

    def cluster(cs, p):  # the NUMA columns (and the amplified allocatable) before the rows are tightened
        return synth.add_numa(make_cluster(cs, p), spec, prof, seed)

    with mock.patch.object(synth, "make_cluster", cluster):
        inp = M.inputs("static" if static else "base", n, n_pre, seed, False, base_per)
    table, a, pres = inp.table, inp.assigned, inp.pres
    # ~15 % of the nodes hold nothing but their listed pods: Fit passes there and NodeNUMAResource decides step 1
    loose = synth.uniform(seed, n, 940) < LOOSE_FRAC
    listed = np.bincount(a["node"], weights=a["pod"]["req"][:, abi.RES_CPU].astype(np.float64), minlength=n).astype(np.int64)
    table["requested0"][loose] = listed[loose]
    # the cpuset preemptors (two of three in the cases)
    pod = pres["pod"]
    cs = np.arange(n_pre) % cpuset_of != cpuset_of - 1
    codes = np.array([abi.numa_policy(*x) for x in synth.CPUSET_POLICIES], np.uint32)
    pol = (synth.splitmix64(seed, n_pre, 941) % np.uint64(len(codes))).astype(np.int64)
    pod["flags"][cs] |= np.uint32(abi.POD_CPUSET)
    pod["numa_cpus"][cs] = (pod["req"][cs, abi.RES_CPU] // 1000).astype(np.int32)
    pod["numa_policy"][cs] = codes[pol[cs]]
    pres["pod"] = pod
    return M.Inputs(prof, table, a, inp.pdb_allowed, pres)


# ------------------------------------------------------------ directed cases
def _numa_node(t: NodeTable, i: int, free_cpus, ncpu: int):
    """Node i: class 0, `free_cpus` free, the other CPUs allocated to cpuset pods."""
    t["numa_class"][i] = 0
    free = 0
    for c in free_cpus:
        free |= 1 << c
    t["numa_free0"][i] = np.uint64(free)
    t["numa_alloc_cnt"][i] = ncpu - len(free_cpus)


def _classes():
    classes = nm.ClassTable()
    topo = nm.linux_topology(2, 1, 4, 2)     # 2 sockets x 1 NUMA node x 4 cores x 2 threads = 16 CPUs
    classes.add(topo)
    return classes.records(), topo.num_cpus


def _cpuset(p, cpus, policy):
    p["pod"]["flags"] |= abi.POD_CPUSET
    p["pod"]["numa_cpus"] = cpus
    p["pod"]["numa_policy"] = abi.numa_policy(*policy)
    return p


AMP_PODS = 10
AMP_VICTIMS = [6, 5, 4, 3, 2, 1, 0]
AMP_FIT_ONLY_VICTIMS = [0]


def _amp() -> M.Inputs:
    """One node of 16 CPUs amplified by 2.0: allocatable 32 CPUs.  Cpuset pods
    hold 8 CPUs (8000 of Requested, not listed), others 2000, and ten listed
    pods 2 CPUs each: pod j has priority j + 1.  Requested = 30000.  The
    preemptor is a cpuset pod of 4 CPUs, no required bind policy.

    NodeResourcesFit: 4000 <= 32000 - Requested, i.e. Requested <= 28000: with
    all ten removed (10000) nine fit back, the last (pod 0) is the victim.
    filterAmplifiedCPUs: the request counts 8000, the 8 allocated CPUs 16000
    instead of 8000: 8000 <= 32000 - (Requested + 8000), i.e. Requested <=
    16000: pods 9, 8, 7 fit back (16000), pods 6 .. 0 do not."""
    pods = [K.A(0, 2000, j + 1, start=j) for j in range(AMP_PODS)]
    a = K.records(pods)
    t = K.table(1, a, extra=[10000])
    t["alloc0"][0] = 32000
    t.numa_classes, ncpu = _classes()
    _numa_node(t, 0, range(8, 16), ncpu)
    t["numa_amp_cpu"][0] = 2.0
    pre = _cpuset(K.preemptor(4000), 4, (abi.CPUBIND_NONE, abi.CPUBIND_FULL_PCPUS, abi.CPUEXCL_NONE))
    return M.Inputs(numa_profile(), t, a, (), np.array([pre], abi.PREEMPTOR_DTYPE))


FROZEN_VICTIMS = [0]


def _frozen() -> M.Inputs:
    """One node of 16 CPUs, all held by four listed cpuset pods of 4 CPUs
    (priorities 10, 20, 30, 40): no CPU is free and Requested is the
    allocatable.  Preemptor 0, a cpuset pod of 4 CPUs with the required policy
    FullPCPUs, finds no free CPU in Allocate whatever is removed: the victims'
    cpusets are not freed, UNFIT.  Preemptor 1, the same pod without a cpuset,
    is a candidate: three pods fit back, pod 0 (priority 10) is the victim."""
    pods = [K.A(0, 4000, 10 * (j + 1), start=j) for j in range(4)]
    for p in pods:
        p["pod"]["flags"] |= abi.POD_CPUSET
        p["pod"]["numa_cpus"] = 4
    a = K.records(pods)
    t = K.table(1, a)
    t["alloc0"][0] = 16000
    t.numa_classes, ncpu = _classes()
    _numa_node(t, 0, (), ncpu)
    full = (abi.CPUBIND_FULL_PCPUS, abi.CPUBIND_FULL_PCPUS, abi.CPUEXCL_NONE)
    pres = [_cpuset(K.preemptor(4000), 4, full), K.preemptor(4000)]
    return M.Inputs(numa_profile(), t, a, (), np.array(pres, abi.PREEMPTOR_DTYPE))


_DIRECTED = {"amp": _amp, "frozen": _frozen}
ALL_CASES = list(CASES) + list(DIRECTED)


class Model:
    pass


@functools.lru_cache(maxsize=None)
def case(name: str) -> Model:
    """The case's inputs and the expected answers of koordhip_preempt /
    koordhip_preempt_node_verdicts in the NUMA mode.  Computed once; callers
    must not modify it."""
    inp = _DIRECTED[name]() if name in _DIRECTED else inputs(*CASES[name])
    m = Model()
    m.name, m.prof, m.table, m.assigned, m.pdb_allowed, m.pres = name, inp.prof, inp.table, inp.assigned, inp.pdb_allowed, inp.pres
    m.cfg = to_c_config(inp.prof)
    m.res, m.verdicts, m.chosen, m.victims, m.potential = dry_run(m.cfg, m.table, m.assigned, m.pdb_allowed, m.pres)
    return m


@functools.lru_cache(maxsize=None)
def stream_case(name: str) -> Model:
    """... of koordhip_preempt_stream."""
    b = case(name)
    m = Model()
    m.name, m.prof, m.table, m.assigned, m.pdb_allowed, m.pres, m.cfg = name, b.prof, b.table, b.assigned, b.pdb_allowed, b.pres, b.cfg
    m.res, m.chosen, m.stats = stream(m.cfg, m.table, m.assigned, m.pdb_allowed, m.pres)
    return m
