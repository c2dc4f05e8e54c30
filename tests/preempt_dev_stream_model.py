"""The sequential preemption dry run under DeviceShare
(koordhip_preempt_stream_ext in the KOORDHIP_PREEMPT_DEVICE mode):
preempt_stream_model.stream's sequence with preempt_dev_model.DevRule's state.

S_k is preempt_stream_model's (gone pods off the rows and out of the lists,
nominated preemptors of preemptor k's priority and above on the rows, budgets
and quota lowered), extended by what the DEVICE mode moves:

    gone        also off xrequested by its xreq over its xmask, and for a device
                preemptor off its node's devices: dev_used[t][s] -= dev_per[t]
                for every slot of its dev_slots[t] (the walk's used - Pd starts
                lower; the free formula is unchanged)
    nominated   also its xreq on xrequested over its xmask (NodeInfo.AddPod)
                and NO devices: DeviceShare's AddPod finds no allocation of a
                nominated pod in the node's device cache (plugin.go:201-212)

Computed twice.  stream() is the overlay form: preempt_stream_model.stream
with a rule per preemptor that starts DevRule's state from S_k.  rebuilt() is
the restatement from scratch: for preemptor k the table is rebuilt with
V_0..V_{k-1} deleted (rows, xrequested and dev_used lowered, the pods dropped
from the assigned arrays, budgets floored, q_used lowered, the qualifying
nominated pods added to rows and xrequested) and preempt_dev_model.dry_run
answers the one preemptor on it.  case() asserts that both agree on every
verdict of every node, the pick and the victims.

The engine builds the call as the per-preemptor chain (every 256-node block
evaluates every preemptor), so its koordhip_preempt_stream_stats follow from
the results by chain_stats().
"""
import functools
from unittest import mock

import numpy as np

from koordinator_amd import abi
from koordinator_amd.config import to_c_config, with_deviceshare
from koordinator_amd.deviceshare import XRES_INDEX, NVIDIA_GPU

import preempt_cases as K
import preempt_dev_model as D
import preempt_model as M
import preempt_numa_model as N
import preempt_stream_model as S

DT, DR, NX, G = D.DT, D.DR, D.NX, D.G
BRANCHES = {}          # branch name -> times taken (the coverage conditions read it)


def _took(name):
    BRANCHES[name] = BRANCHES.get(name, 0) + 1


def _scalars(rec):
    """(j, amount) of the extended scalars a koordhip_pod_ext / koordhip_assigned_ext record holds."""
    return [(j, int(rec["xreq"][j])) for j in range(NX) if (int(rec["xmask"]) >> j) & 1]


def _devices(ax):
    """(type, slot, amounts) of the devices a koordhip_assigned_ext record holds."""
    return [(t, s, np.array(ax["dev_per"][t], np.int64)) for t in range(DT) for s in range(abi.DEV_SLOTS)
            if (int(ax["dev_slots"][t]) >> s) & 1]


# ------------------------------------------------------------ the overlay form
class StreamDevRule(D.DevRule):
    """DevRule started from S_k: `table` holds the rows preempt_stream_model.stream
    moved; the gone pods' scalars and devices and the nominated pods' scalars are
    this rule's.  gone: table indices; nominated: (node, ext record, priority)."""

    def __init__(self, cfg, table, pre, rows, x=None, ax=None, assigned=None, numa=False, gone=(), nominated=()):
        super().__init__(cfg, table, pre, rows, x=x, ax=ax, assigned=assigned, numa=numa)
        n = table.n
        self.out = [set() for _ in range(n)]          # the listed pods off node i at the moment
        self.nom_x = np.zeros((n, NX), np.int64)      # what the qualifying nominated pods add to xrequested
        for j in gone:
            i = int(assigned["node"][j])
            rec = None if ax is None else ax[j]
            if rec is None or not (_scalars(rec) or _devices(rec)):
                _took("gone_without_ext")
                continue
            for r, q in _scalars(rec):
                self.xr[i, r] -= q
            devs = _devices(rec)
            _took("gone_with_devices" if devs else "gone_scalars_only")
            if not self.device or self.nodes[i] is None:
                continue
            for t, s, amt in devs:
                used = self.nodes[i][t]["used"][s]
                assert all(int(a) <= u for a, u in zip(amt, used)), "a gone pod held what dev_used counts"
                self.nodes[i][t]["used"][s] = [u - int(a) for a, u in zip(amt, used)]
                _took("gone_devices_lowered")
        prio = int(pre["priority"])
        for i, nx, p in nominated:
            if not _scalars(nx):
                continue
            if p < prio:
                _took("nominated_scalar_below_priority")
                continue
            _took("nominated_scalar")
            for r, q in _scalars(nx):
                self.nom_x[i, r] += q
        self.xr += self.nom_x

    def fits(self, status, i):
        if status == 0 and not D.xfit(self.x, self.xalloc[i], self.xr[i]) and \
                D.xfit(self.x, self.xalloc[i], self.xr[i] - self.nom_x[i]):
            _took("nominated_scalar_blocks")
        return super().fits(status, i)

    def moved(self, i, a, sign):
        j = (a.__array_interface__["data"][0] - self.assigned.__array_interface__["data"][0]) // self.assigned.itemsize
        (self.out[i].add if sign < 0 else self.out[i].discard)(int(j))
        super().moved(i, a, sign)


class _Sequence:
    """The rule of preempt_stream_model.stream's k-th select_victims call.  What
    the sequence decided for k - 1 (its pick, read where stream() calls
    preempt_model.pick; its victims, the pods off the picked node when the walk
    ended) is settled when the rule of k is made."""

    def __init__(self, assigned, pres, ext, ax, numa):
        self.assigned, self.pres, self.ext, self.ax, self.numa = assigned, pres, ext, ax, numa
        self.gone, self.nominated, self.verdicts = [], [], []
        self.rule, self.node = None, -1

    def __call__(self, cfg, table, pre, rows):
        k = len(self.verdicts)
        if self.rule is not None and self.node >= 0:
            self.gone += sorted(self.rule.out[self.node])
            self.nominated.append((self.node, self.ext[k - 1], int(self.pres[k - 1]["priority"])))
        self.rule = StreamDevRule(cfg, table, pre, rows, x=self.ext[k], ax=self.ax, assigned=self.assigned,
                                  numa=self.numa, gone=tuple(self.gone), nominated=tuple(self.nominated))
        return self.rule

    def picked(self, verdicts, res):
        self.verdicts.append(verdicts.copy())
        self.node = int(res["node"])


def chain_stats(stats: dict, n: int, n_pre: int) -> dict:
    """koordhip_preempt_stream_stats of the per-preemptor chain from preempt_stream_model's bookkeeping: every block
    evaluates every preemptor, none is skipped; full_recomputes keeps its meaning (a changed budget or a freed quota)."""
    nb = (n + S.BLOCK - 1) // S.BLOCK
    return dict(full_recomputes=stats["full_recomputes"], block_recomputes=n_pre * nb, blocks_skipped=0)


def stream(cfg, table, assigned, pdb_allowed, pres, ext=None, ax=None, numa=False):
    """(results, full victim lists per preemptor, stats, verdicts [p][n]).  cfg: the profile WITHOUT DeviceShare."""
    ext = ext if ext is not None else abi.pod_ext_array(len(pres))
    seq = _Sequence(assigned, pres, ext, ax, numa)
    pick = M.pick

    def observed(verdicts):
        res = pick(verdicts)
        seq.picked(verdicts, res)
        return res

    with mock.patch.object(M, "pick", observed):
        res, chosen, stats = S.stream(cfg, table, assigned, pdb_allowed, pres, rule=seq)
    ver = np.array(seq.verdicts, abi.PREEMPT_NODE_DTYPE).reshape(len(pres), table.n)
    return res, chosen, chain_stats(stats, table.n, len(pres)), ver


# --------------------------------------------------- the restatement from scratch
def rebuilt_inputs(table, assigned, pdb_allowed, pres, ext, ax, k, chosen, nodes):
    """S_k as a table of its own: V_0..V_{k-1} deleted, the qualifying nominated
    pods added.  (table, assigned, ax, budgets, preemptor k with its q_used
    lowered, keep: the rebuilt arrays' indices in `assigned`)."""
    t = table.copy()
    has_x = table.has_ext

    def row(i, pod, sign):
        for r in range(M.NRES):
            t[f"requested{r}"][i] += sign * int(pod["req"][r])
        t["nz_cpu_m"][i] += sign * int(pod["nz_cpu_m"])
        t["nz_mem"][i] += sign * int(pod["nz_mem"])
        t["npods"][i] += sign

    allowed = [int(x) for x in pdb_allowed]
    pre = pres[k].copy()
    prio, quota = int(pre["priority"]), int(pre["quota"])
    freed = [0] * abi.PREEMPT_QRES
    gone = []
    for j in range(k):
        if nodes[j] < 0:
            continue
        for v in chosen[j]:
            a = assigned[v]
            i = int(a["node"])
            gone.append(v)
            row(i, a["pod"], -1)
            if ax is not None and has_x:
                for r, q in _scalars(ax[v]):
                    t["xrequested"][i, r] -= q
                for ty, s, amt in _devices(ax[v]):
                    t["dev_used"][i, ty, s] -= amt
            for b in range(len(allowed)):
                if (int(a["pdb_mask"]) >> b) & 1:
                    allowed[b] = max(0, allowed[b] - 1)
            if quota >= 0 and int(pres[j]["quota"]) == quota and int(a["flags"]) & abi.ASG_IN_QUOTA:
                for d in range(abi.PREEMPT_QRES):
                    freed[d] += int(a["qreq"][d])
        if int(pres[j]["priority"]) >= prio:
            row(nodes[j], pres[j]["pod"], +1)
            if has_x:
                for r, q in _scalars(ext[j]):
                    t["xrequested"][nodes[j], r] += q
    for d in range(abi.PREEMPT_QRES):
        pre["q_used"][d] = max(0, int(pre["q_used"][d]) - freed[d])
    keep = np.setdiff1d(np.arange(len(assigned)), np.array(gone, np.int64))
    a_k = np.ascontiguousarray(assigned[keep])
    ax_k = None if ax is None else np.ascontiguousarray(ax[keep])
    return t, a_k, ax_k, tuple(allowed), np.array([pre], abi.PREEMPTOR_DTYPE), keep


def rebuilt(cfg, table, assigned, pdb_allowed, pres, ext, ax, numa, k, chosen, nodes):
    """Preemptor k alone on that table: (result, verdicts [n], victims as indices of `assigned`)."""
    ext = ext if ext is not None else abi.pod_ext_array(len(pres))
    t, a_k, ax_k, allowed, pre, keep = rebuilt_inputs(table, assigned, pdb_allowed, pres, ext, ax, k, chosen, nodes)
    res, ver, vic, _, _ = D.dry_run(cfg, t, a_k, allowed, pre, ext[k:k + 1], ax_k, numa)
    return res[0], ver[0], [int(keep[j]) for j in vic[0]]


def check_rebuilt(cfg, table, assigned, pdb_allowed, pres, ext, ax, numa, res, chosen, ver):
    """The overlay form's answers are the rebuilt tables': every verdict of every node, the pick, the victims."""
    nodes = [int(x) for x in res["node"]]
    for k in range(len(pres)):
        r, v, vic = rebuilt(cfg, table, assigned, pdb_allowed, pres, ext, ax, numa, k, chosen, nodes)
        assert v.tobytes() == ver[k].tobytes(), f"preemptor {k}: verdicts differ at node " \
            f"{int(np.flatnonzero(v != ver[k])[0])}"
        assert r.tobytes() == res[k].tobytes(), f"preemptor {k}: pick {r} against {res[k]}"
        assert vic == [int(j) for j in chosen[k]], f"preemptor {k}: victims {vic} against {chosen[k]}"


# ------------------------------------------------------------ hand-worked cases
NV = XRES_INDEX[NVIDIA_GPU]


def _gpu_nodes(n, pods, holders, nvidia=True, gpus=1):
    """n nodes of 10 CPUs and `gpus` GPUs; holders: listed pod j -> (slot, percent) of its node's GPU, with
    nvidia.com/gpu 1 for a whole one (nvidia: the nodes advertise the scalar, one per GPU)."""
    a, ax = D._pods(*pods)
    t = D._table(n, a)
    for i in range(n):
        D._gpus(t, i, gpus)
        if nvidia:
            t["xalloc"][i, NV] = gpus
    for j, (s, pct) in holders.items():
        i = int(a["node"][j])
        D._hold(t, ax, j, i, G, s, pct)
        if nvidia and pct == 100:
            ax["xreq"][j, NV], ax["xmask"][j] = 1, 1 << NV
            t["xrequested"][i, NV] += 1
    return t, a, ax


def _many(t, a, ax, pres, exts, prof=None):
    ext = np.concatenate(exts)
    return M.Inputs(prof or D._profile(), t, a, (), np.array(pres, abi.PREEMPTOR_DTYPE)), ext, ax


def _reused():
    """freed GPU reused.  Nodes 0 and 1, one GPU and one nvidia.com/gpu each.
    Node 0: pod 0 (priority 10) holds the GPU and the scalar, pod 2 (priority 5)
    holds neither.  Node 1: pod 1 (priority 20) holds the GPU and the scalar.
    Preemptors 0 and 1 (priority 1000) ask 1 CPU, a whole GPU and nvidia.com/gpu 1.

    Alone, each takes node 0: pods 0 and 2 removed, pod 0 back: the GPU is taken:
    victim; pod 2 back: fits: reprieved; its victim of priority 10 beats node
    1's of priority 20.  Both claim pod 0.

    In sequence preemptor 1 sees node 0 without pod 0 (GPU free, scalar 0 of 1)
    and with preemptor 0 nominated: its nvidia.com/gpu is Requested again, 1 > 1
    - 1.  Pod 2 is removed, NodeResourcesFit still fails: UNFIT.  Node 1 answers
    with pod 1.  Nothing nominated holds the GPU itself; the scalar alone keeps
    the two apart."""
    t, a, ax = _gpu_nodes(2, [K.A(0, 1000, 10, start=1), K.A(1, 1000, 20, start=2), K.A(0, 1000, 5, start=3)],
                          {0: (0, 100), 1: (0, 100)})
    x = D._ext(100, 100, nvidia=1)
    return _many(t, a, ax, [K.preemptor(1000), K.preemptor(1000)], [x, x])


def _nodevice_held():
    """nominated pod holds no device.  _reused's nodes without any scalar; the
    preemptors ask 60 % of a GPU (gpu-core 60, gpu-memory-ratio 60) and no
    scalar.  Preemptor 0 takes node 0 and pod 0.  Preemptor 1 finds node 0's
    GPU free: pod 0 is gone and DeviceShare's AddPod found no allocation of the
    nominated preemptor 0 in the node's device cache, so nothing holds the 60 %
    it was promised.  Pod 2 is removed and fits back: node 0 needs no victim and
    wins outright: 120 % of one minor are nominated.  This is the reference's
    behaviour."""
    t, a, ax = _gpu_nodes(2, [K.A(0, 1000, 10, start=1), K.A(1, 1000, 20, start=2), K.A(0, 1000, 5, start=3)],
                          {0: (0, 100), 1: (0, 100)}, nvidia=False)
    x = D._ext(60, 60)
    return _many(t, a, ax, [K.preemptor(1000), K.preemptor(1000)], [x, x])


def _gate():
    """priority gate.  _reused's nodes.  Preemptor 0 (priority 100) takes node 0
    and pod 0.  Preemptor 1 (priority 1000) does not see preemptor 0's pod (100 <
    1000): node 0 has its scalar and its GPU free, pod 2 is removed and fits
    back: no victim.  Preemptor 2 (priority 100) sees both (100 >= 100, 1000 >=
    100): nvidia.com/gpu is Requested twice of 1, and without pod 2 as well:
    UNFIT.  Node 1 answers with pod 1."""
    t, a, ax = _gpu_nodes(2, [K.A(0, 1000, 10, start=1), K.A(1, 1000, 20, start=2), K.A(0, 1000, 5, start=3)],
                          {0: (0, 100), 1: (0, 100)})
    x = D._ext(100, 100, nvidia=1)
    return _many(t, a, ax, [K.preemptor(1000, prio=100), K.preemptor(1000, prio=1000), K.preemptor(1000, prio=100)],
                 [x, x, x])


def _share():
    """gone victim's share.  One node, two GPUs, no scalar.  Minor 0 is held by a
    pod that is not listed; pod 0 (priority 10) holds 50 % of minor 1, pod 1
    (priority 5) holds no device.  Preemptor 0 asks 60 %: 50 % are free; both
    removed: the minor is free; pod 0 back: it does not fit: victim; pod 1 back:
    reprieved.  Preemptor 1 asks a whole GPU.  Pod 0 is gone, so used of minor 1
    starts at 0 for the whole walk and the nominated preemptor 0 holds nothing;
    pod 1 is removed and fits back: CANDIDATE without a victim.  With the gone
    pod's share still in used no removal frees a GPU: UNFIT, no node."""
    t, a, ax = _gpu_nodes(1, [K.A(0, 1000, 10, start=1), K.A(0, 1000, 5, start=2)], {0: (1, 50)}, nvidia=False, gpus=2)
    D._hold(t, ax, None, 0, G, 0, 100)
    return _many(t, a, ax, [K.preemptor(1000), K.preemptor(1000)], [D._ext(60, 60), D._ext(100, 100)])


def _twice():
    """no victim claimed twice.  _reused's nodes without pod 2, three preemptors of one priority
    asking a whole GPU and its scalar.  Alone all three take node 0 and claim pod
    0.  In sequence: node 0 with pod 0, node 1 with pod 1, and for the third both
    nodes have the scalar nominated and nothing left to remove: no node."""
    t, a, ax = _gpu_nodes(2, [K.A(0, 1000, 10, start=1), K.A(1, 1000, 20, start=2)], {0: (0, 100), 1: (0, 100)})
    x = D._ext(100, 100, nvidia=1)
    return _many(t, a, ax, [K.preemptor(1000) for _ in range(3)], [x, x, x])


def _scalar_gone():
    """A gone pod with scalars only.  One node, two GPUs, nvidia.com/gpu 2 of 2
    Requested: one by a pod that is not listed, which holds minor 0, one by pod 0
    (priority 10), which holds no device; pod 1 (priority 5) holds nothing.
    Preemptor 0 (priority 100) asks a whole GPU and the scalar: minor 1 is free,
    1 > 2 - 2; both removed: fits; pod 0 back: the scalar again: victim; pod 1
    back: reprieved.  Preemptor 1 (priority 1000) does not see preemptor 0; pod
    0's scalar is off Requested: 1 <= 2 - 1; pod 1 removed and back: no victim."""
    t, a, ax = _gpu_nodes(1, [K.A(0, 1000, 10, start=1), K.A(0, 1000, 5, start=2)], {}, gpus=2)
    D._hold(t, ax, None, 0, G, 0, 100)
    ax["xreq"][0, NV], ax["xmask"][0] = 1, 1 << NV
    t["xrequested"][0, NV] = 2
    x = D._ext(100, 100, nvidia=1)
    return _many(t, a, ax, [K.preemptor(1000, prio=100), K.preemptor(1000, prio=1000)], [x, x])


def _numa_hand():
    """NUMA (DEVICE | NUMA_FROZEN).  Two nodes of 16 CPUs and one GPU, no scalar.
    Node 0: no free CPU, four listed cpuset pods of 4 CPUs (priorities 10..40),
    pod 0 holds the GPU.  Node 1: CPUs 8..15 free, pod 4 (priority 10, 8 CPUs)
    holds the GPU, pod 5 (priority 20, 8 CPUs) holds none; Requested is the
    allocatable.  Preemptor 0: a cpuset pod of 4 CPUs, required FullPCPUs, a
    whole GPU.  Node 0: the frozen verdict fails whatever is removed: UNFIT.  Node
    1: both removed; pod 5 back: 8 + 4 <= 16 and the GPU is free: reprieved; pod
    4 back: 16 + 4 > 16: victim.  Preemptor 1: the same without a cpuset.  Node 0:
    pods 3, 2, 1 fit back, pod 0 does not: one victim.  Node 1: pod 4 is gone
    and preemptor 0 nominated: 8 + 4 Requested, the GPU free (nothing nominated
    holds it); pod 5 is removed and fits back: no victim, wins outright."""
    pods = [K.A(0, 4000, 10 * (j + 1), start=j) for j in range(4)]
    for p in pods:
        p["pod"]["flags"] |= abi.POD_CPUSET
        p["pod"]["numa_cpus"] = 4
    pods += [K.A(1, 8000, 10, start=5), K.A(1, 8000, 20, start=6)]
    a, ax = D._pods(*pods)
    t = D._table(2, a)
    t["alloc0"][:] = 16000
    t.numa_classes, ncpu = N._classes()
    N._numa_node(t, 0, (), ncpu)
    N._numa_node(t, 1, range(8, 16), ncpu)
    for i, j in ((0, 0), (1, 4)):
        D._gpus(t, i, 1)
        D._hold(t, ax, j, i, G, 0, 100)
    full = (abi.CPUBIND_FULL_PCPUS, abi.CPUBIND_FULL_PCPUS, abi.CPUEXCL_NONE)
    pres = [N._cpuset(K.preemptor(4000), 4, full), K.preemptor(4000)]
    x = D._ext(100, 100)
    return _many(t, a, ax, pres, [x, x], prof=with_deviceshare(N.numa_profile()))


_HAND = {"reused": _reused, "nodevice_held": _nodevice_held, "gate": _gate, "share": _share, "twice": _twice,
         "scalar_gone": _scalar_gone, "numa_hand": _numa_hand}
HAND = tuple(_HAND)
# by hand: per preemptor (node, victims in append order)
EXPECTED = {
    "reused": [(0, [0]), (1, [1])],
    "nodevice_held": [(0, [0]), (0, [])],
    "gate": [(0, [0]), (0, []), (1, [1])],
    "share": [(0, [0]), (0, [])],
    "twice": [(0, [0]), (1, [1]), (-1, [])],
    "scalar_gone": [(0, [0]), (0, [])],
    "numa_hand": [(1, [4]), (1, [])],
}
# ... and of the independent batch (koordhip_preempt_ext), where it is part of the case's point
EXPECTED_INDEPENDENT = {
    "reused": [(0, [0]), (0, [0])],
    "twice": [(0, [0]), (0, [0]), (0, [0])],
}
GENERATED = ("lane", "wave", "tiles", "numa")     # preempt_dev_model.CASES' shapes
ALL_CASES = list(GENERATED) + list(HAND)


def claimed_twice(chosen) -> int:
    """Victims more than one preemptor of a batch claims."""
    seen, twice = set(), set()
    for v in chosen:
        for j in v:
            (twice if j in seen else seen).add(int(j))
    return len(twice)


class Model:
    pass


@functools.lru_cache(maxsize=None)
def case(name: str) -> Model:
    """The case's inputs and the expected answers of koordhip_preempt_stream_ext
    in the DEVICE mode, in both forms.  Computed once; callers must not modify it."""
    numa = name == "numa_hand" or (name in D.CASES and D.CASES[name][4])
    inp, ext, ax = _HAND[name]() if name in _HAND else D.inputs(*D.CASES[name])
    m = Model()
    m.name, m.prof, m.table, m.assigned, m.pdb_allowed, m.pres = name, inp.prof, inp.table, inp.assigned, inp.pdb_allowed, inp.pres
    m.ext, m.ax, m.numa = ext, ax, numa
    m.cfg = to_c_config(inp.prof)
    m.base_cfg = to_c_config(D.without_plugin(inp.prof))
    before = dict(BRANCHES)
    m.res, m.chosen, m.stats, m.verdicts = stream(m.base_cfg, m.table, m.assigned, m.pdb_allowed, m.pres, ext, ax, numa)
    m.branches = {k: v - before.get(k, 0) for k, v in BRANCHES.items() if v - before.get(k, 0)}
    check_rebuilt(m.base_cfg, m.table, m.assigned, m.pdb_allowed, m.pres, ext, ax, numa, m.res, m.chosen, m.verdicts)
    return m
