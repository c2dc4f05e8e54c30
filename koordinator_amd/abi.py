"""ctypes mirror of include/koordhip.h and the loader for libkoordhip.so.

The library is built in-tree by __graft_entry__.build() into
koordinator_amd/lib/libkoordhip.so.  There is no fallback: if the library is
missing, importing the engine raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

KOORDHIP_ABI_VERSION = 15
NRES = 5
NPLUGINS = 4

PLUGIN_FIT, PLUGIN_LOADAWARE, PLUGIN_NUMA, PLUGIN_RESERVATION = 1, 2, 4, 8
PLUGIN_NODE_STATIC, PLUGIN_BALANCED = 16, 32
# normalized-score plugins (the exact sequential cycle, koordhip_place_stream_ext)
PLUGIN_DEVICESHARE, PLUGIN_AFFINITY_SCORE, PLUGIN_TAINT_SCORE, PLUGIN_PTS, PLUGIN_IPA = 64, 128, 256, 512, 1024
NEXT_PLUGINS = 5
EXT_PLUGIN_BITS = (PLUGIN_DEVICESHARE, PLUGIN_AFFINITY_SCORE, PLUGIN_TAINT_SCORE, PLUGIN_PTS, PLUGIN_IPA)
NORMALIZED_PLUGINS = PLUGIN_DEVICESHARE | PLUGIN_AFFINITY_SCORE | PLUGIN_TAINT_SCORE | PLUGIN_PTS | PLUGIN_IPA
PTS_KEYS, PTS_DOMAINS, PTS_CONS, PTS_CLASSES, PTS_POD = 4, 64, 8, 8, 4
PTS_HARD, PTS_SELF = 1, 2
IPA_ENTRIES = 32
IPA_SELF = 1
NXRES = 8
DEV_TYPES, DEV_SLOTS, DEV_RES = 3, 8, 3
DEV_GPU, DEV_RDMA, DEV_FPGA = 0, 1, 2
PODX_DEVICE = 1
# upstream NodeUnschedulable / NodeName / NodeAffinity / TaintToleration all map
# to the host-resolved static filter bit
PLUGIN_BITS = {"NodeResourcesFit": PLUGIN_FIT, "LoadAwareScheduling": PLUGIN_LOADAWARE,
               "NodeNUMAResource": PLUGIN_NUMA, "Reservation": PLUGIN_RESERVATION,
               "NodeUnschedulable": PLUGIN_NODE_STATIC, "NodeAffinity": PLUGIN_NODE_STATIC,
               "NodeName": PLUGIN_NODE_STATIC,
               "TaintToleration": PLUGIN_NODE_STATIC, "NodeResourcesBalancedAllocation": PLUGIN_BALANCED}
# plugin_weight[p] / score plane p
SCORE_PLUGIN_BITS = (PLUGIN_FIT, PLUGIN_LOADAWARE, PLUGIN_NUMA, PLUGIN_BALANCED)
MAX_STATIC_CLASSES = 32
RES_CPU, RES_MEM, RES_EPH, RES_BCPU, RES_BMEM = range(5)

LA_HAS_METRIC, LA_FILTER_SKIP, LA_SCORE_EXPIRED, LA_FILTER_USAGE = 1, 2, 4, 8
LA_PROD_MODE, LA_HAS_PODS_METRIC, LA_AGGREGATED = 16, 32, 64

POD_PROD, POD_DAEMONSET, POD_HAS_REQ, POD_REQ_BCPU, POD_REQ_BMEM = 1, 2, 4, 8, 16
POD_CPUSET, POD_NUMA_SKIP, POD_NUMA_ERROR = 32, 64, 128
POD_KEY_CPU, POD_KEY_MEM = 256, 512
POD_RESV_AFFINITY = 1024
POD_RESERVE = 2048                  # a reserve pod (IsReservePod): its reservation's nodeName / AllocatePolicy checks
POD_RESERVE_POLICY_SHIFT = 12       # bits 12-13: the reserve pod's AllocatePolicy (RESV_POLICY_* codes)
POD_RESV_OPERATING = 16384          # a reservation-operating-mode pod (AllocatePolicy Aligned in bits 12-13)
POD_CPUSET_QOS = 32768              # AllowUseCPUSet: koord-prod and QoS LSE / LSR (nodenumaresource/util.go:42-49)

RESV_PRESENT, RESV_ALLOCATE_ONCE, RESV_UNSCHEDULABLE, RESV_ORDERED = 1, 2, 4, 8
RESV_KEY_CPU, RESV_KEY_MEM = 16, 32
RESV_POLICY_SHIFT, RESV_GROUP_SHIFT = 6, 8
RESV_POLICY_DEFAULT, RESV_POLICY_ALIGNED, RESV_POLICY_RESTRICTED = 0, 1, 2
RESV_MAX_GROUPS, RESV_MAX_ORDERS = 64, 1024
RESV_SLOTS = 4   # Available reservations per node on the pipelined greedy
RESV_SLOTS_MAX = 8   # ... in a snapshot (koordhip_node_soa.resv_slots <= this; more than RESV_SLOTS: the sequential cycle)

CPUBIND_NONE, CPUBIND_FULL_PCPUS, CPUBIND_SPREAD_BY_PCPUS = 0, 1, 2
CPUEXCL_NONE, CPUEXCL_PCPU, CPUEXCL_NUMA = 0, 1, 2
NODE_CPUBIND_NONE, NODE_CPUBIND_FULL_PCPUS_ONLY, NODE_CPUBIND_SPREAD_BY_PCPUS = 0, 1, 2
NODE_NUMA_MOST_ALLOCATED = 4
NODE_NUMA_POLICY_SHIFT = 3
NUMA_TOPO_NONE, NUMA_TOPO_BEST_EFFORT, NUMA_TOPO_RESTRICTED, NUMA_TOPO_SINGLE_NUMA_NODE = 0, 1, 2, 3
NUMA_MAX_CPUS, NUMA_MAX_NODES, NUMA_WORDS = 256, 8, 4
NUMA_MAX_ZONES = 8


def numa_policy(required: int = 0, preferred: int = 0, exclusive: int = 0) -> int:
    return (required & 3) | ((preferred & 3) << 2) | ((exclusive & 3) << 4)

ST_FIT_FAIL, ST_LA_FAIL, ST_NUMA_FAIL, ST_RESV_FAIL, ST_STATIC_FAIL = 1, 2, 4, 8, 16
ST_DEVICE_FAIL, ST_XFIT_FAIL, ST_PTS_FAIL, ST_IPA_FAIL = 32, 64, 128, 256
UNSCHEDULABLE, RESERVE_FAILED = -1, -2
E_INVAL, E_STATE, E_RESERVE = -1, -3, -6
UNIQUE_ID_BYTES = 128

_i64p = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)
_u64p = C.POINTER(C.c_uint64)


class KoordhipKernelStats(C.Structure):
    """include/koordhip.h koordhip_kernel_stats"""
    _fields_ = [("scan_ms", C.c_double), ("scan_launches", C.c_int64),
                ("select_ms", C.c_double), ("select_launches", C.c_int64),
                ("resolve_ms", C.c_double), ("resolve_launches", C.c_int64),
                ("total_ms", C.c_double), ("evals", C.c_int64), ("pods", C.c_int64), ("rounds", C.c_int64),
                ("round_pods", C.c_int64), ("lag", C.c_int64), ("executed_evals", C.c_int64),
                ("plan_us", C.c_int32), ("flags", C.c_int32)]


KSTAT_LOCAL = 1


class KoordhipConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("filter_plugins", C.c_uint32),
        ("score_plugins", C.c_uint32),
        ("device", C.c_int32),
        ("plugin_weight", C.c_int64 * NPLUGINS),
        ("fit_weight", C.c_int64 * NRES),
        ("la_weight_cpu", C.c_int64),
        ("la_weight_mem", C.c_int64),
        ("la_score_according_prod_usage", C.c_int32),
        ("batch_pods", C.c_int32),
        ("numa_weight_cpu", C.c_int32),
        ("numa_weight_mem", C.c_int32),
        ("profile_kernels", C.c_int32),
        ("numa_most_allocated", C.c_int32),
        ("reservation_weight", C.c_int32),
        ("reserved", C.c_int32 * 5),
        ("ext_weight", C.c_int32 * NEXT_PLUGINS),
        ("dev_most_allocated", C.c_int32),
        ("dev_res_weight", C.c_int32 * 5),
        ("reserved2", C.c_int32 * 1),
    ]


class KoordhipNodeSoa(C.Structure):
    _fields_ = [
        ("alloc", _i64p * NRES),
        ("alloc_pods", _i32p),
        ("requested", _i64p * NRES),
        ("nz_cpu_m", _i64p),
        ("nz_mem", _i64p),
        ("npods", _i32p),
        ("la_alloc_cpu_m", _i64p),
        ("la_alloc_mem", _i64p),
        ("la_used_cpu_m", _i64p),
        ("la_used_mem", _i64p),
        ("la_used_prod_cpu_m", _i64p),
        ("la_used_prod_mem", _i64p),
        ("laf_used_m", _i64p * 2),
        ("laf_total_m", _i64p * 2),
        ("laf_prod_used_m", _i64p * 2),
        ("laf_thr", _i64p * 2),
        ("laf_prod_thr", _i64p * 2),
        ("la_flags", _u8p),
        ("numa_classes", C.c_void_p),
        ("n_numa_classes", C.c_int32),
        ("reserved0", C.c_int32),
        ("numa_class", _i32p),
        ("numa_free", _u64p * NUMA_WORDS),
        ("numa_excl_pcpu", _u64p * NUMA_WORDS),
        ("numa_excl_numa", _u64p * NUMA_WORDS),
        ("numa_alloc_cnt", _i32p),
        ("numa_flags", _u8p),
        ("numa_zone_alloc", _i64p),
        ("numa_zone_used", _i64p),
        ("numa_amp_cpu", C.POINTER(C.c_double)),
        ("resv_flags", C.POINTER(C.c_uint32)),
        ("resv_order_rank", _i32p),
        ("resv_alloc", _i64p * 2),
        ("resv_nz", _i64p * 2),
        ("resv_allocated", _i64p * 2),
        ("resv_assigned", _i32p),
        ("static_allow", C.POINTER(C.c_uint32)),
        ("resv_slots", C.c_int32),
        ("reserved1", C.c_int32),
        ("resv_cpus", _u64p * NUMA_WORDS),
        ("dev_slots", C.c_int32),
        ("reserved2", C.c_int32),
        ("dev_present", _u8p),
        ("dev_minor", _i32p),
        ("dev_total", _i64p),
        ("dev_used", _i64p),
        ("xalloc", _i64p),
        ("xrequested", _i64p),
        ("static_score", C.POINTER(C.c_uint16) * 2),
        ("pts_keys", C.c_int32),
        ("pts_hostname", C.c_uint32),
        ("pts_ndom", C.c_int32 * PTS_KEYS),
        ("pts_cons", C.c_int32),
        ("pts_classes", C.c_int32),
        ("pts_cons_key", C.c_int32 * PTS_CONS),
        ("pts_dom", _i32p),
        ("pts_cnt", _i32p),
        ("pts_elig", C.POINTER(C.c_uint16)),
        ("ipa_ents", C.c_int32),
        ("ipa_reserved", C.c_int32),
        ("ipa_ent_key", C.c_int32 * IPA_ENTRIES),
        ("ipa_cnt", _i32p),
        ("resv_dev_slot", _i32p),
        ("resv_dev", _i64p),
        ("resv_xalloc", _i64p),
        ("resv_xallocated", _i64p),
    ]


# numpy twin of koordhip_numa_class
NUMA_CLASS_DTYPE = np.dtype([
    ("num_cpus", "<i4"), ("num_cores", "<i4"), ("num_nodes", "<i4"), ("num_sockets", "<i4"),
    ("cpus_per_core", "<i4"), ("reserved0", "<i4"),
    ("cpu_id", "<i4", (NUMA_MAX_CPUS,)),
    ("node_of", "u1", (NUMA_MAX_CPUS,)),
    ("socket_of", "u1", (NUMA_MAX_CPUS,)),
], align=True)
assert NUMA_CLASS_DTYPE.itemsize == 24 + 4 * 256 + 512


class KoordhipTopk(C.Structure):
    _fields_ = [("node", C.c_int32), ("score", C.c_int32)]


# numpy twin of koordhip_pod (96 bytes)
POD_DTYPE = np.dtype([
    ("req", "<i8", (NRES,)),
    ("nz_cpu_m", "<i8"),
    ("nz_mem", "<i8"),
    ("est_cpu", "<i8"),
    ("est_mem", "<i8"),
    ("flags", "<u4"),
    ("numa_cpus", "<i4"),
    ("numa_policy", "<u4"),
    ("static_class", "<i4"),
    ("resv_match", "<u8"),
], align=True)
assert POD_DTYPE.itemsize == 96
TOPK_DTYPE = np.dtype([("node", "<i4"), ("score", "<i4")])
# numpy twin of koordhip_diag (136 bytes): slot b of any / first counts status bit 1 << b
DIAG_BITS = 16
DIAG_DTYPE = np.dtype([("feasible", "<i4"), ("reserved", "<i4"), ("any", "<i4", (DIAG_BITS,)),
                       ("first", "<i4", (DIAG_BITS,))])
assert DIAG_DTYPE.itemsize == 136
# the framework's Filter order behind `first` (include/koordhip.h)
FILTER_ORDER = (ST_STATIC_FAIL, ST_FIT_FAIL, ST_LA_FAIL, ST_NUMA_FAIL, ST_RESV_FAIL)
# ... with the sequential cycle's plugins (koordhip_diagnose_ext): the (upstream) default list, then the
# koordinator plugins as scheduler-config.yaml's filter.enabled appends them; XFIT is NodeResourcesFit too
FILTER_ORDER_EXT = (ST_STATIC_FAIL, ST_FIT_FAIL, ST_XFIT_FAIL, ST_PTS_FAIL, ST_IPA_FAIL, ST_LA_FAIL, ST_NUMA_FAIL,
                    ST_DEVICE_FAIL, ST_RESV_FAIL)
DIAG_EXT_POD_TILE = 32  # pods per workgroup of koordhip_diagnose_ext's kernel (diag_ext.hip DIAGX_PT)
# FitError reasons (KOORDHIP_REASON_*, include/koordhip.h): bit indices of a node's 32-bit reason mask
(REASON_STATIC, REASON_FIT_PODS, REASON_FIT_CPU, REASON_FIT_MEM, REASON_FIT_EPH, REASON_FIT_BCPU, REASON_FIT_BMEM,
 REASON_LA_USAGE, REASON_NUMA_POD_ERROR, REASON_NUMA_AMP_CPU, REASON_NUMA_NO_TOPOLOGY, REASON_NUMA_SMT_ALIGN,
 REASON_NUMA_FULL_PCPUS_ONLY, REASON_NUMA_CPUS, REASON_NUMA_REQUIRED_POLICY, REASON_NUMA_NO_ZONES, REASON_NUMA_POLICY,
 REASON_RESV_AFFINITY, REASON_RESV_INSUFFICIENT) = range(19)
REASON_COUNT, REASON_SLOTS = 19, 32
# the reasons of each status bit: a status bit is set iff one of its reasons is
REASONS_OF_BIT = {
    ST_STATIC_FAIL: 0x00000001,
    ST_FIT_FAIL: 0x0000007E,
    ST_LA_FAIL: 0x00000080,
    ST_NUMA_FAIL: 0x0001FF00,
    ST_RESV_FAIL: 0x00060000,
}
REASON_UNRESOLVABLE_MASK = 0x00029C01   # the UnschedulableAndUnresolvable reasons
REASON_ERROR_MASK = 0x00000100          # the Error reason (NUMA_POD_ERROR)
# ... and the sequential cycle's (koordhip_diagnose_reasons_ext): REASON_FIT_X0 + j is extended scalar j
# (deviceshare.XRES[j]); the other five are one slot each
REASON_FIT_X0 = 19
(REASON_DEVICE_INSUFFICIENT, REASON_PTS_MISSING_LABEL, REASON_PTS_SKEW, REASON_IPA_AFFINITY,
 REASON_IPA_ANTI) = range(27, 32)
REASON_EXT_COUNT = 32
# Slot order is not Filter order here (XFIT, PTS and IPA precede LoadAware): nine groups, walked in
# FILTER_ORDER_EXT with FIT and XFIT as the one plugin they are
REASONS_OF_BIT_EXT = dict(REASONS_OF_BIT)
REASONS_OF_BIT_EXT.update({
    ST_XFIT_FAIL: 0x07F80000,
    ST_DEVICE_FAIL: 0x08000000,
    ST_PTS_FAIL: 0x30000000,
    ST_IPA_FAIL: 0xC0000000,
})
REASON_EXT_UNRESOLVABLE_MASK = 0x50029C01   # + PTS_MISSING_LABEL, IPA_AFFINITY
# numpy twin of koordhip_reasons (264 bytes)
REASONS_DTYPE = np.dtype([("feasible", "<i4"), ("unresolvable", "<i4"), ("first", "<i4", (REASON_SLOTS,)),
                          ("any", "<i4", (REASON_SLOTS,))])
assert REASONS_DTYPE.itemsize == 264


def reasons_status(mask):
    """The KOORDHIP_ST_* bits a reason mask (int or array) stands for."""
    st = 0
    for bit, group in REASONS_OF_BIT.items():
        st = st | np.where((np.asarray(mask, np.uint32) & np.uint32(group)) != 0, np.uint32(bit), np.uint32(0))
    return st


def first_reasons(mask):
    """The reasons of the first failing plugin (FILTER_ORDER) of a reason mask (int or array)."""
    m = np.asarray(mask, np.uint32)
    out = np.zeros_like(m)
    done = np.zeros(m.shape, bool)
    for bit in FILTER_ORDER:
        g = m & np.uint32(REASONS_OF_BIT[bit])
        take = ~done & (g != 0)
        out = np.where(take, g, out)
        done |= take
    return out


def reasons_status_ext(mask):
    """reasons_status() over all 32 slots: the 16-bit KOORDHIP_ST_* word (koordhip_node_status_ext's)."""
    st = 0
    for bit, group in REASONS_OF_BIT_EXT.items():
        st = st | np.where((np.asarray(mask, np.uint32) & np.uint32(group)) != 0, np.uint32(bit), np.uint32(0))
    return st


def first_reasons_ext(mask):
    """first_reasons() in FILTER_ORDER_EXT: NodeResourcesFit's FIT_* and FIT_X* reasons are one group."""
    m = np.asarray(mask, np.uint32)
    out = np.zeros_like(m)
    done = np.zeros(m.shape, bool)
    fit = REASONS_OF_BIT_EXT[ST_FIT_FAIL] | REASONS_OF_BIT_EXT[ST_XFIT_FAIL]
    for bit in FILTER_ORDER_EXT:
        if bit == ST_XFIT_FAIL:
            continue
        g = m & np.uint32(fit if bit == ST_FIT_FAIL else REASONS_OF_BIT_EXT[bit])
        take = ~done & (g != 0)
        out = np.where(take, g, out)
        done |= take
    return out


# the preemption dry run (koordhip_preempt*): numpy twins of koordhip_assigned (160 bytes),
# koordhip_preemptor (208), koordhip_preempt_node (32) and koordhip_preempt_result (56)
PREEMPT_QRES, PREEMPT_PDBS, PREEMPT_NODE_PODS = 4, 8, 128
ASG_NONPREEMPTIBLE, ASG_IN_QUOTA = 1, 2
ASG_RESV_SLOT_SHIFT, ASG_RESV_SLOT_MASK = 8, 15 << 8   # flags bits 8-11: slot + 1 of the node's reservation the pod is bound to


def asg_resv_slot(q: int) -> int:
    """KOORDHIP_ASG_RESV_SLOT(q): the koordhip_assigned.flags field of a pod bound to reservation slot q of its node."""
    return (q + 1) << ASG_RESV_SLOT_SHIFT


PREEMPT_CANDIDATE, PREEMPT_NO_VICTIMS, PREEMPT_UNFIT, PREEMPT_ERROR, PREEMPT_UNRESOLVABLE = range(5)
PREEMPT_STATUSES = 5
PREEMPT_NUMA_FROZEN = 1   # koordhip_preempt_set_mode: NodeNUMAResource in the Filter, its verdict frozen for the call
PREEMPT_RESV = 2          # ... Reservation state: the walk keeps the plugin's AddPod / RemovePod state
PREEMPT_DEVICE = 4        # ... DeviceShare: the victims' extended scalars and devices move in the walk
PREEMPT_DEVICE_RESV = 8   # ... both states together: only with RESV | DEVICE, on a profile that has both plugins
ASSIGNED_DTYPE = np.dtype([
    ("pod", POD_DTYPE), ("node", "<i4"), ("priority", "<i4"), ("start_time", "<i8"), ("quota", "<i4"),
    ("flags", "<u4"), ("pdb_mask", "<u4"), ("reserved", "<u4"), ("qreq", "<i8", (PREEMPT_QRES,)),
], align=True)
PREEMPTOR_DTYPE = np.dtype([
    ("pod", POD_DTYPE), ("priority", "<i4"), ("quota", "<i4"), ("q_used", "<i8", (PREEMPT_QRES,)),
    ("q_runtime", "<i8", (PREEMPT_QRES,)), ("q_req", "<i8", (PREEMPT_QRES,)), ("q_mask", "<u4"), ("reserved", "<u4"),
], align=True)
PREEMPT_NODE_DTYPE = np.dtype([
    ("status", "<i4"), ("n_victims", "<i4"), ("n_pdb_violations", "<i4"), ("top_priority", "<i4"),
    ("sum_priority", "<i8"), ("earliest_start", "<i8"),
], align=True)
PREEMPT_RESULT_DTYPE = np.dtype([("node", "<i4"), ("count", "<i4", (PREEMPT_STATUSES,)), ("best", PREEMPT_NODE_DTYPE)],
                                align=True)
assert (ASSIGNED_DTYPE.itemsize, PREEMPTOR_DTYPE.itemsize, PREEMPT_NODE_DTYPE.itemsize,
        PREEMPT_RESULT_DTYPE.itemsize) == (160, 208, 32, 56)
# koordhip_assigned_ext (160 bytes), one per ASSIGNED_DTYPE record: the extended scalars and devices a listed pod holds
ASSIGNED_EXT_DTYPE = np.dtype([
    ("xreq", "<i8", (NXRES,)), ("dev_per", "<i8", (DEV_TYPES, DEV_RES)), ("dev_slots", "<u4", (DEV_TYPES,)),
    ("xmask", "<u4"), ("reserved", "<u8"),
], align=True)
assert ASSIGNED_EXT_DTYPE.itemsize == 160
# koordhip_preempt_stream_stats (24 bytes) of the sequential dry run
PREEMPT_STREAM_STATS_DTYPE = np.dtype([("full_recomputes", "<i8"), ("block_recomputes", "<i8"), ("blocks_skipped", "<i8")],
                                      align=True)
assert PREEMPT_STREAM_STATS_DTYPE.itemsize == 24
# numpy twin of koordhip_pod_ext (176 bytes)
POD_EXT_DTYPE = np.dtype([
    ("dev_req", "<i8", (DEV_TYPES, DEV_RES)),
    ("xreq", "<i8", (NXRES,)),
    ("flags", "<u4"),
    ("xmask", "<u4"),
    ("pts_n", "u1"),
    ("pts_class", "u1"),
    ("pts_match", "u1"),
    ("pts_pad", "u1"),
    ("pts_c", "u1", (PTS_POD,)),
    ("pts_fl", "u1", (PTS_POD,)),
    ("pts_skew", "<i4", (PTS_POD,)),
    ("reserve_node", "<i4"),
    ("ipa_inc", "<u4"),
    ("ipa_aff", "<u4"),
    ("ipa_anti", "<u4"),
    ("ipa_score", "<u4"),
    ("ipa_flags", "<u4"),
    ("ipa_reserved", "<i4"),
    ("ipa_w", "<i4", (IPA_ENTRIES,)),
], align=True)
assert POD_EXT_DTYPE.itemsize == 328


def pod_ext_array(n: int) -> np.ndarray:
    """n koordhip_pod_ext records with no device request (dev_req -1 / 0)."""
    a = np.zeros(n, POD_EXT_DTYPE)
    a["dev_req"][:, DEV_GPU, :] = -1
    return a

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libkoordhip.so")


class KoordhipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"koordhip error {code}: {msg}")
        self.code = code


_lib = None
# additive to ABI 15 (no version bump): a build without them still loads
ADDITIVE_SYMBOLS = ("koordhip_diagnose_ext", "koordhip_node_status_ext", "koordhip_diagnose_reasons",
                    "koordhip_node_reasons", "koordhip_fetch_reasons", "koordhip_fetch_node_reasons",
                    "koordhip_diagnose_reasons_ext", "koordhip_node_reasons_ext", "koordhip_preempt_set_mode",
                    "koordhip_preempt_load_pods_ext", "koordhip_preempt_ext", "koordhip_preempt_node_verdicts_ext",
                    "koordhip_preempt_stream_ext", "koordhip_preempt_stream_resv")


def load_library(path: str = LIB_PATH):
    """Load libkoordhip.so.  Fails loudly when it has not been built.

    KOORDHIP_LIB names another build of the same library (A/B of compile-time
    variants, e.g. `make VARIANT=...`); it must still be a libkoordhip build."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("KOORDHIP_LIB", path)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
                           " (there is no CPU fallback)")
    lib = C.CDLL(path)
    vp = C.c_void_p
    sig = {
        "koordhip_last_error": (C.c_char_p, []),
        "koordhip_abi_version": (C.c_int, []),
        "koordhip_create": (C.c_int, [C.POINTER(KoordhipConfig), C.POINTER(vp)]),
        "koordhip_destroy": (C.c_int, [vp]),
        "koordhip_load_snapshot": (C.c_int, [vp, C.POINTER(KoordhipNodeSoa), C.c_int32]),
        "koordhip_update_nodes": (C.c_int, [vp, _i32p, C.POINTER(KoordhipNodeSoa), C.c_int32]),
        "koordhip_read_nodes": (C.c_int, [vp, _i64p, _i64p, _i32p, _i64p, _i64p]),
        "koordhip_eval": (C.c_int, [vp, vp, C.c_int32, _u8p, _i32p, vp, C.c_int32]),
        "koordhip_place_stream": (C.c_int, [vp, vp, C.c_int32, _i32p]),
        "koordhip_place_stream_ext": (C.c_int, [vp, vp, vp, C.c_int32, _i32p]),
        "koordhip_eval_ext": (C.c_int, [vp, vp, vp, C.c_int32, C.POINTER(C.c_uint16), _i32p, vp, C.c_int32]),
        "koordhip_fetch_devices": (C.c_int, [vp, C.POINTER(C.c_uint32), C.c_int32]),
        "koordhip_read_devices": (C.c_int, [vp, _i64p, _i64p]),
        "koordhip_read_pts": (C.c_int, [vp, _i32p]),
        "koordhip_read_ipa": (C.c_int, [vp, _i32p]),
        "koordhip_stage_pods": (C.c_int, [vp, vp, C.c_int32]),
        "koordhip_stage_pods_ext": (C.c_int, [vp, vp, vp, C.c_int32]),
        "koordhip_place_staged": (C.c_int, [vp]),
        "koordhip_fetch_placements": (C.c_int, [vp, _i32p, C.c_int32]),
        "koordhip_synchronize": (C.c_int, [vp]),
        "koordhip_checkpoint": (C.c_int, [vp]),
        "koordhip_restore": (C.c_int, [vp]),
        "koordhip_commit": (C.c_int, [vp, vp, C.c_int32, _u64p]),
        "koordhip_uncommit": (C.c_int, [vp, vp, C.c_int32, _u64p]),
        "koordhip_commit_ext": (C.c_int, [vp, vp, vp, C.c_int32, _u64p, C.POINTER(C.c_uint32)]),
        "koordhip_uncommit_ext": (C.c_int, [vp, vp, vp, C.c_int32, _u64p, C.POINTER(C.c_uint32)]),
        "koordhip_fetch_cpusets": (C.c_int, [vp, _u64p, C.c_int32]),
        "koordhip_diagnose": (C.c_int, [vp, vp, C.c_int32, vp]),
        "koordhip_fetch_diagnosis": (C.c_int, [vp, vp, C.c_int32]),
        "koordhip_fetch_node_status": (C.c_int, [vp, C.c_int32, _u8p]),
        "koordhip_diagnose_ext": (C.c_int, [vp, vp, vp, C.c_int32, vp]),
        "koordhip_node_status_ext": (C.c_int, [vp, vp, vp, C.POINTER(C.c_uint16)]),
        "koordhip_diagnose_reasons": (C.c_int, [vp, vp, C.c_int32, vp]),
        "koordhip_node_reasons": (C.c_int, [vp, vp, C.POINTER(C.c_uint32)]),
        "koordhip_fetch_reasons": (C.c_int, [vp, vp, C.c_int32]),
        "koordhip_fetch_node_reasons": (C.c_int, [vp, C.c_int32, C.POINTER(C.c_uint32)]),
        "koordhip_diagnose_reasons_ext": (C.c_int, [vp, vp, vp, C.c_int32, vp]),
        "koordhip_node_reasons_ext": (C.c_int, [vp, vp, vp, C.POINTER(C.c_uint32)]),
        "koordhip_preempt_load_pods": (C.c_int, [vp, vp, C.c_int32, _i32p, C.c_int32]),
        "koordhip_preempt": (C.c_int, [vp, vp, C.c_int32, vp, _i32p, C.c_int32]),
        "koordhip_preempt_node_verdicts": (C.c_int, [vp, vp, vp]),
        "koordhip_preempt_stream": (C.c_int, [vp, vp, C.c_int32, vp, _i32p, C.c_int32, vp]),
        "koordhip_preempt_set_mode": (C.c_int, [vp, C.c_uint32]),
        "koordhip_preempt_load_pods_ext": (C.c_int, [vp, vp, vp, C.c_int32, _i32p, C.c_int32]),
        "koordhip_preempt_ext": (C.c_int, [vp, vp, vp, C.c_int32, vp, _i32p, C.c_int32]),
        "koordhip_preempt_node_verdicts_ext": (C.c_int, [vp, vp, vp, vp]),
        "koordhip_preempt_stream_ext": (C.c_int, [vp, vp, vp, C.c_int32, vp, _i32p, C.c_int32, vp]),
        "koordhip_preempt_stream_resv": (C.c_int, [vp, vp, C.c_int32, vp, _i32p, C.c_int32, vp]),
        "koordhip_read_numa": (C.c_int, [vp, _u64p, _u64p, _u64p, _i32p]),
        "koordhip_read_numa_zones": (C.c_int, [vp, _i64p]),
        "koordhip_read_reservations": (C.c_int, [vp, _i64p, _i32p]),
        "koordhip_read_resv_cpus": (C.c_int, [vp, _u64p]),
        "koordhip_read_resv_devices": (C.c_int, [vp, _i64p]),
        "koordhip_read_resv_scalars": (C.c_int, [vp, _i64p]),
        "koordhip_last_stats": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
        "koordhip_last_kernel_stats": (C.c_int, [vp, C.POINTER(KoordhipKernelStats)]),
        "koordhip_set_profile_kernels": (C.c_int, [vp, C.c_int32]),
        "koordhip_last_kernel_names": (C.c_int, [vp, C.c_char_p, C.c_char_p, C.c_int32]),
        "koordhip_comm_unique_id": (C.c_int, [C.c_char_p]),
        "koordhip_comm_init": (C.c_int, [vp, C.c_char_p, C.c_int32, C.c_int32]),
        "koordhip_comm_init_local": (C.c_int, [C.POINTER(vp), C.c_int32]),
    }
    for name, (res, args) in sig.items():
        if name in ADDITIVE_SYMBOLS and not hasattr(lib, name):
            continue    # an older ABI 15 build (KOORDHIP_LIB): the call is detected by its symbol
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    if lib.koordhip_abi_version() != KOORDHIP_ABI_VERSION:
        raise RuntimeError("libkoordhip.so ABI version mismatch; rebuild")
    _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "koordhip_last_error", "koordhip_abi_version", "koordhip_create", "koordhip_destroy",
    "koordhip_load_snapshot", "koordhip_update_nodes", "koordhip_read_nodes", "koordhip_eval",
    "koordhip_place_stream", "koordhip_place_stream_ext", "koordhip_eval_ext", "koordhip_fetch_devices",
    "koordhip_read_devices", "koordhip_read_pts", "koordhip_read_ipa", "koordhip_stage_pods", "koordhip_stage_pods_ext", "koordhip_place_staged", "koordhip_fetch_placements",
    "koordhip_synchronize", "koordhip_checkpoint", "koordhip_restore", "koordhip_commit", "koordhip_uncommit",
    "koordhip_commit_ext", "koordhip_uncommit_ext",
    "koordhip_diagnose", "koordhip_fetch_diagnosis", "koordhip_fetch_node_status",
    "koordhip_diagnose_ext", "koordhip_node_status_ext",
    "koordhip_diagnose_reasons", "koordhip_node_reasons", "koordhip_fetch_reasons", "koordhip_fetch_node_reasons",
    "koordhip_diagnose_reasons_ext", "koordhip_node_reasons_ext",
    "koordhip_preempt_load_pods", "koordhip_preempt", "koordhip_preempt_node_verdicts",
    "koordhip_preempt_stream", "koordhip_preempt_set_mode",
    "koordhip_preempt_load_pods_ext", "koordhip_preempt_ext", "koordhip_preempt_node_verdicts_ext",
    "koordhip_preempt_stream_ext", "koordhip_preempt_stream_resv",
    "koordhip_fetch_cpusets", "koordhip_read_numa", "koordhip_read_numa_zones", "koordhip_read_reservations",
    "koordhip_read_resv_cpus", "koordhip_read_resv_devices", "koordhip_read_resv_scalars", "koordhip_last_stats", "koordhip_last_kernel_stats",
    "koordhip_set_profile_kernels", "koordhip_last_kernel_names",
    "koordhip_comm_unique_id", "koordhip_comm_init", "koordhip_comm_init_local",
]


def check(lib, rc: int):
    if rc != 0:
        raise KoordhipError(rc, (lib.koordhip_last_error() or b"").decode())
    return rc


def ptr(a: np.ndarray, ctype):
    return a.ctypes.data_as(C.POINTER(ctype)) if a is not None else None
