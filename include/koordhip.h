/*
 * koordhip.h -- C-ABI of libkoordhip.so, the MI355X batched placement engine
 * for koord-scheduler's Filter/Score hot path (NodeResourcesFit,
 * LoadAwareScheduling, NodeNUMAResource) plus argmax and the Reserve delta.
 *
 * Plain C, no torch / HIP types in any signature: a Go host binds it with cgo
 * (see INTEGRATION.md), Python with ctypes.  Every function returns 0 on
 * success and a negative KOORDHIP_E* code on error; the message of the last
 * error on the calling thread is returned by koordhip_last_error().
 *
 * Reference interfaces each entry point replaces (paths relative to the
 * koordinator tree, "(upstream)" = k8s.io/kubernetes v1.24.15):
 *   koordhip_create         <- loadaware.New            pkg/scheduler/plugins/loadaware/load_aware.go:76-110
 *                              nodenumaresource.New     pkg/scheduler/plugins/nodenumaresource/plugin.go:101-151
 *                              (upstream) noderesources.NewFit + args from config/manager/scheduler-config.yaml:17-46
 *   koordhip_load_snapshot  <- the per-cycle NodeInfo snapshot + NodeMetric lister reads
 *                              load_aware.go:133,270-278; (upstream) Snapshot.NodeInfos()
 *   koordhip_update_nodes   <- informer deltas: podAssignCache.OnAdd/OnUpdate/OnDelete pod_assign_cache.go:82-117,
 *                              NodeMetric informer (load_aware.go:114-121)
 *   koordhip_eval           <- Filter  load_aware.go:123-171, (upstream) fit.go Filter/fitsRequest,
 *                              Score   load_aware.go:269-335, (upstream) resource_allocation.go score,
 *                              called per (pod,node) by frameworkext/framework_extender.go:192-238
 *   koordhip_place_stream   <- (upstream) schedule_one.go scheduleOne: findNodesThatFitPod ->
 *                              prioritizeNodes -> selectHost (tie -> lowest node index) -> Reserve
 *   koordhip_commit         <- Reserve  load_aware.go:260-263 (podAssignCache.assign, pod_assign_cache.go:53-68),
 *                              (upstream) cache.AssumePod -> NodeInfo.AddPod
 *   koordhip_uncommit       <- Unreserve load_aware.go:265-267 (pod_assign_cache.go:70-80)
 *   koordhip_commit_ext / koordhip_uncommit_ext
 *                           <- the same plus DeviceShare Reserve / Unreserve deviceshare/plugin.go:368-426 and the
 *                              (upstream) PodTopologySpread / InterPodAffinity AddPod / RemovePod of the pod
 *   reservation columns     <- Reservation BeforePreFilter restore reservation/transformer.go:48-293,
 *                              filterWithReservations plugin.go:373-494, PreScore/Score scoring.go:42-200,
 *                              NominateReservation nominator.go:32-85, Reserve -> reservationCache.assumePod
 *                              plugin.go:537-575 / cache.go:170-191
 *   resv_cpus columns       <- NodeNUMAResource RestoreReservation nodenumaresource/reservation.go:68-122 and the
 *                              reservation-preferred CPUs of getResourceOptions plugin.go:455-524 (Score / Reserve)
 *   dev_* columns, koordhip_pod_ext
 *                           <- DeviceShare PreFilter plugin.go:146-182, Filter :284-323, Score scoring.go:33-80,
 *                              Reserve plugin.go:368-405 over nodeDevice (device_cache.go:44-482) and the
 *                              default allocator (allocator.go:91-122)
 *   static_score columns    <- (upstream) NodeAffinity / TaintToleration Score + NormalizeScore
 *   koordhip_diagnose / koordhip_fetch_diagnosis / koordhip_fetch_node_status /
 *   koordhip_diagnose_ext / koordhip_node_status_ext
 *                           <- the Filter half of a failed cycle: framework.Diagnosis{NodeToStatusMap,
 *                              UnschedulablePlugins} of the FitError ((upstream) schedule_one.go findNodesThatFitPod),
 *                              read by frameworkext/eventhandlers/reservation_handler.go:92-94 and handed to every
 *                              PostFilter (elasticquota/plugin.go:310, reservation/plugin.go:496,
 *                              coscheduling/core/core.go:289-293)
 *   koordhip_diagnose_reasons / koordhip_node_reasons / koordhip_fetch_reasons / koordhip_fetch_node_reasons /
 *   koordhip_diagnose_reasons_ext / koordhip_node_reasons_ext
 *                           <- the Status reason and code behind each of those nodes: fitsRequest's
 *                              InsufficientResource list ((upstream) fit.go), nodenumaresource/plugin.go:266-363 and
 *                              resource_manager.go:244-326,442-453, reservation/plugin.go:373-440,
 *                              deviceshare/plugin.go:322 and reservation.go:280, (upstream) podtopologyspread and
 *                              interpodaffinity filtering.go; what FitError.Error() prints and
 *                              nodesWherePreemptionMightHelp drops
 *   koordhip_place_stream_ext / koordhip_eval_ext
 *                           <- the exact sequential cycle for profiles with plugins whose scores are normalized
 *                              over the feasible nodes (DefaultNormalizeScore, upstream helper/normalize_score.go)
 */
#ifndef KOORDHIP_H
#define KOORDHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KOORDHIP_ABI_VERSION 15

/* ---- error codes ------------------------------------------------------- */
#define KOORDHIP_OK 0
#define KOORDHIP_EINVAL (-1)   /* bad argument / config (validation_pluginargs.go:31-95 analogue) */
#define KOORDHIP_EDEVICE (-2)  /* HIP runtime error */
#define KOORDHIP_ESTATE (-3)   /* call out of order (e.g. eval before load_snapshot) */
#define KOORDHIP_ENOMEM (-4)
#define KOORDHIP_ECOMM (-5)    /* RCCL error */
#define KOORDHIP_ERESERVE (-6) /* a Reserve plugin failed (NodeNUMAResource Allocate, plugin.go:398-401) */

/* ---- plugins ------------------------------------------------------------ */
#define KOORDHIP_PLUGIN_FIT 1u        /* NodeResourcesFit (upstream) */
#define KOORDHIP_PLUGIN_LOADAWARE 2u  /* LoadAwareScheduling */
#define KOORDHIP_PLUGIN_NUMA 4u       /* NodeNUMAResource */
#define KOORDHIP_PLUGIN_RESERVATION 8u /* Reservation (restore + filterWithReservations + Score, weight
                                          koordhip_config.reservation_weight) */
/* Upstream default-profile plugins (k8s v1.24.15, un-vendored: SURVEY.md
 * section 8(f)#4; restated in DESIGN.md, parity unpinned by reference tests): */
#define KOORDHIP_PLUGIN_NODE_STATIC 16u /* Filter: NodeUnschedulable + NodeAffinity (nodeSelector +
                                           requiredDuringScheduling) + TaintToleration (NoSchedule /
                                           NoExecute), resolved per (pod static class, node) by the host
                                           into koordhip_node_soa.static_allow */
#define KOORDHIP_PLUGIN_BALANCED 32u    /* Score: NodeResourcesBalancedAllocation (cpu + memory,
                                           Requested + the pod request, 1 - |f_cpu - f_mem| / 2) */
#define KOORDHIP_NPLUGINS 4             /* plugins with a per-node score in koordhip_eval's scores:
                                           Fit, LoadAware, NUMA, BalancedAllocation */
/* Plugins whose Score is normalized over the pod's feasible nodes
 * (DefaultNormalizeScore(100, reverse)): a profile enabling any of them places
 * through the exact sequential cycle (koordhip_place_stream_ext).
 * Their raw scores are planes KOORDHIP_NPLUGINS.. of koordhip_eval_ext. */
#define KOORDHIP_PLUGIN_DEVICESHARE 64u      /* DeviceShare Filter / Score / Reserve (koordhip_pod_ext, dev_* columns) */
#define KOORDHIP_PLUGIN_AFFINITY_SCORE 128u  /* NodeAffinity Score: preferred terms (static_score[0]) */
#define KOORDHIP_PLUGIN_TAINT_SCORE 256u     /* TaintToleration Score: intolerable PreferNoSchedule taints
                                                (static_score[1], normalized reversed) */
#define KOORDHIP_PLUGIN_PTS 512u             /* PodTopologySpread Filter (DoNotSchedule constraints) and Score
                                                (ScheduleAnyway constraints, weight ext_weight[3]; its own
                                                min-max NormalizeScore); pts_* columns, koordhip_pod_ext.pts_* */
#define KOORDHIP_PLUGIN_IPA 1024u            /* InterPodAffinity Filter (required affinity / anti-affinity, the
                                                existing pods' required anti-affinity) and Score (preferred terms,
                                                the existing pods' terms; weight ext_weight[4]; its own min-max
                                                NormalizeScore); ipa_* columns, koordhip_pod_ext.ipa_* */
#define KOORDHIP_NEXT_PLUGINS 5              /* DeviceShare, NodeAffinity, TaintToleration, PodTopologySpread,
                                                InterPodAffinity */
/* PodTopologySpread envelope (k8s v1.24 podtopologyspread, not vendored): */
#define KOORDHIP_PTS_KEYS 4      /* distinct topology keys of the snapshot's constraints */
#define KOORDHIP_PTS_DOMAINS 64  /* values of a non-hostname key */
#define KOORDHIP_PTS_CONS 8      /* distinct (label selector, namespace) of the snapshot's constraints */
#define KOORDHIP_PTS_CLASSES 8   /* spread classes: (required node affinity, hard keys, soft keys) */
#define KOORDHIP_PTS_POD 4       /* constraints per pod */
/* InterPodAffinity envelope (k8s v1.24 interpodaffinity, not vendored): the
 * topology keys are the pts_* keys (shared with PodTopologySpread) */
#define KOORDHIP_IPA_ENTRIES 32  /* count entries of the snapshot (ipa_cnt rows) */
/* NodeResourcesFit's extended scalar resources of device pods (koordinator.sh/
 * gpu-core, gpu-memory-ratio, gpu-memory, nvidia.com/gpu, ...): fitsRequest
 * checks each one the pod requests against Allocatable - Requested (upstream
 * fit.go); koordhip_pod_ext.xreq / koordhip_node_soa.xalloc, xrequested */
#define KOORDHIP_NXRES 8
#define KOORDHIP_MAX_STATIC_CLASSES 32  /* distinct pod static classes (koordhip_pod.static_class) */

/* Fit resource slots (ResourceSpec names in scheduler-config.yaml:21-31). */
#define KOORDHIP_RES_CPU 0   /* "cpu", milli-CPU */
#define KOORDHIP_RES_MEM 1   /* "memory", bytes */
#define KOORDHIP_RES_EPH 2   /* "ephemeral-storage", bytes */
#define KOORDHIP_RES_BCPU 3  /* "kubernetes.io/batch-cpu", Value() */
#define KOORDHIP_RES_BMEM 4  /* "kubernetes.io/batch-memory", bytes */
#define KOORDHIP_NRES 5

/* Per-node LoadAware snapshot flags (koordhip_node_soa.la_flags), resolved by the
 * marshaller at snapshot time T0 (wall-clock predicates are never re-read). */
#define KOORDHIP_LA_HAS_METRIC 1u        /* nodeMetricLister.Get found (load_aware.go:133-142,278-286) */
#define KOORDHIP_LA_FILTER_SKIP 2u       /* FilterExpiredNodeMetrics && expired (load_aware.go:144-147) */
#define KOORDHIP_LA_SCORE_EXPIRED 4u     /* isNodeMetricExpired(NodeMetricExpirationSeconds) (load_aware.go:287-289) */
#define KOORDHIP_LA_FILTER_USAGE 8u      /* Status.NodeMetric != nil and the filter's usage source non-nil (load_aware.go:174-211) */
#define KOORDHIP_LA_PROD_MODE 16u        /* len(ProdUsageThresholds) > 0 (load_aware.go:150) */
#define KOORDHIP_LA_HAS_PODS_METRIC 32u  /* len(Status.PodsMetric) > 0 (load_aware.go:227-229) */
#define KOORDHIP_LA_AGGREGATED 64u       /* filter uses aggregated usage (status reason only) */

/* Per-pod flags (koordhip_pod.flags), computed once per pod by the host
 * (PreFilter analogue). */
#define KOORDHIP_POD_PROD 1u          /* GetPodPriorityClassWithDefault == koord-prod (priority_utils.go:26-34) */
#define KOORDHIP_POD_DAEMONSET 2u     /* isDaemonSetPod (helper.go:188-196) */
#define KOORDHIP_POD_HAS_REQ 4u       /* request not all-zero / scalar map non-empty (upstream fitsRequest) */
#define KOORDHIP_POD_REQ_BCPU 8u      /* batch-cpu key present in the pod request map */
#define KOORDHIP_POD_REQ_BMEM 16u     /* batch-memory key present in the pod request map */
#define KOORDHIP_POD_CPUSET 32u       /* NUMA: requestCPUBind (plugin.go:230-245) */
#define KOORDHIP_POD_NUMA_SKIP 64u    /* NUMA: PreFilter skip (zero request) (plugin.go:218-226) */
#define KOORDHIP_POD_NUMA_ERROR 128u  /* NUMA: PreFilter error (non-integral cpuset request, plugin.go:242-245) */
#define KOORDHIP_POD_KEY_CPU 256u     /* "cpu" key present in PodRequestsAndLimits (Reservation nominate / score / Restricted) */
#define KOORDHIP_POD_KEY_MEM 512u     /* "memory" key present */
#define KOORDHIP_POD_RESERVE 2048u    /* a reserve pod (IsReservePod, util/reservation): the Reservation Filter checks
                                         its reservation's nodeName (koordhip_pod_ext.reserve_node) and AllocatePolicy
                                         against the node's Available reservations (plugin.go:326-362), no reservation
                                         matches it (transformer.go:60,96; resv_match must be 0), its Reservation
                                         Score is 0 (scoring.go:127-130) and its Reserve assumes a reservation that is
                                         not Available yet (no slot, plugin.go:538-548).  A batch holding one runs in
                                         the sequential cycle (ABI 11) */
#define KOORDHIP_POD_RESERVE_POLICY_SHIFT 12  /* bits 12-13: the reserve pod's AllocatePolicy (KOORDHIP_RESV_POLICY codes) */
#define KOORDHIP_POD_RESV_OPERATING 16384u /* a pod in the reservation operating mode (IsReservationOperatingMode,
                                              apis/extension/operating_pod.go:51-53): the Reservation Filter checks
                                              AllocatePolicy Aligned (bits 12-13 = 1) against the node's Available
                                              reservations (plugin.go:332-357), then filterWithReservations as for
                                              any pod; a batch holding one runs in the sequential cycle (ABI 11) */
#define KOORDHIP_POD_RESERVE_POLICY(f) (((f) >> KOORDHIP_POD_RESERVE_POLICY_SHIFT) & 3u)
#define KOORDHIP_POD_CPUSET_QOS 32768u /* ABI 12: AllowUseCPUSet (nodenumaresource/util.go:42-49: koord-prod and
                                          QoS LSE / LSR) -- such a pod gets the nominated reservation's reserved
                                          CPUs restored (reservation.go:68-74) even when it binds none; on
                                          topology-policy or CPU-amplified nodes that changes its zone / amplified
                                          Score and Reserve (plugin.go:465-479), which the engine does not model
                                          for non-binding pods: such a batch is refused (KOORDHIP_EINVAL) on a
                                          snapshot with reservations holding CPUs on such nodes */
#define KOORDHIP_POD_RESV_AFFINITY 1024u /* a required reservation affinity (util/reservation/reservation.go:444-487): a node
                                            without a matched reservation fails the Reservation Filter (plugin.go:378-381) */

/* koordhip_node_soa.resv_flags: a node's Available reservations, one per slot
 * (koordhip_node_soa.resv_slots).  The reference keeps them in a map
 * (cache.go:236-252: forEachAvailableReservationOnNode iterates in Go map
 * order) and its nomination ties (findMostPreferredReservationByOrder's first
 * smallest order, nominator.go:60; sort.Slice by score, nominator.go:69-71)
 * follow that order: here they go to the lowest slot.  0 = empty slot. */
#define KOORDHIP_RESV_PRESENT 1u       /* IsAvailable && ParseError == nil (transformer.go:87-89) */
#define KOORDHIP_RESV_ALLOCATE_ONCE 2u /* IsReservationAllocateOnce (apis/extension/reservation.go:98-100) */
#define KOORDHIP_RESV_UNSCHEDULABLE 4u /* IsUnschedulable: spec.unschedulable or terminating (reservation_info.go:248-255) */
#define KOORDHIP_RESV_ORDERED 8u       /* label scheduling.koordinator.sh/reservation-order parses to != 0 (scoring.go:156-175) */
#define KOORDHIP_RESV_KEY_CPU 16u      /* "cpu" in ResourceNames (the Allocatable keys, reservation_info.go:80-81) */
#define KOORDHIP_RESV_KEY_MEM 32u      /* "memory" in ResourceNames */
#define KOORDHIP_RESV_POLICY_SHIFT 6   /* bits 6-7 AllocatePolicy: 0 Default, 1 Aligned, 2 Restricted */
#define KOORDHIP_RESV_POLICY(f) (((f) >> KOORDHIP_RESV_POLICY_SHIFT) & 3u)
#define KOORDHIP_RESV_GROUP_SHIFT 8    /* bits 8-13: owner group g, the pod matches iff bit g of koordhip_pod.resv_match */
#define KOORDHIP_RESV_GROUP(f) (((f) >> KOORDHIP_RESV_GROUP_SHIFT) & 63u)
#define KOORDHIP_RESV_MAX_ORDERS 1024  /* distinct reservation-order values (resv_order_rank < this) */
#define KOORDHIP_RESV_SLOTS 4          /* Available reservations per node on the pipelined greedy */
#define KOORDHIP_RESV_SLOTS_MAX 8      /* ... in a snapshot (koordhip_node_soa.resv_slots <= this); a snapshot with
                                          more than KOORDHIP_RESV_SLOTS runs in the sequential cycle (ABI 11) */

/* koordhip_pod.numa_policy, the NUMA PreFilter state (plugin.go:227-255):
 * bits 0-1 requiredCPUBindPolicy, 2-3 preferredCPUBindPolicy (= required when
 * set), 4-5 preferredCPUExclusivePolicy. */
#define KOORDHIP_CPUBIND_NONE 0u
#define KOORDHIP_CPUBIND_FULL_PCPUS 1u
#define KOORDHIP_CPUBIND_SPREAD_BY_PCPUS 2u
#define KOORDHIP_CPUEXCL_NONE 0u
#define KOORDHIP_CPUEXCL_PCPU 1u
#define KOORDHIP_CPUEXCL_NUMA 2u
#define KOORDHIP_NUMA_REQUIRED(p) ((p) & 3u)
#define KOORDHIP_NUMA_PREFERRED(p) (((p) >> 2) & 3u)
#define KOORDHIP_NUMA_EXCLUSIVE(p) (((p) >> 4) & 3u)

/* koordhip_node_soa.numa_flags: node CPU bind policy (GetNodeCPUBindPolicy,
 * apis/extension/numa_aware.go:314-325) and NUMA allocate strategy
 * (GetNUMAAllocateStrategy, nodenumaresource/util.go:34-40). */
#define KOORDHIP_NODE_CPUBIND_MASK 3u   /* 0 None, 1 FullPCPUsOnly, 2 SpreadByPCPUs */
#define KOORDHIP_NODE_NUMA_MOST_ALLOCATED 4u
/* bits 3-4: the node's NUMA topology policy (getNUMATopologyPolicy: label
 * node.koordinator.sh/numa-topology-policy over the NRT's policy,
 * nodenumaresource/util.go; apis/extension/numa_aware.go:56-64) */
#define KOORDHIP_NODE_NUMA_POLICY_SHIFT 3
#define KOORDHIP_NODE_NUMA_POLICY(f) (((f) >> KOORDHIP_NODE_NUMA_POLICY_SHIFT) & 3u)
#define KOORDHIP_NUMA_TOPO_NONE 0u
#define KOORDHIP_NUMA_TOPO_BEST_EFFORT 1u
#define KOORDHIP_NUMA_TOPO_RESTRICTED 2u
#define KOORDHIP_NUMA_TOPO_SINGLE_NUMA_NODE 3u
/* NUMA zones (NRT zones "node-<k>", zone k = NUMA node rank k) of a node with
 * a topology policy: up to this many (hint merge over <= 255 masks per
 * (pod, node), e.g. a 2-socket host in NPS4 mode). */
#define KOORDHIP_NUMA_MAX_ZONES 8

/* CPU topology of a node (cpu_topology.go:25-103), shared by every node of
 * the same shape.  CPU "positions" are core-major: pos = core_rank *
 * cpus_per_core + t, cores in ascending CoreID, t in ascending CPU id, so one
 * bit per position in a 4 x 64-bit mask.  NUMA nodes and sockets are ranked
 * by ascending id.  Every core must hold exactly cpus_per_core CPUs. */
#define KOORDHIP_NUMA_MAX_CPUS 256
#define KOORDHIP_NUMA_MAX_NODES 8
#define KOORDHIP_NUMA_WORDS 4
typedef struct koordhip_numa_class {
  int32_t num_cpus, num_cores, num_nodes, num_sockets; /* CPUTopology counters (builder semantics) */
  int32_t cpus_per_core;
  int32_t reserved0;
  int32_t cpu_id[KOORDHIP_NUMA_MAX_CPUS];       /* pos -> logical CPU id */
  uint8_t node_of[KOORDHIP_NUMA_MAX_CPUS];      /* pos -> NUMA node rank */
  uint8_t socket_of[KOORDHIP_NUMA_MAX_CPUS];    /* pos -> socket rank */
} koordhip_numa_class;

/* Per-(pod,node) status bits written by koordhip_eval (no short-circuit, one
 * bit per plugin that returned non-Success from Filter). */
#define KOORDHIP_ST_FIT_FAIL 1u
#define KOORDHIP_ST_LA_FAIL 2u
#define KOORDHIP_ST_NUMA_FAIL 4u
#define KOORDHIP_ST_RESV_FAIL 8u  /* filterWithReservations (reservation/plugin.go:373-440) */
#define KOORDHIP_ST_STATIC_FAIL 16u /* NodeUnschedulable / NodeAffinity / TaintToleration */
#define KOORDHIP_ST_DEVICE_FAIL 32u /* DeviceShare Filter (plugin.go:284-323) */
#define KOORDHIP_ST_XFIT_FAIL 64u   /* NodeResourcesFit on an extended scalar resource (koordhip_pod_ext.xreq) */
#define KOORDHIP_ST_PTS_FAIL 128u   /* PodTopologySpread Filter (a missing topology key, or the skew) */
#define KOORDHIP_ST_IPA_FAIL 256u   /* InterPodAffinity Filter (koordhip_eval_ext's 16-bit status only) */

/* DeviceShare's device model (nodeDevice, device_cache.go:44-50): per node
 * and device type up to KOORDHIP_DEV_SLOTS minors, each with the Device CR's
 * resources (deviceTotal) and what pods hold (deviceUsed); free = total - used
 * clamped at 0 per resource (resetDeviceFree, :185-202). */
#define KOORDHIP_DEV_TYPES 3  /* 0 gpu, 1 rdma, 2 fpga (DeviceResourceNames, device_resources.go:42-53) */
#define KOORDHIP_DEV_GPU 0
#define KOORDHIP_DEV_RDMA 1
#define KOORDHIP_DEV_FPGA 2
#define KOORDHIP_DEV_SLOTS 8  /* minors per type per node */
#define KOORDHIP_DEV_RES 3    /* gpu: [0] koordinator.sh/gpu-core, [1] gpu-memory-ratio, [2] gpu-memory (bytes);
                                 rdma / fpga: [0] koordinator.sh/rdma | fpga */

/* place_stream out_node values */
#define KOORDHIP_UNSCHEDULABLE (-1)
#define KOORDHIP_RESERVE_FAILED (-2)

typedef struct koordhip_ctx koordhip_ctx;

/* Plugin arguments (pkg/scheduler/apis/config/types.go:29-108, defaults
 * v1beta2/defaults.go:32-121, weights scheduler-config.yaml:82-91). */
typedef struct koordhip_config {
  int32_t abi_version;      /* must be KOORDHIP_ABI_VERSION */
  uint32_t filter_plugins;  /* KOORDHIP_PLUGIN_* bits enabled at Filter */
  uint32_t score_plugins;   /* KOORDHIP_PLUGIN_* bits enabled at Score */
  int32_t device;           /* HIP device ordinal; -1 = current device */
  int64_t plugin_weight[KOORDHIP_NPLUGINS]; /* score weight: Fit, LoadAware, NUMA, BalancedAllocation (1..100) */
  int64_t fit_weight[KOORDHIP_NRES];        /* NodeResourcesFitArgs LeastAllocated weights, 0 = resource not listed */
  int64_t la_weight_cpu;                    /* LoadAwareSchedulingArgs.ResourceWeights[cpu] (1..100) */
  int64_t la_weight_mem;                    /* LoadAwareSchedulingArgs.ResourceWeights[memory] (1..100) */
  int32_t la_score_according_prod_usage;    /* LoadAwareSchedulingArgs.ScoreAccordingProdUsage */
  int32_t batch_pods;       /* pods per pipelined round of place_stream (0 = default: 32, 16 with NodeNUMAResource; max 64) */
  int32_t numa_weight_cpu;  /* NodeNUMAResourceArgs.ScoringStrategy LeastAllocated weights */
  int32_t numa_weight_mem;
  int32_t profile_kernels;  /* 1 = time every stream eval launch with HIP events (koordhip_last_stats) */
  int32_t numa_most_allocated; /* NodeNUMAResourceArgs.ScoringStrategy.Type == MostAllocated
                                  (nodenumaresource/most_allocated.go:30-62); 0 = LeastAllocated */
  int32_t reservation_weight;  /* Reservation score weight (scheduler-config.yaml:90-91: 5000); must exceed
                                  100 x the sum of the other score weights (Reservation key) */
  int32_t reserved[5];
  /* ABI 9: the normalized-score plugins */
  int32_t ext_weight[KOORDHIP_NEXT_PLUGINS]; /* score weights: DeviceShare (scheduler-config.yaml:88-89: 1),
                                               NodeAffinity, TaintToleration, PodTopologySpread,
                                               InterPodAffinity (1..100) */
  int32_t dev_most_allocated;  /* DeviceShareArgs.ScoringStrategy.Type == MostAllocated (scoring.go:125-132) */
  int32_t dev_res_weight[5];   /* DeviceShareArgs.ScoringStrategy.Resources weights (0 = not listed): gpu-core,
                                  gpu-memory-ratio, gpu-memory, rdma, fpga (defaults v1beta2/defaults.go:168-189:
                                  gpu-memory-ratio, rdma, fpga at 1) */
  int32_t reserved2[1];
} koordhip_config;

/* Columnar node snapshot, all arrays of length n, little-endian, caller-owned
 * and copied by koordhip_load_snapshot.  Units: CPU in milli-cores, memory /
 * ephemeral storage in bytes, batch-cpu as Quantity.Value().  Mutable columns
 * (requested / nz / npods / la_used*) are advanced on device by commits.
 * Every resource quantity (alloc, requested, nz_*, la_alloc_*, la_used_*, the
 * NUMA zone and reservation amounts, and koordhip_pod's req / nz_* / est_*)
 * must be in [0, 2^45): load_snapshot, update_nodes and every call taking a
 * pod record refuse any other value with KOORDHIP_EINVAL (the scores of a
 * negative quantity leave [0, 100], the range the engine ranks in). */
typedef struct koordhip_node_soa {
  /* NodeResourcesFit: NodeInfo.Allocatable (upstream framework/types.go) */
  const int64_t *alloc[KOORDHIP_NRES];
  const int32_t *alloc_pods;               /* Allocatable.AllowedPodNumber */
  /* NodeResourcesFit: NodeInfo.Requested, .NonZeroRequested, len(.Pods) */
  const int64_t *requested[KOORDHIP_NRES];
  const int64_t *nz_cpu_m;
  const int64_t *nz_mem;
  const int32_t *npods;
  /* LoadAwareScheduling Score (load_aware.go:269-335) */
  const int64_t *la_alloc_cpu_m;           /* EstimateNode(node)[cpu].MilliValue() (default_estimator.go:110-129) */
  const int64_t *la_alloc_mem;             /* EstimateNode(node)[memory].Value() */
  const int64_t *la_used_cpu_m;            /* assigned-pod estimates + nodeUsage (cond. minus estimated pods' actual) */
  const int64_t *la_used_mem;
  const int64_t *la_used_prod_cpu_m;       /* prod-pod variant (ScoreAccordingProdUsage); may be NULL otherwise */
  const int64_t *la_used_prod_mem;
  /* LoadAwareScheduling Filter inputs (load_aware.go:173-254), milli values */
  const int64_t *laf_used_m[2];            /* nodeUsage (or target aggregated usage) cpu, memory: MilliValue() */
  const int64_t *laf_total_m[2];           /* EstimateNode allocatable cpu, memory: MilliValue() */
  const int64_t *laf_prod_used_m[2];       /* sum of prod pods' usage (buildPodMetricMap+sumPodUsages) */
  const int64_t *laf_thr[2];               /* resolved usage thresholds cpu, memory (0 = disabled) */
  const int64_t *laf_prod_thr[2];          /* resolved prod usage thresholds (0 = disabled) */
  const uint8_t *la_flags;                 /* KOORDHIP_LA_* */
  /* NodeNUMAResource (TopologyOptions + NodeAllocation, topology_options.go:40-48,
   * node_allocation.go:32-38); all NULL / n_numa_classes = 0 when unused */
  const koordhip_numa_class *numa_classes;
  int32_t n_numa_classes;
  int32_t reserved0;
  const int32_t *numa_class;               /* class index, -1 = no (valid) CPU topology */
  const uint64_t *numa_free[KOORDHIP_NUMA_WORDS];      /* available CPUs: all - refcount>=1 - ReservedCPUs (node_allocation.go:133-153) */
  const uint64_t *numa_excl_pcpu[KOORDHIP_NUMA_WORDS]; /* allocated CPUs whose ExclusivePolicy is PCPULevel */
  const uint64_t *numa_excl_numa[KOORDHIP_NUMA_WORDS]; /* allocated CPUs whose ExclusivePolicy is NUMANodeLevel */
  const int32_t *numa_alloc_cnt;           /* |allocatedCPUs| (scoring.go:161-166) */
  const uint8_t *numa_flags;               /* KOORDHIP_NODE_* */
  /* NUMA zone resources, [n][2][KOORDHIP_NUMA_MAX_NODES] row-major, [.][0][k] cpu
   * (milli), [.][1][k] memory (bytes) of zone k: NRT zone allocatable
   * (TopologyOptions.NUMANodeResources, topology_options.go:181-211) and the
   * amounts allocated by pods (NodeAllocation.allocatedResources,
   * node_allocation.go:76-103).  Read only for nodes with a topology policy;
   * NULL when no node has one. */
  const int64_t *numa_zone_alloc;
  const int64_t *numa_zone_used;
  /* CPU amplification ratio of the node (annotation node.koordinator.sh/
   * resource-amplification-ratio, apis/extension/node_resource_amplification.go:
   * 56-76; the same ratio the NodeResourceTopology carries): NodeNUMAResource's
   * filterAmplifiedCPUs / scoreWithAmplifiedCPUs / amplified cpuset requests
   * (plugin.go:326-363, scoring.go:95-168).  NULL or <= 1: not amplified. */
  const double *numa_amp_cpu;
  /* Reservation (KOORDHIP_PLUGIN_RESERVATION): the node's Available reservation,
   * KOORDHIP_RESV_* flags (NULL = no reservations), the rank of its order label
   * among the snapshot's distinct orders (ascending, smaller order = preferred),
   * ReservationInfo.Allocatable / .Allocated (cpu milli, memory bytes; masked to
   * ResourceNames) and len(AssignedPods).  Allocated / assigned are advanced by
   * commits of pods the reservation is nominated for.  resv_nz: the reserve
   * pod's non-zero cpu / memory request (calculateResource, transformer.go:
   * 302-333; Requested of the reserve pod is resv_alloc). */
  const uint32_t *resv_flags;
  const int32_t *resv_order_rank;
  const int64_t *resv_alloc[2];
  const int64_t *resv_nz[2];
  const int64_t *resv_allocated[2];
  const int32_t *resv_assigned;
  /* KOORDHIP_PLUGIN_NODE_STATIC: bit c set = pods of static class c pass
   * NodeUnschedulable, NodeAffinity and TaintToleration's Filter on this node
   * (the node's labels, taints and spec.unschedulable against the class's
   * nodeSelector, required affinity and tolerations); NULL = every class. */
  const uint32_t *static_allow;
  /* Reservation slots per node held by the resv_* columns: 0 or 1 = one
   * reservation per node (columns of n values); S in [2, KOORDHIP_RESV_SLOTS_MAX]
   * = up to S per node (S > KOORDHIP_RESV_SLOTS: the sequential cycle places), every resv_* column then holds S x n values,
   * slot-major (slot s of node i at [s * n + i]); a node's reservations fill
   * its slots from 0, unused slots have resv_flags 0.  koordhip_update_nodes
   * rows use the loaded snapshot's slot count. */
  int32_t resv_slots;
  int32_t reserved1;
  /* NodeNUMAResource's reservation restore (RestoreReservation,
   * nodenumaresource/reservation.go:76-113): per reservation slot, the CPUs of
   * the reservation's cpuset allocation not held by its AssignedPods (core-major
   * positions of the node's topology class, slot-major like the resv_* columns).
   * These CPUs are allocated in the node's NodeAllocation (not in numa_free).  A
   * cpuset pod nominated into the reservation (PreScore) takes them first
   * (takePreferredCPUs, cpu_accumulator.go:29-85) at Score and Reserve; a
   * Reserve removes the pod's CPUs.  NULL = no reservation holds CPUs (also
   * the update_nodes default). */
  const uint64_t *resv_cpus[KOORDHIP_NUMA_WORDS];
  /* ---- ABI 9 (read only by the sequential cycle, koordhip_place_stream_ext) */
  /* DeviceShare: minors per type per node held by the dev_* columns (0 = no
   * devices anywhere: the columns may be NULL); dev_minor [n][TYPES][dev_slots]
   * in ascending minor order, -1 = empty slot; dev_total / dev_used
   * [n][TYPES][dev_slots][RES]: the minor's Device CR resources (all 0 for an
   * unhealthy device, buildDeviceResources device_cache.go:550-568) and the
   * amounts pods hold (advanced by Reserve) */
  int32_t dev_slots;
  int32_t reserved2;
  const uint8_t *dev_present;  /* [n] 1 = the node has a nodeDevice entry (a Device CR); without one DeviceShare's
                                  Filter passes, its Score is 0 and its Reserve allocates nothing (plugin.go:298-301,
                                  scoring.go:42-45, :377-380) */
  const int32_t *dev_minor;
  const int64_t *dev_total;
  const int64_t *dev_used;
  /* NodeResourcesFit extended scalars [KOORDHIP_NXRES][n]: Allocatable and
   * Requested (advanced by Reserve); NULL = 0 */
  const int64_t *xalloc;
  const int64_t *xrequested;
  /* raw NodeAffinity (sum of the weights of the class's preferred terms that
   * match) and TaintToleration (count of PreferNoSchedule taints the class does
   * not tolerate) scores per (pod static class, node), [MAX_STATIC_CLASSES][n];
   * NULL = 0 */
  const uint16_t *static_score[2];
  /* PodTopologySpread (KOORDHIP_PLUGIN_PTS): the topology keys of the
   * snapshot's constraints (pts_keys <= KOORDHIP_PTS_KEYS; bit k of
   * pts_hostname: key k is kubernetes.io/hostname, whose domain is the node
   * itself), pts_dom [keys][n] = the node's domain for key k (0 ..
   * pts_ndom[k] - 1 < KOORDHIP_PTS_DOMAINS; the node index for a hostname key;
   * -1 = the node has no such label); the constraint table (pts_cons <=
   * KOORDHIP_PTS_CONS distinct (label selector, namespace), pts_cons_key[c] =
   * its key) with pts_cnt [cons][n] = the node's pods in that namespace the
   * selector matches (countPodsMatchSelector; advanced by Reserve); pts_elig [n]
   * bit 2s = the node matches spread class s's required node affinity and holds
   * every DoNotSchedule key of the class, bit 2s + 1 = ... every ScheduleAnyway
   * key (pts_classes <= KOORDHIP_PTS_CLASSES).  pts_keys 0: no columns. */
  int32_t pts_keys;
  uint32_t pts_hostname;
  int32_t pts_ndom[KOORDHIP_PTS_KEYS];
  int32_t pts_cons;
  int32_t pts_classes;
  int32_t pts_cons_key[KOORDHIP_PTS_CONS];
  const int32_t *pts_dom;
  const int32_t *pts_cnt;
  const uint16_t *pts_elig;
  /* InterPodAffinity (KOORDHIP_PLUGIN_IPA): count entries over the pts_* topology
   * keys (ipa_ents <= KOORDHIP_IPA_ENTRIES, entry e on key ipa_ent_key[e]); ipa_cnt
   * [ents][n] = the node's pods entry e counts (advanced by Reserve): a "match"
   * entry counts the pods a term (or, for a pod's required affinity, all of its
   * terms) matches, a "carry" entry the pods that carry an affinity term.  The
   * pod-side masks and weights (koordhip_pod_ext.ipa_*) say which entries a pod
   * reads and how; the domain sums over the nodes of a (key, value) pair are the
   * reference's topologyPair counts.  ipa_ents 0: no columns. */
  int32_t ipa_ents;
  int32_t ipa_reserved;
  int32_t ipa_ent_key[KOORDHIP_IPA_ENTRIES];
  const int32_t *ipa_cnt;
  /* ABI 13: DeviceShare with a reservation holding devices (the reservation
   * restore, deviceshare/reservation.go:119-170; Filter / FilterReservation /
   * Score / ScoreReservation / Reserve through tryAllocateFromReservation
   * :181-283 and the nominated reservation :365-443).  resv_dev_slot [n]: the
   * reservation slot (0 .. max(resv_slots, 1) - 1) of node i's one reservation
   * holding devices, -1 = none (at most one per node: the host rejects more).
   * resv_dev [n][2][TYPES][dev_slots][RES]: [0] that reservation's allocatable
   * (its reserve pod's device allocation, nd.getUsed(reservePod)) and [1] its
   * allocated (its AssignedPods' allocations on those minors,
   * appendAllocatedByHints :145-151; advanced by Reserve).  Both allocations
   * are also in dev_used, as in the reference's deviceUsed.  NULL = none.  The
   * sequential cycle places batches on such snapshots. */
  const int32_t *resv_dev_slot;
  const int64_t *resv_dev;
  /* ABI 14: the NodeResourcesFit extended scalars of that reservation
   * (koordinator.sh/gpu-core, nvidia.com/gpu, ...; the KOORDHIP_NXRES slots of
   * xalloc): resv_xalloc [NXRES][n] = its Allocatable's scalars (the reserve
   * pod's scalar requests; a scalar it lists must be > 0: the host rejects a
   * zero-valued key), resv_xallocated [NXRES][n] = its Allocated's (its
   * AssignedPods' scalar requests masked to those keys, reservation_info.go:
   * 297-306; advanced by Reserve).  0 on nodes whose resv_dev_slot is -1.  They
   * enter every rule the reference applies to a reservation's ResourceList:
   * the restore of NodeInfo.Requested's scalars (RemovePod of the reserve pod
   * for a matched reservation, -Allocatable + SubtractWithNonNegativeResult(
   * Allocatable, Allocated) for an unmatched one with assigned pods,
   * transformer.go:227-293), filterWithReservations' fitsNode over the pod's
   * scalars (plugin.go:445-494), Restricted's LessThanOrEqual (:420-432),
   * FilterReservation's intersection (:504-535), scoreReservation's
   * MostAllocated over RemoveZeros(Allocatable) (scoring.go:177-200) and the
   * Reserve's AddAssignedPod.  NULL = none.  A snapshot with a non-zero value
   * places every batch in the sequential cycle (koordhip_eval refuses it: use
   * koordhip_eval_ext). */
  const int64_t *resv_xalloc;
  const int64_t *resv_xallocated;
} koordhip_node_soa;

/* One pod of the stream, the host-side PreFilter product (96 bytes). */
typedef struct koordhip_pod {
  int64_t req[KOORDHIP_NRES]; /* computePodResourceRequest (upstream fit.go): max(sum containers, init) + overhead */
  int64_t nz_cpu_m;           /* non-zero request: GetNonzeroRequests defaults 100m / 200Mi (upstream) */
  int64_t nz_mem;
  int64_t est_cpu;            /* EstimatePod(pod)[cpu]    (default_estimator.go:57-108) */
  int64_t est_mem;            /* EstimatePod(pod)[memory] */
  uint32_t flags;             /* KOORDHIP_POD_* */
  int32_t numa_cpus;          /* NUMA numCPUsNeeded (plugin.go:252) */
  uint32_t numa_policy;       /* KOORDHIP_NUMA_* packed policies */
  int32_t static_class;       /* KOORDHIP_PLUGIN_NODE_STATIC: the pod's class (0 .. MAX_STATIC_CLASSES-1): pods
                                 of one class share nodeSelector, required node affinity and tolerations */
  uint64_t resv_match;        /* bit g: MatchReservationOwners(pod, owner group g) (util/reservation/reservation.go:389-410) */
} koordhip_pod;

/* Per-pod inputs of the normalized-score plugins (the host's DeviceShare
 * PreFilter: PreparePod, plugin.go:162-182), beside koordhip_pod. */
typedef struct koordhip_pod_ext {
  /* ConvertDeviceRequest of each type's request (utils.go:86-181): gpu [0]
   * core, [1] memory-ratio, [2] memory bytes, -1 = key absent (memory and
   * ratio are completed per node from its GPU memory, fillGPUTotalMem
   * utils.go:211-233); rdma / fpga [t][0], 0 = none */
  int64_t dev_req[KOORDHIP_DEV_TYPES][KOORDHIP_DEV_RES];
  int64_t xreq[KOORDHIP_NXRES];  /* NodeResourcesFit extended scalar requests */
  uint32_t flags;                /* KOORDHIP_PODX_* */
  uint32_t xmask;                /* bit j: the pod's request map holds extended scalar j (xreq[j], even 0) */
  /* PodTopologySpread: the pod's spec.topologySpreadConstraints in order
   * (pts_n <= KOORDHIP_PTS_POD): pts_c[j] = its constraint table index,
   * pts_fl[j] KOORDHIP_PTS_HARD (DoNotSchedule) / KOORDHIP_PTS_SELF (its
   * selector matches the pod's own labels), pts_skew[j] = maxSkew; pts_class =
   * the pod's spread class; pts_match bit c = table constraint c counts this
   * pod once it is placed (its namespace and selector match). */
  uint8_t pts_n;
  uint8_t pts_class;
  uint8_t pts_match;
  uint8_t pts_pad;
  uint8_t pts_c[KOORDHIP_PTS_POD];
  uint8_t pts_fl[KOORDHIP_PTS_POD];
  int32_t pts_skew[KOORDHIP_PTS_POD];
  int32_t reserve_node;  /* KOORDHIP_POD_RESERVE: 1 + the node index its reservation names
                            (GetReservePodNodeName, plugin.go:335-339), 0 = any node */
  /* InterPodAffinity, bit e = count entry e of the snapshot:
   *   ipa_inc   entries that count this pod once it is placed (NodeInfo.AddPod)
   *   ipa_aff   its required affinity terms' entry per topology key: a node
   *             passes when it has every key and each pair counts > 0, or when
   *             no pair counts anywhere and KOORDHIP_IPA_SELF (satisfyPodAffinity)
   *   ipa_anti  its required anti-affinity terms' entries and the existing
   *             pods' required anti-affinity terms that match it: a node fails
   *             when one of them counts > 0 in the node's pair
   *   ipa_score entries with a nonzero ipa_w: raw Score = sum of ipa_w[e] x the
   *             pair count of e at the node (the reference's topologyScore) */
  uint32_t ipa_inc;
  uint32_t ipa_aff;
  uint32_t ipa_anti;
  uint32_t ipa_score;
  uint32_t ipa_flags;
  int32_t ipa_reserved;
  int32_t ipa_w[KOORDHIP_IPA_ENTRIES];
} koordhip_pod_ext;
#define KOORDHIP_PODX_DEVICE 1u  /* some device request (DeviceShare state.skip == false) */
#define KOORDHIP_PTS_HARD 1u
#define KOORDHIP_PTS_SELF 2u
#define KOORDHIP_IPA_SELF 1u     /* the pod matches all of its own required affinity terms */

/* One top-k record of koordhip_eval. */
typedef struct koordhip_topk {
  int32_t node;   /* node index, -1 = none */
  int32_t score;  /* total weighted score */
} koordhip_topk;

/* ---- lifecycle ---------------------------------------------------------- */
const char *koordhip_last_error(void);
int koordhip_abi_version(void);
int koordhip_create(const koordhip_config *cfg, koordhip_ctx **out);
int koordhip_destroy(koordhip_ctx *ctx);

/* Copy a full snapshot of n nodes to device (replaces any previous one) and
 * run the on-device LoadAware threshold-mask kernel. */
int koordhip_load_snapshot(koordhip_ctx *ctx, const koordhip_node_soa *soa, int32_t n);

/* Replace rows idx[0..m) with rows 0..m of `rows` (informer deltas) and
 * recompute their masks. */
int koordhip_update_nodes(koordhip_ctx *ctx, const int32_t *idx, const koordhip_node_soa *rows, int32_t m);

/* Copy the current (committed) mutable columns back to host arrays; any
 * pointer may be NULL.  Used by tests and the Go shim's debug service. */
int koordhip_read_nodes(koordhip_ctx *ctx, int64_t *requested /* [NRES][n] */, int64_t *nz /* [2][n] */,
                        int32_t *npods, int64_t *la_used /* [2][n] */, int64_t *la_used_prod /* [2][n] */);
/* NodeNUMAResource mutable state: free / exclusive masks [WORDS][n], allocated CPU counts [n]. */
int koordhip_read_numa(koordhip_ctx *ctx, uint64_t *free_mask, uint64_t *excl_pcpu, uint64_t *excl_numa,
                       int32_t *alloc_cnt);
/* ... and the NUMA zone allocations, [n][2][KOORDHIP_NUMA_MAX_NODES] like numa_zone_used
 * (rows of nodes without a topology policy read as 0: the engine does not keep them). */
int koordhip_read_numa_zones(koordhip_ctx *ctx, int64_t *zone_used);
/* Reservation mutable state: Allocated [2][S n] (cpu milli, memory), len(AssignedPods) [S n],
 * S = the loaded snapshot's reservation slots (1 when resv_slots <= 1), slot-major like the columns. */
int koordhip_read_reservations(koordhip_ctx *ctx, int64_t *allocated, int32_t *assigned);
/* ... and the reservations' remaining reserved CPUs [WORDS][S n] (zeros when no loaded reservation holds CPUs). */
int koordhip_read_resv_cpus(koordhip_ctx *ctx, uint64_t *cpus);
/* ABI 13: the loaded resv_dev column [n][2][TYPES][dev_slots][RES] (its
 * allocated half advanced by Reserve); zeros without one. */
int koordhip_read_resv_devices(koordhip_ctx *ctx, int64_t *resv_dev);
/* ABI 14: the loaded resv_xallocated column [NXRES][n] (advanced by Reserve);
 * zeros without one. */
int koordhip_read_resv_scalars(koordhip_ctx *ctx, int64_t *resv_xallocated);

/* Parity/debug mode, no commit: for n_pods pods against the current state.
 *   status : optional, [n_pods][n] KOORDHIP_ST_* bits (every plugin evaluated)
 *   scores : optional, [n_pods][KOORDHIP_NPLUGINS][n] per-plugin scores (0 where the plugin is disabled;
 *            the NodeNUMAResource score of a pair failing the NUMA Filter is unspecified, as the
 *            framework never scores such a node)
 *   topk   : optional, [n_pods][k] best feasible nodes by (total desc, index asc), node = -1 past the end
 *            (with the Reservation plugin, `score` is the ranking total of DESIGN.md's Reservation key:
 *            its order equals the order of the normalized weighted sums for the pod) */
int koordhip_eval(koordhip_ctx *ctx, const koordhip_pod *pods, int32_t n_pods, uint8_t *status, int32_t *scores,
                  koordhip_topk *topk, int32_t k);

/* ABI 9: the same with koordhip_pod_ext records (ext may be NULL: no device
 * requests), for every profile, including the normalized-score plugins.
 * status: [n_pods][n] 16-bit KOORDHIP_ST_* bits (incl. KOORDHIP_ST_IPA_FAIL).
 * scores: [n_pods][KOORDHIP_NPLUGINS + KOORDHIP_NEXT_PLUGINS][n], planes
 * NPLUGINS.. the raw (un-normalized) DeviceShare / NodeAffinity /
 * TaintToleration / PodTopologySpread (feasible nodes) / InterPodAffinity
 * (every node) scores; topk ranks the normalized weighted sums. */
int koordhip_eval_ext(koordhip_ctx *ctx, const koordhip_pod *pods, const koordhip_pod_ext *ext, int32_t n_pods,
                      uint16_t *status, int32_t *scores, koordhip_topk *topk, int32_t k);

/* Greedy stream: pods attempted once, in order, each against the state left
 * by all earlier commits; winner = lowest-index max total score; the Reserve
 * delta is applied on device.  out_node[i] = node, -1 unschedulable, -2 the
 * winner's Reserve failed (NodeNUMAResource Allocate; nothing committed, no
 * retry). */
int koordhip_place_stream(koordhip_ctx *ctx, const koordhip_pod *pods, int32_t n_pods, int32_t *out_node);
/* ABI 9: the greedy stream with koordhip_pod_ext records (ext may be NULL).
 * A profile enabling a normalized-score plugin (DeviceShare, NodeAffinity /
 * TaintToleration Score) runs the exact sequential cycle: per pod, every node
 * is filtered and scored on the state all earlier commits left, the
 * normalized plugins' maxima are reduced over the feasible nodes, then the
 * lowest-index argmax commits -- one persistent launch over every CU. */
int koordhip_place_stream_ext(koordhip_ctx *ctx, const koordhip_pod *pods, const koordhip_pod_ext *ext,
                              int32_t n_pods, int32_t *out_node);
/* Devices each pod of the last place call got: [n_pods][KOORDHIP_DEV_TYPES]
 * bit s = dev slot s of its node (the DeviceAllocations PreBind writes,
 * plugin.go:465-478: every allocated minor holds the pod's per-card request). */
int koordhip_fetch_devices(koordhip_ctx *ctx, uint32_t *slots, int32_t n_pods);
/* DeviceShare and extended-scalar mutable state: dev_used [n][TYPES][dev_slots][RES],
 * xrequested [NXRES][n] (either may be NULL). */
int koordhip_read_devices(koordhip_ctx *ctx, int64_t *dev_used, int64_t *xrequested);
/* PodTopologySpread: each table constraint's matching pods per node after the
 * last place call, [pts_cons][n] (NodeInfo.AddPod of the placed pods). */
int koordhip_read_pts(koordhip_ctx *ctx, int32_t *cnt);
/* InterPodAffinity: each count entry's pods per node after the last place
 * call, [ipa_ents][n]. */
int koordhip_read_ipa(koordhip_ctx *ctx, int32_t *cnt);

/* ---- ABI 15: why a pod is unschedulable ----------------------------------
 * Per-plugin node counts of a pod's Filter result, reduced on device (136
 * bytes per pod instead of one status byte per node).  Slot b of `any` and
 * `first` counts KOORDHIP_ST_* bit (1u << b).
 *   any[b]   nodes whose status has the bit: every plugin evaluated, no
 *            short-circuit, exactly koordhip_eval's status
 *   first[b] nodes whose FIRST failing Filter plugin is the bit, in the
 *            framework's Filter order STATIC -> FIT -> LA -> NUMA -> RESV: the
 *            (upstream) default order (NodeUnschedulable / TaintToleration /
 *            NodeAffinity, then NodeResourcesFit) followed by the koordinator
 *            plugins as config/manager/scheduler-config.yaml:65-70 lists them.
 *            The upstream half of that order is k8s v1.24.15's default plugin
 *            list, which is not vendored: like the other upstream parity in
 *            DESIGN.md it is restated, unpinned by reference tests.  Upstream
 *            stops at a node's first failing Filter plugin, so `first` is what
 *            Diagnosis.UnschedulablePlugins and the "0/N nodes are available"
 *            event counts are made of.
 * feasible + sum(first) = n. */
#define KOORDHIP_DIAG_BITS 16
typedef struct koordhip_diag {
  int32_t feasible;                   /* nodes with no Filter bit set */
  int32_t reserved;
  int32_t any[KOORDHIP_DIAG_BITS];
  int32_t first[KOORDHIP_DIAG_BITS];
} koordhip_diag;

/* Stateless, no commit: out[p] = the record of pods[p] against the current
 * state.  Every profile koordhip_eval's own kernel covers (Reservation
 * snapshots included); KOORDHIP_EINVAL on a sequential-cycle profile or
 * snapshot and for reserve / reservation-operating-mode pods. */
int koordhip_diagnose(koordhip_ctx *ctx, const koordhip_pod *pods, int32_t n_pods, koordhip_diag *out);
/* The last place call's unplaced pods at their DECISION state: for every pod
 * p with out_node[p] < 0 (-1 and -2) the record evaluated on the state the
 * commits of pods < p left; all-zero records for placed pods.  Computed on
 * demand from the pods, placements and cpusets the place call left on device
 * by un-applying later commits from the final rows in registers:
 * it writes no engine state and costs nothing when not called.
 * KOORDHIP_ESTATE once a state-changing call followed the place call
 * (koordhip_commit / koordhip_uncommit and their _ext forms,
 * koordhip_update_nodes, koordhip_load_snapshot, koordhip_restore, another
 * stage or place call).  The envelope is koordhip_uncommit's: no Reservation
 * plugin state, no NUMA topology-policy nodes, no sequential-cycle profile,
 * no koordhip_pod_ext records, no reserve pods, no communicator attached --
 * outside it KOORDHIP_EINVAL (the placements are untouched). */
int koordhip_fetch_diagnosis(koordhip_ctx *ctx, koordhip_diag *out /* [n_pods] */, int32_t n_pods);
/* The [n] KOORDHIP_ST_* status bytes of ONE unplaced pod of the last place
 * call at its decision state: the NodeToStatusMap of the pod the host runs
 * PostFilter (preemption) for.  Same envelope and validity rule;
 * KOORDHIP_EINVAL for a pod that was placed. */
int koordhip_fetch_node_status(koordhip_ctx *ctx, int32_t pod_index, uint8_t *status /* [n] */);

/* ---- ... for the sequential cycle's profiles (additive to ABI 15: detect it
 * by the symbols) ------------------------------------------------------------
 * The two calls below answer for every profile and snapshot koordhip_eval_ext
 * evaluates: DeviceShare, the extended scalars, PodTopologySpread,
 * InterPodAffinity, the normalized NodeAffinity / TaintToleration Scores, and
 * Reservation snapshots with more than KOORDHIP_RESV_SLOTS reservations on a
 * node, topology-policy nodes or reservations holding devices.  Both evaluate
 * against the CURRENT engine state and change none of it (a later
 * koordhip_fetch_diagnosis still works).
 *
 * The record is the koordhip_diag above with four more slots filled: 5
 * KOORDHIP_ST_DEVICE_FAIL, 6 KOORDHIP_ST_XFIT_FAIL, 7 KOORDHIP_ST_PTS_FAIL and 8
 * KOORDHIP_ST_IPA_FAIL.  any[b] is the histogram of koordhip_eval_ext's status,
 * with one difference: filterWithReservations' fitsNode covers the pod's
 * extended scalars (reservation/plugin.go:445-494), so RESV is also set where
 * only they fail the matched Aligned / Restricted reservations -- the
 * reference's answer, which koordhip_eval_ext's RESV bit does not give yet.
 * first[b] follows the framework's Filter order
 *   STATIC -> FIT -> XFIT -> PTS -> IPA -> LA -> NUMA -> DEVICE -> RESV
 * The first half is the (upstream) k8s v1.24 v1beta2 default plugin list --
 * NodeUnschedulable / TaintToleration / NodeAffinity, NodeResourcesFit,
 * PodTopologySpread, InterPodAffinity -- not vendored and therefore unpinned,
 * like the rest of the upstream parity.  The second half is what
 * config/manager/scheduler-config.yaml's filter.enabled list appends:
 * LoadAwareScheduling, NodeNUMAResource, DeviceShare, Reservation.  XFIT is
 * NodeResourcesFit on the extended scalars, the same plugin as FIT: the two are
 * adjacent and a node failing both counts under FIT.  Restricted to the five
 * older bits this is the order above, so a record without one of the new bits
 * is identical to what the plain call gives; feasible + sum(first) = n holds.
 *
 * Validation is that of koordhip_eval_ext (the ext records against the
 * profile and the snapshot's tables: KOORDHIP_EINVAL; no snapshot:
 * KOORDHIP_ESTATE) and, as for the plain call, KOORDHIP_EINVAL for reserve /
 * reservation-operating-mode pods.  ext may be NULL (no pod carries a record).
 * Device traffic to the host is the records alone (136 B per pod): no
 * per-(pod, node) plane exists on either side. */
int koordhip_diagnose_ext(koordhip_ctx *ctx, const koordhip_pod *pods, const koordhip_pod_ext *ext, int32_t n_pods,
                          koordhip_diag *out /* [n_pods] */);
/* One pod's NodeToStatusMap on the current state: status[n], the 16-bit
 * KOORDHIP_ST_* bits koordhip_eval_ext reports for that pod (every plugin
 * evaluated), without its score planes and per-call buffers. */
int koordhip_node_status_ext(koordhip_ctx *ctx, const koordhip_pod *pod, const koordhip_pod_ext *ext,
                             uint16_t *status /* [n] */);

/* ---- FitError reasons per node (additive to ABI 15: detect it by the symbols)
 * What upstream's FitError.Error() prints is a histogram of Status REASONS, not
 * of plugin names, and PostFilter's nodesWherePreemptionMightHelp drops the
 * nodes whose status code is UnschedulableAndUnresolvable.  A reason is a bit
 * index; the code (U = Unschedulable, UU = UnschedulableAndUnresolvable, E =
 * Error) is fixed per reason.
 *
 *   slot name                  reference string / site                       code
 *    0   STATIC                NodeUnschedulable / NodeAffinity /            UU
 *                              TaintToleration (the host-resolved class bit)
 *    1   FIT_PODS              "Too many pods"                               U
 *    2   FIT_CPU               "Insufficient cpu"                            U
 *    3   FIT_MEM               "Insufficient memory"                         U
 *    4   FIT_EPH               "Insufficient ephemeral-storage"              U
 *    5   FIT_BCPU              "Insufficient kubernetes.io/batch-cpu"        U
 *    6   FIT_BMEM              "Insufficient kubernetes.io/batch-memory"     U
 *    7   LA_USAGE              load_aware.go:45-46 (one slot)                U
 *    8   NUMA_POD_ERROR        plugin.go:244 (KOORDHIP_POD_NUMA_ERROR)       E
 *    9   NUMA_AMP_CPU          ErrInsufficientAmplifiedCPU, plugin.go:360    U
 *   10   NUMA_NO_TOPOLOGY      ErrNotFoundCPUTopology / ErrInvalidCPUTopology UU
 *                              plugin.go:286,293
 *   11   NUMA_SMT_ALIGN        ErrSMTAlignmentError, plugin.go:298           UU
 *   12   NUMA_FULL_PCPUS_ONLY  ErrRequiredFullPCPUsPolicy, plugin.go:303     UU
 *   13   NUMA_CPUS             "not enough cpus available to satisfy         U
 *                              request", resource_manager.go:258
 *   14   NUMA_REQUIRED_POLICY  "insufficient CPUs to satisfy required cpu    U
 *                              bind policy", resource_manager.go:450
 *   15   NUMA_NO_ZONES         "node(s) missing NUMA resources",             UU
 *                              topology_hint.go:36
 *   16   NUMA_POLICY           Admit / Allocate fails on a topology-policy   U
 *                              node (one slot)
 *   17   RESV_AFFINITY         ErrReasonReservationAffinity                  UU
 *   18   RESV_INSUFFICIENT     ErrReasonReservationInsufficientResources     U
 *   19-31 the sequential cycle's plugins, filled by koordhip_diagnose_reasons_ext
 *        / koordhip_node_reasons_ext alone (zero from every other call):
 *   19+j FIT_X0 .. FIT_X7      "Insufficient <extended scalar j>" (j = 0 ..    U
 *                              KOORDHIP_NXRES-1; upstream fitsRequest over
 *                              ScalarResources)
 *   27   DEVICE_INSUFFICIENT   ErrInsufficientDevices, deviceshare/            U
 *                              plugin.go:322; also "node(s) reservations
 *                              insufficient devices", deviceshare/
 *                              reservation.go:280 (one slot: the engine's
 *                              device evaluation gives one verdict)
 *   28   PTS_MISSING_LABEL     upstream ErrReasonNodeLabelNotMatch             UU
 *   29   PTS_SKEW              upstream ErrReasonConstraintsNotMatch           U
 *   30   IPA_AFFINITY          upstream ErrReasonAffinityRulesNotMatch         UU
 *   31   IPA_ANTI              upstream ErrReasonAntiAffinityRulesNotMatch;    U
 *                              also ErrReasonExistingAntiAffinityRulesNotMatch
 *                              (one slot: koordhip_pod_ext.ipa_anti folds both)
 *
 * NodeResourcesFit reports every failing resource of fitsRequest -- the FIT_*
 * and FIT_X* slots are one plugin's; every other plugin reports one reason, the
 * reference's first exit.  PodTopologySpread walks the pod's DoNotSchedule
 * constraints in record order: the first whose key the node lacks gives
 * PTS_MISSING_LABEL, the first whose skew exceeds maxSkew PTS_SKEW.
 * InterPodAffinity checks the required affinity before the two anti-affinity
 * checks (satisfyPodAffinity first): a node failing both reports IPA_AFFINITY.
 * The upstream plugins are not vendored: these exits are unpinned like the
 * rest of the upstream parity. */
#define KOORDHIP_REASON_STATIC 0
#define KOORDHIP_REASON_FIT_PODS 1
#define KOORDHIP_REASON_FIT_CPU 2
#define KOORDHIP_REASON_FIT_MEM 3
#define KOORDHIP_REASON_FIT_EPH 4
#define KOORDHIP_REASON_FIT_BCPU 5
#define KOORDHIP_REASON_FIT_BMEM 6
#define KOORDHIP_REASON_LA_USAGE 7
#define KOORDHIP_REASON_NUMA_POD_ERROR 8
#define KOORDHIP_REASON_NUMA_AMP_CPU 9
#define KOORDHIP_REASON_NUMA_NO_TOPOLOGY 10
#define KOORDHIP_REASON_NUMA_SMT_ALIGN 11
#define KOORDHIP_REASON_NUMA_FULL_PCPUS_ONLY 12
#define KOORDHIP_REASON_NUMA_CPUS 13
#define KOORDHIP_REASON_NUMA_REQUIRED_POLICY 14
#define KOORDHIP_REASON_NUMA_NO_ZONES 15
#define KOORDHIP_REASON_NUMA_POLICY 16
#define KOORDHIP_REASON_RESV_AFFINITY 17
#define KOORDHIP_REASON_RESV_INSUFFICIENT 18
#define KOORDHIP_REASON_COUNT 19
#define KOORDHIP_REASON_SLOTS 32
/* ... and the sequential cycle's (the _ext calls below) */
#define KOORDHIP_REASON_FIT_X0 19 /* + j: extended scalar j */
#define KOORDHIP_REASON_DEVICE_INSUFFICIENT 27
#define KOORDHIP_REASON_PTS_MISSING_LABEL 28
#define KOORDHIP_REASON_PTS_SKEW 29
#define KOORDHIP_REASON_IPA_AFFINITY 30
#define KOORDHIP_REASON_IPA_ANTI 31
#define KOORDHIP_REASON_EXT_COUNT 32
/* the reasons of each KOORDHIP_ST_* bit (a status bit is set iff one of its reasons is) */
#define KOORDHIP_REASONS_OF_STATIC 0x00000001u
#define KOORDHIP_REASONS_OF_FIT 0x0000007Eu
#define KOORDHIP_REASONS_OF_LA 0x00000080u
#define KOORDHIP_REASONS_OF_NUMA 0x0001FF00u
#define KOORDHIP_REASONS_OF_RESV 0x00060000u
/* the reasons whose code is UnschedulableAndUnresolvable: STATIC, NUMA_NO_TOPOLOGY,
 * NUMA_SMT_ALIGN, NUMA_FULL_PCPUS_ONLY, NUMA_NO_ZONES, RESV_AFFINITY */
#define KOORDHIP_REASON_UNRESOLVABLE_MASK 0x00029C01u
/* ... and Error: NUMA_POD_ERROR */
#define KOORDHIP_REASON_ERROR_MASK 0x00000100u
/* the sequential cycle's groups (XFIT: NodeResourcesFit as well, one plugin with REASONS_OF_FIT) ... */
#define KOORDHIP_REASONS_OF_XFIT 0x07F80000u
#define KOORDHIP_REASONS_OF_DEVICE 0x08000000u
#define KOORDHIP_REASONS_OF_PTS 0x30000000u
#define KOORDHIP_REASONS_OF_IPA 0xC0000000u
/* ... and the UnschedulableAndUnresolvable reasons with theirs: + PTS_MISSING_LABEL, IPA_AFFINITY */
#define KOORDHIP_REASON_EXT_UNRESOLVABLE_MASK 0x50029C01u

typedef struct koordhip_reasons { /* 264 B */
  int32_t feasible;               /* nodes with no reason set */
  int32_t unresolvable;           /* nodes whose FIRST failing plugin reports a UU reason */
  int32_t first[KOORDHIP_REASON_SLOTS]; /* nodes whose first failing plugin (the order of koordhip_diag.first) reports
                                            reason r: the histogram FitError.Error() prints */
  int32_t any[KOORDHIP_REASON_SLOTS];   /* nodes where reason r holds, every plugin evaluated */
} koordhip_reasons;

/* koordhip_diagnose's call with reason records: the current state, the same
 * envelope, error codes and "writes no engine state" rule. */
int koordhip_diagnose_reasons(koordhip_ctx *ctx, const koordhip_pod *pods, int32_t n_pods, koordhip_reasons *out);
/* One pod on the current state: mask[i] = the reasons of every failing plugin
 * on node i (the `any` view; the first plugin and the code follow from it). */
int koordhip_node_reasons(koordhip_ctx *ctx, const koordhip_pod *pod, uint32_t *mask /* [n] */);
/* koordhip_fetch_diagnosis' call with reason records: the last place call's
 * unplaced pods at their decision states; same envelope and validity rule. */
int koordhip_fetch_reasons(koordhip_ctx *ctx, koordhip_reasons *out /* [n_pods] */, int32_t n_pods);
/* koordhip_fetch_node_status' call with reason masks. */
int koordhip_fetch_node_reasons(koordhip_ctx *ctx, int32_t pod_index, uint32_t *mask /* [n] */);

/* ---- ... for the sequential cycle's profiles (additive to ABI 15: detect it
 * by the symbols) ------------------------------------------------------------
 * koordhip_diagnose_ext's call with reason records, for every profile and
 * snapshot it answers for: the current state, its validation and error codes
 * (KOORDHIP_EINVAL for reserve / reservation-operating-mode pods and for bad
 * ext records, KOORDHIP_ESTATE without a snapshot), no engine state written
 * (a later koordhip_fetch_diagnosis still works).  The record fills slots
 * 19-31 too.  `first` follows koordhip_diagnose_ext's Filter order with
 * NodeResourcesFit's FIT_* and FIT_X* reasons as one group (a node whose first
 * failing plugin is NodeResourcesFit reports all of them); `unresolvable`
 * counts the nodes whose first failing plugin reports a reason of
 * KOORDHIP_REASON_EXT_UNRESOLVABLE_MASK.  RESV_INSUFFICIENT follows
 * koordhip_diagnose_ext's RESV convention (the pod's extended scalars are part
 * of fitsNode).  On a profile outside the sequential cycle with ext NULL the
 * record is byte-identical to koordhip_diagnose_reasons'. */
int koordhip_diagnose_reasons_ext(koordhip_ctx *ctx, const koordhip_pod *pods, const koordhip_pod_ext *ext /* may be NULL */,
                                  int32_t n_pods, koordhip_reasons *out /* [n_pods] */);
/* One pod on the current state: mask[i] = the reasons of every failing plugin
 * on node i; its KOORDHIP_ST_* bits are koordhip_node_status_ext's. */
int koordhip_node_reasons_ext(koordhip_ctx *ctx, const koordhip_pod *pod, const koordhip_pod_ext *ext,
                              uint32_t *mask /* [n] */);

/* ---- preemption dry run (additive to ABI 15: detect it by the symbols) -----
 * The PostFilter of elasticquota/plugin.go:310-329: SelectVictimsOnNode
 * (elasticquota/preempt.go:111-215) on EVERY node, then one candidate picked,
 * all on device against the current engine state.  It writes no engine state.
 *
 * The host keeps a table of the pods that sit on the nodes: one record per
 * assigned pod.  `pod` is the record its Reserve used, i.e. what
 * NodeInfo.RemovePod / AddPod move. */
#define KOORDHIP_PREEMPT_QRES 4        /* quota dimensions (the host chooses which resources) */
#define KOORDHIP_PREEMPT_PDBS 8        /* PodDisruptionBudgets of one table */
#define KOORDHIP_PREEMPT_NODE_PODS 128 /* listed pods per node at most */

#define KOORDHIP_ASG_NONPREEMPTIBLE 1u /* extension.IsPodNonPreemptible */
#define KOORDHIP_ASG_IN_QUOTA 2u       /* quotaInfo.IsPodExist: the quota's used moves with the pod (plugin.go:302-305) */
/* bit 2 (4u) is the library's own (it marks the records koordhip_preempt_load_pods_ext gave a non-empty
 * koordhip_assigned_ext): a caller's bit there is ignored. */
/* bits 8-11 of flags: the reservation slot of ITS NODE the pod is bound to (its
 * reservation-allocated annotation), read in the KOORDHIP_PREEMPT_RESV mode
 * only.  A field value of 0 means not bound. */
#define KOORDHIP_ASG_RESV_SLOT(q) ((uint32_t)((q) + 1) << 8)
#define KOORDHIP_ASG_RESV_SLOT_MASK (15u << 8)
#define KOORDHIP_ASG_RESV_SLOT_OF(flags) (((flags) >> 8) & 15u) /* the field: slot + 1, 0 = not bound */

typedef struct koordhip_assigned {
  koordhip_pod pod;
  int32_t node;       /* node index in the loaded snapshot */
  int32_t priority;   /* corev1helpers.PodPriority */
  int64_t start_time; /* GetPodStartTime as unix ns (status.startTime, else the host's "now") */
  int32_t quota;      /* id of getPodAssociateQuotaName, host-assigned, >= 0 */
  uint32_t flags;     /* KOORDHIP_ASG_* */
  uint32_t pdb_mask;  /* bit i: PDB i matches the pod and the pod is not in its DisruptedPods (preempt.go:231-250) */
  uint32_t reserved;
  int64_t qreq[KOORDHIP_PREEMPT_QRES]; /* core.PodRequestsAndLimits in the quota dimensions, 0 .. 2^53 */
} koordhip_assigned;

typedef struct koordhip_preemptor {
  koordhip_pod pod;
  int32_t priority;
  int32_t quota;      /* -1: postFilterState.skip (no quota check; canPreempt still compares ids: no victims) */
  int64_t q_used[KOORDHIP_PREEMPT_QRES];    /* postFilterState.used, 0 .. 2^53 */
  int64_t q_runtime[KOORDHIP_PREEMPT_QRES]; /* postFilterState.runtime */
  int64_t q_req[KOORDHIP_PREEMPT_QRES];     /* the preemptor's own request, 0 .. 2^53 */
  uint32_t q_mask;    /* dimensions present in runtime (quotav1.LessThanOrEqual walks runtime's keys only) */
  uint32_t reserved;
} koordhip_preemptor;

#define KOORDHIP_PREEMPT_CANDIDATE 0    /* the preemptor fits once the victims are gone */
#define KOORDHIP_PREEMPT_NO_VICTIMS 1   /* no pod canPreempt accepts (preempt.go:150-153) */
#define KOORDHIP_PREEMPT_UNFIT 2        /* does not fit with every potential victim removed (:161-163) */
#define KOORDHIP_PREEMPT_ERROR 3        /* a pod removed twice: NodeInfo.RemovePod fails, the node is dropped */
#define KOORDHIP_PREEMPT_UNRESOLVABLE 4 /* KOORDHIP_ST_STATIC_FAIL (NUMA mode: see koordhip_preempt_set_mode): skipped by nodesWherePreemptionMightHelp */
#define KOORDHIP_PREEMPT_STATUSES 5

/* One node's verdict for one preemptor.  Every field but status is 0 unless
 * status is CANDIDATE (and 0 for a candidate without victims). */
typedef struct koordhip_preempt_node {
  int32_t status;
  int32_t n_victims;        /* the victims list's length */
  int32_t n_pdb_violations; /* PDB-violating pods that did not fit back (:201-207) */
  int32_t top_priority;     /* priority of the list's first victim (upstream reads Pods[0]) */
  int64_t sum_priority;     /* sum of (priority + 2^31) */
  int64_t earliest_start;   /* smallest start_time among the victims of maximal priority */
} koordhip_preempt_node;

typedef struct koordhip_preempt_result {
  int32_t node;                            /* the chosen node, -1: no candidate */
  int32_t count[KOORDHIP_PREEMPT_STATUSES]; /* nodes per status */
  koordhip_preempt_node best;              /* the chosen node's verdict (zero when node = -1) */
} koordhip_preempt_result;

/* Upload the table and build each node's list on device, ordered by
 * util.MoreImportantPod (priority descending, start_time ascending) and then
 * by ascending input index (Go's sort.Slice is unstable there; this rule is
 * the engine's).  The table does not depend on the node state: it stays until
 * the next call of this function or of load_snapshot.  KOORDHIP_EINVAL for a
 * node outside [0, n), more than KOORDHIP_PREEMPT_NODE_PODS pods on a node,
 * n_pdb above KOORDHIP_PREEMPT_PDBS, a pdb_mask bit at or above n_pdb, a
 * KOORDHIP_ASG_RESV_SLOT field above the loaded snapshot's resv_slots (ignored
 * without reservation columns; whether the slot is present on the node is not
 * checked). */
int koordhip_preempt_load_pods(koordhip_ctx *ctx, const koordhip_assigned *a, int32_t n_assigned,
                               const int32_t *pdb_allowed /* [n_pdb] DisruptionsAllowed */, int32_t n_pdb);
/* The dry run of n_pre preemptors, each on its own against the current state.
 * out[p].node is the lexicographic minimum over the CANDIDATE nodes of (has
 * victims, n_pdb_violations, top_priority, sum_priority, n_victims,
 * -earliest_start, node index): upstream v1.24 pickOneNodeForPreemption with
 * the lowest node index as its last rule.  victims (may be NULL) receives the
 * chosen node's victims as indices into a[], in the order the reference
 * appends them, padded with -1; with max_victims below best.n_victims the
 * list is truncated.  Profiles whose Filter is NodeResourcesFit, LoadAware
 * and the static filters on the pipelined path; KOORDHIP_EINVAL for
 * NodeNUMAResource, Reservation in the Filter or Reservation snapshots (each
 * unless koordhip_preempt_set_mode below accepted it), sequential-cycle profiles,
 * reserve pods and an attached communicator; KOORDHIP_ESTATE without a
 * snapshot or a loaded table. */
int koordhip_preempt(koordhip_ctx *ctx, const koordhip_preemptor *pre, int32_t n_pre, koordhip_preempt_result *out,
                     int32_t *victims /* [n_pre][max_victims] */, int32_t max_victims);
/* One preemptor's verdict on every node (the evaluator's per-node statuses). */
int koordhip_preempt_node_verdicts(koordhip_ctx *ctx, const koordhip_preemptor *pre,
                                   koordhip_preempt_node *per_node /* [n] */);

/* ---- the dry run under NodeNUMAResource (additive to ABI 15: detect it by the symbol)
 * koordhip_preempt_set_mode(ctx, KOORDHIP_PREEMPT_NUMA_FROZEN) lets the three
 * dry-run calls (koordhip_preempt, koordhip_preempt_node_verdicts,
 * koordhip_preempt_stream) accept NodeNUMAResource in the Filter: cpuset
 * preemptors, topology-policy nodes, amplified nodes.  The flag stands for a
 * semantic the host accepts by setting it.  NodeNUMAResource has no
 * PreFilterExtensions (nodenumaresource/plugin.go:262-264), so while
 * SelectVictimsOnNode removes and re-adds pods its state does not move:
 *   - a victim's cpuset and zone amounts are NOT freed: a node without enough
 *     free CPUs for a cpuset preemptor stays unfit however many cpuset pods
 *     would be evicted;
 *   - in koordhip_preempt_stream a nominated cpuset preemptor holds NO CPUs
 *     and no zone amounts on its node; only its requests are on the row.
 * The reference behaves the same way (see the TODO at plugin.go:346).
 *
 * Per (preemptor P, node) the plugin's Filter is split in two.  F is its
 * verdict without filterAmplifiedCPUs, on the loaded NUMA state: one constant
 * for the whole call.  A(w) is filterAmplifiedCPUs (plugin.go:326-363) on the
 * hypothetical row w: it reads Requested cpu, so it moves with the walk.
 *   - UNRESOLVABLE: KOORDHIP_ST_STATIC_FAIL as before, or NodeNUMAResource is
 *     the first failing plugin on the row the walk starts from (Fit, LoadAware
 *     and A pass there) and F is one of KOORDHIP_REASON_UNRESOLVABLE_MASK's
 *     reasons (NO_TOPOLOGY, NO_ZONES, SMT_ALIGN, FULL_PCPUS_ONLY);
 *   - every later "does P fit row w" is the Fit / LoadAware / static test
 *     together with F passing and A(w).  A node where F fails otherwise is
 *     NO_VICTIMS without a potential victim and UNFIT with one.
 * Everything else (the split, the reprieve order, the pick, the stream's
 * overlay) is unchanged.
 *
 * flags = 0 (the default) restores the refusal.  The mode belongs to the
 * context: it outlives load_snapshot and koordhip_preempt_load_pods, and it is
 * inert on a profile without NodeNUMAResource in the Filter.  KOORDHIP_EINVAL
 * for an unknown bit (the mode then stays as it was).  With the flag set still KOORDHIP_EINVAL: everything
 * koordhip_preempt lists besides NodeNUMAResource, and a preemptor with
 * KOORDHIP_POD_NUMA_ERROR (a PreFilter error aborts the cycle: no PostFilter). */
#define KOORDHIP_PREEMPT_NUMA_FROZEN 1u
/* ---- the dry run under Reservation (additive to ABI 15: detect it by the flag's acceptance)
 * KOORDHIP_PREEMPT_RESV lets koordhip_preempt and koordhip_preempt_node_verdicts
 * accept Reservation columns and the Reservation Filter on the pipelined path
 * (at most KOORDHIP_RESV_SLOTS reservations per node, no sequential-cycle
 * snapshot).  Unlike NodeNUMAResource the plugin has PreFilterExtensions
 * (reservation/plugin.go:250-323): its AddPod / RemovePod keep
 * preemptible[node] and preemptibleInRRs[node][reservation UID], and
 * filterWithReservations / fitsNode read both (:373-494).  The walk keeps that
 * state per (preemptor P, node):
 *   start row   the loaded row after the cycle's Reservation restore for P
 *               (the PostFilter runs on the NodeInfo BeforePreFilter restored).
 *   frozen      the reservation slots (Allocatable, Allocated, assigned count,
 *               policy, class) and nodeRState.podRequested, the clone taken
 *               before the matched restore (transformer.go:129); a node without
 *               a matched / unmatched-with-pods reservation has none (0).
 *   moving      over cpu, memory, ephemeral-storage, batch-cpu, batch-memory:
 *               RemovePod of a listed pod with a non-zero request adds its
 *               requests to Pn (not bound) or Pr[q] (bound to slot q, see
 *               KOORDHIP_ASG_RESV_SLOT); AddPod of a pod that is not bound
 *               subtracts from Pn, floored at 0.  AddPod of a BOUND pod is
 *               restated literally (:278-286): Pr[q] is deleted when Pr[q] -
 *               requests is zero in every resource and otherwise KEEPS ITS OLD
 *               VALUE (the reference never stores the difference; no reference
 *               table pins the partial add-back: parity unpinned, followed
 *               literally).  An entry is present iff some resource is
 *               non-zero.  Pods without requests move the row only.
 * Every "does P fit row w" is the test of the default mode (in the NUMA mode
 * with F and A(w)) and the Reservation Filter: without a matched reservation a
 * pod with KOORDHIP_POD_RESV_AFFINITY fails, otherwise, if Pn or some Pr[q] is
 * present, fitsNode(nil, preemptible = Pn) decides (ErrReasonPreemptionFailed);
 * with matched reservations fitsNode per slot q with preemptible = Pr[q] + Pn
 * and rRemained from the unmodified Allocated: a Default slot is insufficient
 * only if Pr[q] or Pn is present and fitsNode fails, an Aligned slot passes the
 * node if fitsNode passes, a Restricted one if also podRequests <= max(0,
 * Allocatable - a) over its resource names, a = max(0, Allocated - Pr[q]) with
 * Pr[q] present, else Allocated (:420-432); the node fails iff no Aligned /
 * Restricted slot passed and one policy group is non-empty and wholly
 * insufficient (:434-437).  UNRESOLVABLE as koordhip_diagnose_reasons counts
 * it: on the start row the first failing plugin holds one of
 * KOORDHIP_REASON_UNRESOLVABLE_MASK's reasons, now RESV_AFFINITY too.
 *
 * Named deviation: reserve pods are NOT listed in this mode (AddPod / RemovePod
 * skip them at :255,293, but NodeInfo.RemovePod would still move the restored
 * row): they are never potential victims.  Still KOORDHIP_EINVAL: reserve and
 * operating-mode preemptors; koordhip_preempt_stream on Reservation state, flag
 * or not (earlier victims have to leave the reservations' Allocated: the mode's
 * sequential dry run is koordhip_preempt_stream_resv below);
 * with NodeNUMAResource in the Filter the flag without
 * KOORDHIP_PREEMPT_NUMA_FROZEN, and both flags on a snapshot loaded with
 * resv_cpus (the frozen verdict does not model the restore of reserved CPUs).
 * The flag is inert on a context without Reservation state, with one
 * exception that koordhip_preempt_set_mode itself answers: on a profile with
 * NodeNUMAResource in the Filter and WITHOUT the Reservation plugin the word
 * is live (it decides the NUMA refusal), and a word with this bit is
 * KOORDHIP_EINVAL like an unknown bit and leaves the mode as it was: such a
 * context can never hold Reservation state. */
#define KOORDHIP_PREEMPT_RESV 2u
/* ---- the dry run under DeviceShare (additive to ABI 15: detect it by the symbols below)
 * KOORDHIP_PREEMPT_DEVICE lets koordhip_preempt, koordhip_preempt_node_verdicts
 * and their _ext forms accept a profile whose sequential-cycle plugins are
 * DeviceShare only (the NodeAffinity / TaintToleration normalized Scores may be
 * present: the dry run reads no Score).  The plugin has PreFilterExtensions
 * (deviceshare/plugin.go:184-282): RemovePod adds the victim's device
 * allocation to preemptibleDevices[node], AddPod subtracts it again, Filter
 * (:284-323) hands the map to the allocator, which frees it per minor
 * (device_cache.go:316-365, calcFreeWithPreemptible :454-482).  A victim's
 * extended scalars leave NodeInfo.Requested.ScalarResources through
 * NodeInfo.RemovePod, which NodeResourcesFit reads.  Per (preemptor P, node):
 *   row         also xrequested[j] of the scalars in P's xmask.
 *   RemovePod   of a listed pod: the row as before, xrequested[j] -= its xreq[j],
 *               and, when P has KOORDHIP_PODX_DEVICE, the node has a nodeDevice
 *               entry and the pod holds devices, Pd[t][s] += dev_per[t] for every
 *               slot s of its dev_slots[t].  AddPod is the reverse
 *               (SubtractWithNonNegativeResult per minor, a zero entry deleted,
 *               the difference stored: device_resources.go:65-104).  A pod is
 *               added back only after it was removed, so no clamp triggers and
 *               Pd is the sum over the pods removed at the moment.
 *   fit test    the mode's test, xfit on the moved xrequested, and for a device
 *               preemptor on a nodeDevice node the DeviceShare Filter with the
 *               free amounts of slot s of type t taken as
 *               max0(total - max0(used - Pd)); the rest as in the cycle
 *               (fillGPUTotalMem per node, calcDeviceWanted, a device counts if
 *               its free vector is non-zero and holds the per-card request,
 *               count >= wanted per requested type, a missing type fails).
 * LoadAware's columns do not move.  XFIT and DEVICE reasons are Unschedulable,
 * so UNRESOLVABLE keeps its rule and equals koordhip_diagnose_reasons_ext's
 * `unresolvable`.  Device pods' cpusets stay frozen under
 * KOORDHIP_PREEMPT_NUMA_FROZEN, which combines with this flag.
 * On a profile without DeviceShare (Filter or Score) a word with this bit is
 * KOORDHIP_EINVAL like an unknown bit and leaves the mode as it was.  Still
 * KOORDHIP_EINVAL with the flag set: PodTopologySpread or InterPodAffinity in
 * the profile (AddPod / RemovePod state of their own); any Reservation state
 * (the plugin in the Filter or Score, reservation columns, resv_dev_slot
 * columns), with or without KOORDHIP_PREEMPT_RESV, unless
 * KOORDHIP_PREEMPT_DEVICE_RESV below opted in (cpu / memory reservations only:
 * device-holding ones need tryAllocateFromReservation and are not built);
 * the plain koordhip_preempt_stream (it takes no koordhip_pod_ext records:
 * the mode's sequential dry run is koordhip_preempt_stream_ext below); what
 * koordhip_preempt refuses besides. */
#define KOORDHIP_PREEMPT_DEVICE 4u
/* ---- the dry run under DeviceShare beside Reservation state (additive to ABI 15: detect it by the flag's acceptance)
 * KOORDHIP_PREEMPT_DEVICE_RESV is the opt-in for the word KOORDHIP_PREEMPT_DEVICE
 * | KOORDHIP_PREEMPT_RESV | KOORDHIP_PREEMPT_DEVICE_RESV (with
 * KOORDHIP_PREEMPT_NUMA_FROZEN where NodeNUMAResource is in the Filter: the
 * shipped profile with DeviceShare needs all four).  koordhip_preempt_set_mode
 * accepts the bit only together with both other bits and on a profile that has
 * DeviceShare and the Reservation plugin (each in the Filter or Score);
 * everywhere else a word holding it is KOORDHIP_EINVAL like an unknown bit and
 * leaves the mode as it was.  With that word koordhip_preempt,
 * koordhip_preempt_ext, koordhip_preempt_node_verdicts and
 * koordhip_preempt_node_verdicts_ext accept a profile whose sequential-cycle
 * plugins are DeviceShare only, reservation columns with up to
 * KOORDHIP_RESV_SLOTS reservations per node holding cpu / memory, and listed
 * pods that name a slot (KOORDHIP_ASG_RESV_SLOT) and have a
 * koordhip_assigned_ext record.  Per (preemptor P, node) the walk is that of
 * the two modes together, with three rules that exist only where both states do:
 *   bound victims  DeviceShare's RemovePod / AddPod put a victim bound to a
 *               reservation into preemptibleInRRs[node][uid], not into
 *               preemptibleDevices[node] (deviceshare/plugin.go:188-282), and
 *               without a device-holding reservation nothing reads that map
 *               (reservation.go:192): Pd moves only for a pod that is NOT bound
 *               to a slot.  Its scalars still leave NodeInfo.Requested:
 *               xrequested moves for every listed pod.
 *   scalars     the Reservation plugin's maps are whole ResourceLists: Pn and
 *               Pr[q] also hold the listed pods' extended scalars, all
 *               KOORDHIP_NXRES of them ("has a non-zero request", presence and
 *               the literal add-back of a bound pod count them), and fitsNode
 *               tests every scalar j of P's xmask: fail if xreq[j] >
 *               xalloc[j] - (podRequested.x[j] - pre.x[j]), podRequested.x[j]
 *               the loaded xrequested[j] on a node with a nodeRState, else 0,
 *               pre = Pn without a matched slot, Pr[q] + Pn per matched slot.
 *               NodeResourcesFit reads the moved Requested, fitsNode the frozen
 *               one: fitsNode is the stricter test whenever a removed pod is
 *               bound to a reservation other than the one tested.
 *   order       DeviceShare precedes Reservation in the Filter: a required
 *               affinity without a match makes the node UNRESOLVABLE only where
 *               xfit and the DeviceShare Filter pass on the start row too.
 * count[UNRESOLVABLE] equals koordhip_diagnose_reasons_ext's `unresolvable`.
 * No reference test pins the bound branch of DeviceShare's RemovePod or
 * fitsNode's scalar term with something preemptible: parity unpinned, followed
 * literally.  Still KOORDHIP_EINVAL in this mode: resv_dev_slot / resv_dev /
 * resv_xalloc columns (device-holding reservations need mergedUnmatchedUsed,
 * mergedMatchedAllocatable and tryAllocateFromReservation: the follow-up); a
 * snapshot that places in the sequential cycle by its reservations (more than
 * KOORDHIP_RESV_SLOTS slots, topology-policy zones); resv_cpus with
 * KOORDHIP_PREEMPT_NUMA_FROZEN; koordhip_preempt_stream, _stream_ext and
 * _stream_resv (the sequential dry run under both states is not built); and
 * what the two modes refuse besides. */
#define KOORDHIP_PREEMPT_DEVICE_RESV 8u
int koordhip_preempt_set_mode(koordhip_ctx *ctx, uint32_t flags);

/* What a listed pod holds beyond its koordhip_pod, one record per koordhip_assigned
 * (parallel arrays).  Quantities in [0, 2^45). */
typedef struct koordhip_assigned_ext {
  int64_t xreq[KOORDHIP_NXRES]; /* its extended scalars in NodeInfo.Requested (moved by NodeInfo.RemovePod / AddPod) */
  int64_t dev_per[KOORDHIP_DEV_TYPES][KOORDHIP_DEV_RES]; /* the amount it holds on EACH of its minors of a type
                                                          * (every allocated minor holds the per-card request,
                                                          * plugin.go:465-478) */
  uint32_t dev_slots[KOORDHIP_DEV_TYPES]; /* bit s: device slot s of its node (koordhip_fetch_devices' convention) */
  uint32_t xmask;                         /* bit j: xreq[j] is present */
  uint64_t reserved;
} koordhip_assigned_ext;
/* koordhip_preempt_load_pods with the second table; ax == NULL is that call.
 * KOORDHIP_EINVAL, checked before anything else and leaving the loaded table
 * in place: a dev_slots bit at or above the snapshot's dev_slots, device
 * amounts on a context without device columns, a quantity out of range, an
 * xmask bit past KOORDHIP_NXRES. */
int koordhip_preempt_load_pods_ext(koordhip_ctx *ctx, const koordhip_assigned *a, const koordhip_assigned_ext *ax,
                                   int32_t n_assigned, const int32_t *pdb_allowed, int32_t n_pdb);
/* koordhip_preempt / koordhip_preempt_node_verdicts with the preemptors'
 * koordhip_pod_ext records (ext[p] beside pre[p]; NULL: all empty, which is the
 * plain call: state.skip makes the plugin's three hooks no-ops,
 * plugin.go:197,247,289).  Only dev_req, xreq, xmask and KOORDHIP_PODX_DEVICE
 * are read; a record with spread or affinity fields set is KOORDHIP_EINVAL, and
 * so is a non-NULL ext outside the KOORDHIP_PREEMPT_DEVICE mode. */
int koordhip_preempt_ext(koordhip_ctx *ctx, const koordhip_preemptor *pre, const koordhip_pod_ext *ext, int32_t n_pre,
                         koordhip_preempt_result *out, int32_t *victims, int32_t max_victims);
int koordhip_preempt_node_verdicts_ext(koordhip_ctx *ctx, const koordhip_preemptor *pre, const koordhip_pod_ext *ext,
                                       koordhip_preempt_node *per_node);

/* ---- sequential preemption dry run (additive to ABI 15: detect it by the symbol)
 * The same dry run for a batch whose answers have to hold together: the
 * preemptors are processed in input order and preemptor k gets the verdicts
 * and the pick of koordhip_preempt on the state S_k the earlier ones left.
 * For every earlier preemptor j that ended with a node c >= 0 and the (full)
 * victim list V_j:
 *   - the pods of V_j are gone: off their nodes' rows, never a potential
 *     victim, no PDB budget consumed in the split;
 *   - j's own pod is on the row of c iff priority_j >= priority_k (upstream's
 *     RunFilterPluginsWithNominatedPods); a nominated pod is never a victim;
 *   - per victim and per bit b of its pdb_mask: allowed[b] = max(0, allowed[b] - 1);
 *   - if quota_k == quota_j >= 0, q_used_k = max(0, q_used_k - sum of qreq of
 *     V_j's KOORDHIP_ASG_IN_QUOTA pods) per dimension.  Every q_used is given
 *     AS OF THE START OF THE CALL; the nominated pod is not added to it.
 * out[k] / victims[k] are those of koordhip_preempt on S_k.  A preemptor that
 * ends with node = -1 changes nothing.  The call writes no engine state and
 * leaves the loaded table as it was; envelope and error codes are those of
 * koordhip_preempt.  One host synchronisation, at the end. */
typedef struct koordhip_preempt_stream_stats {
  int64_t full_recomputes;  /* preemptors for which a changed PDB budget / freed quota made every 256-node block evaluate again */
  int64_t block_recomputes; /* blocks evaluated again, over all preemptors */
  int64_t blocks_skipped;   /* blocks whose evaluation on the loaded state was kept */
} koordhip_preempt_stream_stats;
int koordhip_preempt_stream(koordhip_ctx *ctx, const koordhip_preemptor *pre, int32_t n_pre,
                            koordhip_preempt_result *out /* [n_pre] */,
                            int32_t *victims /* [n_pre][max_victims], may be NULL */, int32_t max_victims,
                            koordhip_preempt_stream_stats *stats /* may be NULL */);
/* The sequential dry run in the KOORDHIP_PREEMPT_DEVICE mode (additive to ABI
 * 15: detect it by the symbol): koordhip_preempt_stream with the preemptors'
 * koordhip_pod_ext records (ext[p] beside pre[p]; NULL: all empty; the same
 * check as koordhip_preempt_ext).  S_k is the state above, extended by what the
 * mode moves:
 *   - a gone pod is also off xrequested[x] by its xreq[x] over its xmask, and
 *     for a call with a device preemptor off its node's devices:
 *     used[t][s][r] -= dev_per[t][r] for every slot s of its dev_slots[t],
 *     before the walk and for the whole of it (the walk's used - Pd starts
 *     lower; free stays max0(total - max0(used - Pd)));
 *   - a nominated pod j with priority_j >= priority_k also has its xreq on
 *     xrequested over its xmask (NodeInfo.AddPod counts a nominated pod's
 *     scalars);
 *   - a nominated pod holds NO devices.  This is the reference's behaviour:
 *     DeviceShare's AddPod looks the pod up in the node's device cache
 *     (deviceshare/plugin.go:201-212), a nominated pod has no allocation there
 *     and the hook returns without touching preemptibleDevices.  Two device
 *     preemptors can therefore be nominated onto the same freed minor; only the
 *     scalars (nvidia.com/gpu, ...) keep them apart.
 * UNRESOLVABLE is the mode's rule on S_k's start row.  For n_pre = 1 the call
 * is koordhip_preempt_ext.  Accepted only in the KOORDHIP_PREEMPT_DEVICE mode
 * (with KOORDHIP_PREEMPT_NUMA_FROZEN or without), ext NULL or not; refused as
 * the mode's other calls are (PodTopologySpread / InterPodAffinity, Reservation
 * state, reserve / operating-mode preemptors, a communicator,
 * KOORDHIP_POD_NUMA_ERROR).  Every preemptor is evaluated on every node (the
 * per-preemptor chain; no block is skipped), so stats is full_recomputes as
 * above, block_recomputes = n_pre * ceil(n / 256), blocks_skipped = 0. */
int koordhip_preempt_stream_ext(koordhip_ctx *ctx, const koordhip_preemptor *pre, const koordhip_pod_ext *ext,
                                int32_t n_pre, koordhip_preempt_result *out /* [n_pre] */,
                                int32_t *victims /* [n_pre][max_victims], may be NULL */, int32_t max_victims,
                                koordhip_preempt_stream_stats *stats /* may be NULL */);
/* The sequential dry run in the KOORDHIP_PREEMPT_RESV mode (additive to ABI 15:
 * detect it by the symbol): koordhip_preempt_stream's inputs, records, victims
 * layout, stats and error codes, on a context with Reservation state.  It is a
 * call of its own because koordhip_preempt_stream keeps its refusal there.  S_k
 * is the state above; for (preemptor k, node) the RESV mode's walk changes so:
 *   - a gone listed pod bound to slot q (KOORDHIP_ASG_RESV_SLOT) has left its
 *     reservation (RemoveAssignedPod, frameworkext/reservation_info.go:308-319):
 *     Allocated[q][c] = max(0, Allocated[q][c] - req[c]) for c in {cpu, memory}
 *     where the slot holds c (KOORDHIP_RESV_KEY_*), the assigned count drops by
 *     one, floored at 0;
 *   - class, restore and the frozen podRequested are those of the lowered
 *     slots: a class-2 slot whose last assigned pod is gone becomes class 0 and
 *     its restore no longer happens; a Restricted slot holds more; rRemained
 *     and the matched Allocated move;
 *   - a slot with KOORDHIP_RESV_ALLOCATE_ONCE that had an assigned pod when the
 *     call began stays class 0 for the whole call (the reference's controller
 *     marks it Succeeded, reservation/controller/controller.go:245-247; the
 *     engine keeps no phase, so this is the rule);
 *   - order at the walk's start: the gone pods come off the row and the slots,
 *     then the restore, then podRequested is frozen (WITHOUT any nominated pod:
 *     nominated pods are not in the snapshot NodeInfo, transformer.go:129), only
 *     then the nominated pods with priority_j >= priority_k go onto the row;
 *     fitsNode's ephemeral-storage and batch amounts are the loaded row's
 *     without the gone pods;
 *   - a nominated pod moves the plugin's state at every fit test (upstream's
 *     addNominatedPods clones the cycle state and runs AddPod, which for a pod
 *     without a reservation-allocated annotation lowers preemptible[node],
 *     plugin.go:270-276): with N the summed requests of the qualifying
 *     nominated pods over the five resources the test reads Pn_eff = max(0, Pn -
 *     N) in place of Pn (present iff some resource is non-zero); the walk's own
 *     Pn and every Pr[q] are untouched; a nominated pod is bound to no slot;
 *   - two passes (RunFilterPluginsWithNominatedPods): on a node with at least
 *     one qualifying nominated pod "P fits" is T(row with them, Pn_eff) and then
 *     T(row without them, Pn); the second can fail where the first passes (a
 *     Default slot is insufficient only while something preemptible is present;
 *     the branch without a matched reservation calls fitsNode only then).
 * UNRESOLVABLE is the RESV mode's rule on S_k's start row with the qualifying
 * nominated pods on it.  For n_pre = 1 the call is koordhip_preempt in the same
 * mode.  Accepted exactly where koordhip_preempt is in the RESV mode: the flag
 * set on a context with Reservation state, with NodeNUMAResource in the Filter
 * KOORDHIP_PREEMPT_NUMA_FROZEN as well, at most KOORDHIP_RESV_SLOTS slots.
 * KOORDHIP_EINVAL (the context stays usable): the flag missing; no Reservation
 * state (the sequential dry run there is koordhip_preempt_stream);
 * KOORDHIP_PREEMPT_DEVICE set; both flags on a resv_cpus snapshot; reserve /
 * operating-mode preemptors; a communicator; a sequential-cycle snapshot.
 * Built as the per-preemptor chain: stats is full_recomputes as above,
 * block_recomputes = n_pre * ceil(n / 256), blocks_skipped = 0. */
int koordhip_preempt_stream_resv(koordhip_ctx *ctx, const koordhip_preemptor *pre, int32_t n_pre,
                                 koordhip_preempt_result *out /* [n_pre] */,
                                 int32_t *victims /* [n_pre][max_victims], may be NULL */, int32_t max_victims,
                                 koordhip_preempt_stream_stats *stats /* may be NULL */);

/* The same split in two so a caller can time the device part alone: stage
 * (host -> HBM copy) then place (HBM-resident pods, result kept on device
 * until koordhip_fetch_placements). */
int koordhip_stage_pods(koordhip_ctx *ctx, const koordhip_pod *pods, int32_t n_pods);
/* ABI 9: stage pods with their koordhip_pod_ext records (ext may be NULL),
 * for koordhip_place_staged on a sequential-cycle profile. */
int koordhip_stage_pods_ext(koordhip_ctx *ctx, const koordhip_pod *pods, const koordhip_pod_ext *ext,
                            int32_t n_pods);
int koordhip_place_staged(koordhip_ctx *ctx);
int koordhip_fetch_placements(koordhip_ctx *ctx, int32_t *out_node, int32_t n_pods);
int koordhip_synchronize(koordhip_ctx *ctx);

/* Device-side checkpoint of the mutable columns (requested / nz / npods /
 * la_used* / flags) and its restore: rolls a whole speculative cycle back
 * (bulk Unreserve) without re-uploading the snapshot. */
int koordhip_checkpoint(koordhip_ctx *ctx);
int koordhip_restore(koordhip_ctx *ctx);

/* Reserve / Unreserve of one pod on one node (state delta only).  For a
 * cpuset pod the NodeNUMAResource Reserve allocates CPUs (the exact
 * cpuAccumulator choice, cpu_accumulator.go:87-232); cpus_out (optional,
 * KOORDHIP_NUMA_WORDS words, core-major positions) receives them, and
 * KOORDHIP_ERESERVE means Allocate failed and nothing was committed.
 * Unreserve of a cpuset pod takes the CPUs it was given. */
int koordhip_commit(koordhip_ctx *ctx, const koordhip_pod *pod, int32_t node, uint64_t *cpus_out);
int koordhip_uncommit(koordhip_ctx *ctx, const koordhip_pod *pod, int32_t node, const uint64_t *cpus);

/* ABI 12: Reserve / Unreserve of one pod WITH its koordhip_pod_ext record on
 * one node -- the same Reserve the sequential cycle runs on its winner:
 *   DeviceShare Reserve   <- deviceshare/plugin.go:368-405 (allocator.go:91-122: the
 *                            device choice; deviceUsed += the per-device request)
 *   DeviceShare Unreserve <- deviceshare/plugin.go:407-426 (deviceUsed -= it)
 *   NodeResourcesFit      <- the extended scalars' Requested (xrequested) +/- xreq
 *   PodTopologySpread / InterPodAffinity <- upstream AddPod / RemovePod of the
 *                            placed pod: pts_cnt / ipa_cnt of the constraints and
 *                            entries it counts for (pts_match, ipa_inc) +/- 1
 * plus everything koordhip_commit does (Fit / LoadAware, NodeNUMAResource,
 * Reservation).  Reserve assumes the cycle ran PreScore (more than one
 * feasible node: a matched reservation is nominated).  dev_slots_out /
 * dev_slots ([KOORDHIP_DEV_TYPES], bit s = device slot s of the type, as
 * koordhip_fetch_devices): what Reserve took, what Unreserve returns.
 * KOORDHIP_ERESERVE: Reserve failed and nothing was applied.  Unreserve is
 * refused (KOORDHIP_EINVAL) where koordhip_uncommit is. */
int koordhip_commit_ext(koordhip_ctx *ctx, const koordhip_pod *pod, const koordhip_pod_ext *ext, int32_t node,
                        uint64_t *cpus_out, uint32_t *dev_slots_out);
int koordhip_uncommit_ext(koordhip_ctx *ctx, const koordhip_pod *pod, const koordhip_pod_ext *ext, int32_t node,
                          const uint64_t *cpus, const uint32_t *dev_slots);

/* CPUs allocated to each pod of the last place call ([n_pods][KOORDHIP_NUMA_WORDS],
 * zero for non-cpuset pods): what PreBind writes into the resource-status
 * annotation (plugin.go:425-453). */
int koordhip_fetch_cpusets(koordhip_ctx *ctx, uint64_t *cpus, int32_t n_pods);

/* Device-time of the last place call's eval kernels, split for roofline
 * accounting: total ms of eval kernels, launches, evals processed. */
int koordhip_last_stats(koordhip_ctx *ctx, double *eval_ms, int64_t *eval_launches, int64_t *evals,
                        double *total_ms);

/* Per-kernel device time of the last place call (profile_kernels = 1: HIP
 * event pairs on the stream each kernel is launched on): the evaluation
 * (k_scan), the top-k selection (k_select_split) and the
 * sequential resolve (k_resolve; one persistent launch per call unless the
 * context is in a local group).  Roofline accounting in bench.py. */
typedef struct koordhip_kernel_stats {
  /* *_ms / *_launches: the timed launches only -- a persistent pipeline times
   * the evaluation launches of ~256 evenly spaced rounds (their averages are
   * what the sample is for); `rounds` counts every round */
  double scan_ms;
  int64_t scan_launches;
  double select_ms;
  int64_t select_launches;
  double resolve_ms;
  int64_t resolve_launches;
  double total_ms;   /* the place call, first to last event on the engine stream */
  int64_t evals;     /* (pod, node) pairs evaluated by this rank */
  int64_t pods;      /* pods of the staged stream */
  int64_t rounds;    /* pipelined rounds */
  int64_t round_pods; /* pods per round (batch_pods, LDS-clamped) */
  int64_t lag;        /* pipeline depth: round r's lists see the state after round r - 1 - lag */
  int64_t executed_evals; /* (pod, node) evaluations actually run: class-list builds + incremental
                            * re-evaluations + device pods' pre-evaluations and final re-evaluations
                            * (evals is the equivalent work: every pair decided exactly) */
  int32_t plan_us;        /* host time of the class-list plan of the call */
  int32_t flags;          /* KOORDHIP_KSTAT_LOCAL: a sharded rank ran the full table (no exchange) */
} koordhip_kernel_stats;
#define KOORDHIP_KSTAT_LOCAL 1
int koordhip_last_kernel_stats(koordhip_ctx *ctx, koordhip_kernel_stats *out);
/* Turn the per-launch event timing on / off for later place calls (the
 * events cost a few microseconds per round: bench.py times its steps with it
 * off and takes the per-kernel split from one extra step). */
int koordhip_set_profile_kernels(koordhip_ctx *ctx, int32_t on);
/* The template instantiations the last place call launched for its evaluation
 * (k_scan / k_eval_topk) and its resolve, spelled as rocprofv3 names them
 * ("kh::k_scan<4, 0>"), NUL-terminated in buffers of `cap` bytes -- so a
 * profile can be matched to the exact kernel a timed run used. */
int koordhip_last_kernel_names(koordhip_ctx *ctx, char *eval_out, char *resolve_out, int32_t cap);

/* ---- multi-GPU (node-index sharding, RCCL all-gather of per-shard top-k) -- */
#define KOORDHIP_UNIQUE_ID_BYTES 128
int koordhip_comm_unique_id(uint8_t *id_out /* KOORDHIP_UNIQUE_ID_BYTES */);
/* Attach an RCCL communicator: this context then evaluates only node shard
 * [rank*n/world, (rank+1)*n/world) and merges per-shard top-k over xGMI.
 * world == 1 attaches a one-rank communicator: the whole table, through the
 * same per-round all-gather + merge path (lag 1, one evaluation stream). */
int koordhip_comm_init(koordhip_ctx *ctx, const uint8_t *id, int32_t world, int32_t rank);
/* The same sharding for `world` contexts driven by ONE process (one host
 * thread per context, e.g. one scheduler process owning several GPUs, or
 * several contexts on one GPU): ctxs[r] becomes rank r and the per-round
 * exchange is a device-to-device copy instead of RCCL.  The contexts'
 * place_staged / place_stream calls must then run concurrently with the same
 * pod stream, as collective calls. */
int koordhip_comm_init_local(koordhip_ctx **ctxs, int32_t world);

#ifdef __cplusplus
}
#endif

#endif /* KOORDHIP_H */
