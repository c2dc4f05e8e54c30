// preempt.h -- launch wrappers of preempt.hip (host side): the preemption dry
// run, SelectVictimsOnNode on every node and the candidate pick on device.
#pragma once
#include <hip/hip_runtime.h>

#include "eval.hpp"

namespace kh {

// Device copy of one koordhip_assigned (quantities of the pod as exact f64).
struct DevAsg {
  DevPod pod;
  int64_t start;
  int64_t qreq[KOORDHIP_PREEMPT_QRES];
  int32_t prio, quota;
  uint32_t flags, pdb_mask;
  int32_t idx;  // index into the caller's table
  int32_t node;
};
static_assert(sizeof(DevAsg) == 160 && sizeof(DevAsg) % 16 == 0, "DevAsg is 160 bytes");
// DevAsg::flags bit the library sets (a caller's bit there is dropped): the pod's record of the second table
// (DevAsgX) is not empty.  A walk reads that table for such records only.
constexpr uint32_t ASG_HAS_EXT = 4u;

// Device copy of one koordhip_assigned_ext (same layout): what a listed pod holds of the extended scalars and
// of its node's devices.  The second table is permuted with the first, so list[k]'s record is xlist[k].
struct DevAsgX {
  int64_t xreq[KOORDHIP_NXRES];
  int64_t dev_per[KOORDHIP_DEV_TYPES][KOORDHIP_DEV_RES];
  uint32_t dev_slots[KOORDHIP_DEV_TYPES];
  uint32_t xmask;
  uint64_t reserved;
};
static_assert(sizeof(DevAsgX) == sizeof(koordhip_assigned_ext) && sizeof(DevAsgX) == sizeof(DevAsg),
              "DevAsgX mirrors koordhip_assigned_ext and permutes like DevAsg");

// Device copy of one koordhip_preemptor.
struct DevPre {
  DevPod pod;
  int64_t used[KOORDHIP_PREEMPT_QRES], runtime[KOORDHIP_PREEMPT_QRES], req[KOORDHIP_PREEMPT_QRES];
  int32_t prio, quota;
  uint32_t qmask, pad;
};
static_assert(sizeof(DevPre) == 208, "DevPre is 208 bytes");

struct PdbAllowed {
  int32_t a[KOORDHIP_PREEMPT_PDBS];
};

// One workgroup's best candidate of one preemptor (node -1: none): the
// verdict's own fields are the pick's key.
struct PreemptPartial {
  koordhip_preempt_node v;
  int32_t node, pad;
};
static_assert(sizeof(PreemptPartial) == 40, "partials are 40 bytes");

constexpr int PREEMPT_THREADS = 256;
inline int32_t preempt_blocks(int32_t n) { return (n + PREEMPT_THREADS - 1) / PREEMPT_THREADS; }

// The node-sorted table: node i's pods are sorted[off[i] .. off[i + 1]) in list
// order (priority descending, start ascending, input index ascending).
//   raw [m] the records in input order; sorted [m] the permuted copy
//   ws  int32 workspace of preempt_ws_ints(n, m) words: cnt [n + 1], off [n + 1], nl [m], tot [1]
size_t preempt_ws_ints(int32_t n, int32_t m);
inline int32_t *preempt_off(int32_t *ws, int32_t n) { return ws + n + 1; }
// xraw / xsorted: the second table (DevAsgX, NULL: none), permuted by the same order.
hipError_t launch_preempt_lists(const DevAsg *raw, DevAsg *sorted, int32_t m, int32_t n, int32_t *ws, hipStream_t s,
                                const void *xraw = nullptr, void *xsorted = nullptr);

// The DEVICE mode's inputs of a dry-run call (m.dev > 0; empty otherwise): the permuted second table (NULL: no
// listed pod holds a scalar or a device) and the preemptors' koordhip_pod_ext records.
struct DevWalk {
  const DevAsgX *xtab;
  const void *px;  // DevPodX [n_pre] (dev.hpp)
};

// Which walk a dry-run call runs: what the profile / snapshot holds and what
// koordhip_preempt_set_mode's flags accepted of it.  The launchers pick their
// kernels' instantiation from numa and rs alone.
struct WalkMode {
  bool numa;  // NodeNUMAResource is in the Filter and the host accepted the frozen verdict: the walk reads the plane
  bool resv;  // the context has Reservation state (the Filter plugin or reservation columns) ...
  int rs;     // ... and the host accepted the walk that keeps the plugin's AddPod / RemovePod state: the
              // reservation slots per row (1, or KOORDHIP_RESV_SLOTS where the snapshot's resv_slots ask), else 0
  bool devp;  // DeviceShare is in the profile (Filter or Score) ...
  int dev;    // ... and the host accepted the walk that moves the victims' extended scalars (1) and, for a call
              // with a device preemptor, their devices (2: the launchers' callers raise 1 to 2 per call); else 0
  bool both;  // rs > 0 and dev > 0, and the host accepted the walk that keeps both plugins' state
              // (KOORDHIP_PREEMPT_DEVICE_RESV): without it a mode with both is refused
};
inline WalkMode preempt_walk_mode(const DevCfg &c, uint32_t pre_mode) {
  WalkMode m{};
  m.numa = (pre_mode & KOORDHIP_PREEMPT_NUMA_FROZEN) && (c.filt & KOORDHIP_PLUGIN_NUMA);
  m.resv = c.resv || (c.filt & KOORDHIP_PLUGIN_RESERVATION);
  m.rs = (pre_mode & KOORDHIP_PREEMPT_RESV) && m.resv ? (c.resv_slots > 1 ? KOORDHIP_RESV_SLOTS : 1) : 0;
  m.devp = ((c.filt | c.score) & KOORDHIP_PLUGIN_DEVICESHARE) != 0;
  m.dev = (pre_mode & KOORDHIP_PREEMPT_DEVICE) && m.devp ? 1 : 0;
  m.both = (pre_mode & KOORDHIP_PREEMPT_DEVICE_RESV) && m.rs > 0 && m.dev > 0;
  return m;
}

// The dry run of pre[0, n_pre) on the current rows.  count [n_pre][5] (zeroed by
// the caller) receives the nodes per status, part [n_pre][preempt_blocks(n)]
// the workgroups' best candidates; per_node (n_pre = 1 only, may be NULL) every
// node's verdict.  m: the context's preempt_walk_mode; the call is refused
// unless it covers every state the profile has.  plane: with m.numa the words
// launch_preempt_numa wrote for these preemptors (the walk then reads the
// plugin's verdict there and evaluates filterAmplifiedCPUs on every row), else
// NULL.  With m.rs the walk starts from the restored row and keeps the plugin's
// AddPod / RemovePod state; DevAsg::flags bits 8-11 name the slot a listed pod
// is bound to.  With m.dev the walk moves the listed pods' extended scalars
// (1) and devices (2) as dw describes them; beside m.rs only with m.both, the
// walk that keeps both states (k_preempt_dev_resv).
hipError_t launch_preempt(const DevCfg &c, const DevNodes &d, const DevAsg *tab, const int32_t *off,
                          const PdbAllowed &pdb, const DevPre *pre, int32_t n_pre, int32_t *count,
                          PreemptPartial *part, koordhip_preempt_node *per_node, const uint64_t *plane, WalkMode m,
                          hipStream_t s, DevWalk dw = DevWalk{});
// The frozen NUMA verdict plane of pre[0, n_pre): plane [n_pre][2][ceil(n / 64)]
// u64 (preempt_plane_words), bit b of word w is node 64 w + b; [p][0]: the
// NodeNUMAResource Filter without filterAmplifiedCPUs fails on the loaded NUMA
// row, [p][1]: with one of KOORDHIP_REASON_UNRESOLVABLE_MASK's reasons.
size_t preempt_plane_words(int32_t n, int32_t n_pre);
hipError_t launch_preempt_numa(const DevCfg &c, const DevNodes &d, const DevPre *pre, int32_t n_pre, uint64_t *plane,
                               hipStream_t s);
// part -> res[p].node / best (count is copied in), then the chosen nodes'
// victims [n_pre][max_victims], -1 padded (victims may be NULL).  m: launch_preempt's.
hipError_t launch_preempt_pick(const DevCfg &c, const DevNodes &d, const DevAsg *tab, const int32_t *off,
                               const PdbAllowed &pdb, const DevPre *pre, int32_t n_pre, const int32_t *count,
                               const PreemptPartial *part, koordhip_preempt_result *res, int32_t *victims,
                               int32_t max_victims, WalkMode m, hipStream_t s, DevWalk dw = DevWalk{});

// ---- the sequential dry run (koordhip_preempt_stream) ----------------------
// Preemptor k is answered on the state the preemptors before it left: their
// victims gone, they themselves nominated on their nodes, the PDB budgets and
// their quotas' used lowered.  All of it lives in the call's own buffers.

// One nominated preemptor on its node's overlay list (entry k is preemptor k's).
struct NomEntry {
  DevPod pod;
  int32_t prio, next;  // next entry of the same node, -1: none
};
static_assert(sizeof(NomEntry) == 104, "NomEntry is 104 bytes");

struct StreamFlags {
  int32_t pdb;   // the budgets differ from the loaded ones
  int32_t full;  // KOORDHIP_PREEMPT_STREAM_FULL: every block evaluates every preemptor again
};

// The call's device state.  The caller clears gone, freed, touched, qflag and
// stats and sets head and victims to -1 before launch_preempt_stream, which
// writes pdb and flags itself; the rest is written before it is read.
struct StreamState {
  PreemptPartial *part;   // [n_pre][nb]    a block's best candidate
  int32_t *bcnt;          // [n_pre][nb][5] a block's nodes per status
  koordhip_preempt_result *res;  // [n_pre]
  uint64_t *gone;         // [n][2] bit k: position k of the node's list is gone
  NomEntry *nom;          // [n_pre]
  int32_t *head;          // [n] first overlay entry of the node, -1: none
  PdbAllowed *pdb;        // the current budgets
  int64_t *freed;         // [n_pre][QRES] what earlier preemptors of the same quota freed
  int32_t *touched;       // [nb] the block's rows / lists differ from the loaded state
  int32_t *qflag;         // [n_pre] freed[k] is not zero
  StreamFlags *flags;
  koordhip_preempt_stream_stats *stats;
  int32_t *vpos;          // [KOORDHIP_PREEMPT_NODE_PODS] the chosen node's victims as list positions
  int32_t *victims;       // [n_pre][max_victims], -1 filled (may be NULL)
};

// Phase 1 (the preemptors on the loaded state, per-block partials and counts,
// a tile of 32 at a time) and per preemptor k: k_preempt_seq (the blocks that
// have to evaluate k again), k_preempt_seq_pick, k_preempt_apply.  full: the
// A/B knob, every block evaluates every preemptor again.  plane, m: as for
// launch_preempt, the plane written once before the first preemptor.  With
// m.rs > 0 (koordhip_preempt_stream_resv) the walk carries the node's
// reservation slots, lowered per walk by the gone positions' records, and the
// call is built as the per-preemptor chain only: no phase 1, `full` forced,
// the stats those of launch_preempt_stream_dev.  Nothing synchronises.
hipError_t launch_preempt_stream(const DevCfg &c, const DevNodes &d, const DevAsg *tab, const int32_t *off,
                                 const PdbAllowed &pdb, const DevPre *pre, int32_t n_pre, const StreamState &st,
                                 int32_t max_victims, bool full, const uint64_t *plane, WalkMode m, hipStream_t s);
// ... in the DEVICE mode (koordhip_preempt_stream_ext; m.dev 1 or 2, dw as for launch_preempt): the same state
// and the same answers' layout, built as the per-preemptor chain only: k_preempt_seq_dev on every block,
// k_preempt_seq_pick, k_preempt_apply_dev.  A gone pod's scalars and devices are read off its second-table
// record by every later walk; NomEntry k is preemptor k's, whose scalars are dw.px[k]'s.  The stats are those of
// the chain: block_recomputes = n_pre * blocks, blocks_skipped = 0, full_recomputes as in the plain stream.
hipError_t launch_preempt_stream_dev(const DevCfg &c, const DevNodes &d, const DevAsg *tab, const int32_t *off,
                                     const PdbAllowed &pdb, const DevPre *pre, int32_t n_pre, const StreamState &st,
                                     int32_t max_victims, const uint64_t *plane, WalkMode m, hipStream_t s, DevWalk dw);

}  // namespace kh
