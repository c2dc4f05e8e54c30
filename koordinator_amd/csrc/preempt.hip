// preempt.hip -- the preemption dry run: elasticquota's SelectVictimsOnNode
// (preempt.go:111-215) on every node and the pick of one candidate
// (upstream pickOneNodeForPreemption), against the current rows.  Nothing
// here writes engine state.
//
//   k_pre_count / (k_diag_scan) / k_pre_fill / k_pre_sort / k_pre_permute
//                     the node-sorted table: per node its assigned pods, each
//                     list ordered by MoreImportantPod then input index, and a
//                     permuted COPY of the records so that a thread's list is
//                     one contiguous run of 160-B records (no index gather in
//                     the hot kernel).
//   k_preempt<NUMA, RS>
//                     256-node tiles x preemptor tiles; the tile's preemptors
//                     are staged in LDS, a thread loads its node row once and
//                     copies it per preemptor.  The walk over a node's list
//                     diverges, the loop over preemptors does not: per
//                     preemptor the wave counts the statuses with ballots and
//                     reduces the pick's key with shuffles, the workgroup
//                     writes ONE partial (the best candidate's verdict) per
//                     preemptor.  No 128-bit key ever meets a global atomic.
//   k_preempt_pick    one wave per preemptor over the workgroups' partials.
//   k_preempt_numa    the NUMA mode's pre-pass: the NodeNUMAResource Filter of
//                     every (preemptor, node) on the loaded NUMA rows, two bits
//                     per pair (fails / fails unresolvably), written as one
//                     ballot word per wave.  The plugin has no
//                     PreFilterExtensions, so the verdict holds for the whole
//                     call; the NUMA instantiations are the walk reading it.
//   k_preempt_victims<NUMA, RS>
//                     one thread per preemptor re-runs its chosen node and
//                     writes the victims in the reference's append order.
//   k_preempt_dev<NUMA, DEV> / k_preempt_dev_resv<NUMA, RS, DEV> (and their _victims kernels)
//                     k_preempt / k_preempt_victims in the DEVICE mode, without
//                     and with Reservation state: kernels of their own, so that
//                     the others keep their argument lists and code.
//   k_preempt_blk<NUMA> / k_preempt_seq<NUMA, RS> / k_preempt_seq_pick / k_preempt_apply<NUMA, RS>
//                     the sequential dry run (koordhip_preempt_stream): the
//                     preemptors in input order, each on the state the earlier
//                     ones left (victims gone, preemptors nominated, budgets
//                     and quota lowered), all of it in the call's own buffers.
//                     k_preempt_blk is k_preempt keeping per-block counts; per
//                     preemptor only the blocks something changed for
//                     evaluate again, one wave picks, one wave re-runs the
//                     chosen node and applies it.
//
// The five walk kernels are templates on what preempt.h's WalkMode says of the
// call, and with_walk below is the one place a WalkMode becomes template
// arguments.  NUMA: NodeNUMAResource is in the Filter, the walk reads
// k_preempt_numa's plane (the kernels that read verdicts take a NumaPlane, empty
// without NUMA).  RS > 0: Reservation state (KOORDHIP_PREEMPT_RESV): the walk
// starts from the row after the cycle's restore for the preemptor and keeps
// the plugin's AddPod / RemovePod state (preemptible, preemptibleInRRs:
// resv.hpp ResvPre) per (preemptor, node) in registers; RS = 1 or
// KOORDHIP_RESV_SLOTS reservation slots per node.  In the stream
// (koordhip_preempt_stream_resv) k_preempt_seq / k_preempt_apply take the same
// RS, run as the chain without phase 1: a walk lowers its copy of the slots by
// the gone pods and runs both passes of RunFilterPluginsWithNominatedPods on a
// node with a nominated pod (preempt_node, OVL with RS > 0).
// DEV > 0 (KOORDHIP_PREEMPT_DEVICE): the
// listed pods' extended scalars move with them (1), and for a call with a
// device preemptor so do their devices (2): DeviceShare's preemptibleDevices
// per (preemptor, node) as used - Pd in LDS, one column per thread.  In the
// stream (koordhip_preempt_stream_ext) these are kernels of their own,
// k_preempt_seq_dev<NUMA, DEV> / k_preempt_apply_dev<NUMA, DEV>, the chain
// without phase 1; k_preempt_seq_pick is shared.
// RS > 0 and DEV > 0 (KOORDHIP_PREEMPT_DEVICE_RESV):
// k_preempt_dev_resv<NUMA, RS, DEV> / k_preempt_victims_dev_resv<NUMA, RS, DEV>
// over the same tiles and the same walk: the Reservation maps carry the listed
// pods' extended scalars (resv.hpp ResvPre<S, true>), fitsNode tests the
// preemptor's, and a victim bound to a slot frees no device.  Not in a stream.
//
// Thread-per-node, not wave-per-node: a node's walk is a chain (every Filter
// reads the row the previous add / remove left), so a wave would hold 63 idle
// lanes per step; with a thread per node the chain's steps of 64 nodes issue
// together and the records stream through L2 one contiguous run per lane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "dev.hpp"
#include "diag.h"
#include "eval.hpp"
#include "preempt.h"

namespace kh {

constexpr int PRE_PT = 32;  // preemptors per LDS tile
constexpr int PRE_WORDS = (int)(sizeof(DevPre) / sizeof(uint64_t));
constexpr int PRE_WAVES = PREEMPT_THREADS / 64;
constexpr int ASG_VEC = (int)(sizeof(DevAsg) / sizeof(uint4));
static_assert(sizeof(DevPre) % sizeof(uint64_t) == 0, "preemptor records are staged as 8-B words");
static_assert(KOORDHIP_PREEMPT_NODE_PODS == 128, "a node's potential / violating sets are two 64-bit masks");

// ---------------------------------------------------------------------------
// the node-sorted table

__global__ void k_pre_count(const DevAsg *__restrict__ raw, int32_t m, int32_t n, int32_t *__restrict__ cnt) {
  const int32_t j = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= m) return;
  const int32_t node = raw[j].node;
  if (node >= 0 && node < n) atomicAdd(&cnt[node], 1);
}

__global__ void k_pre_fill(const DevAsg *__restrict__ raw, int32_t m, int32_t n, const int32_t *__restrict__ off,
                           int32_t *__restrict__ cur, int32_t *__restrict__ nl) {
  const int32_t j = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= m) return;
  const int32_t node = raw[j].node;
  if (node >= 0 && node < n) nl[off[node] + atomicAdd(&cur[node], 1)] = j;
}

// MoreImportantPod, then the input index (the engine's rule where Go's unstable sort has none)
__device__ __forceinline__ bool list_before(int32_t pa, int64_t sa, int32_t ia, int32_t pb, int64_t sb, int32_t ib) {
  if (pa != pb) return pa > pb;
  if (sa != sb) return sa < sb;
  return ia < ib;
}

// each node's list into list order (the fill's order is arbitrary; lists hold 128 entries at most)
__global__ void k_pre_sort(const DevAsg *__restrict__ raw, const int32_t *__restrict__ off, int32_t *__restrict__ nl,
                           int32_t n) {
  const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const int32_t lo = off[i], hi = off[i + 1];
  for (int32_t a = lo + 1; a < hi; a++) {
    const int32_t x = nl[a];
    const int32_t px = raw[x].prio;
    const int64_t sx = raw[x].start;
    int32_t b = a;
    for (; b > lo; b--) {
      const int32_t y = nl[b - 1];
      if (!list_before(px, sx, x, raw[y].prio, raw[y].start, y)) break;
      nl[b] = y;
    }
    nl[b] = x;
  }
}

// sorted[j] = raw[nl[j]], 16 bytes per thread
__global__ void k_pre_permute(const DevAsg *__restrict__ raw, DevAsg *__restrict__ sorted,
                              const int32_t *__restrict__ nl, int32_t m) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (int64_t)m * ASG_VEC) return;
  const int32_t j = (int32_t)(g / ASG_VEC), k = (int32_t)(g - (int64_t)j * ASG_VEC);
  reinterpret_cast<uint4 *>(sorted)[g] = reinterpret_cast<const uint4 *>(raw)[(int64_t)nl[j] * ASG_VEC + k];
}

// ---------------------------------------------------------------------------
// one (preemptor, node)

// a is picked before b (na / nb: their nodes, -1 = no candidate)
__device__ __forceinline__ bool pick_before(const koordhip_preempt_node &a, int32_t na, const koordhip_preempt_node &b,
                                            int32_t nb) {
  if (na < 0) return false;
  if (nb < 0) return true;
  const bool za = a.n_victims == 0, zb = b.n_victims == 0;
  if (za != zb) return za;  // a node that needs no victim wins outright
  if (a.n_pdb_violations != b.n_pdb_violations) return a.n_pdb_violations < b.n_pdb_violations;
  if (a.top_priority != b.top_priority) return a.top_priority < b.top_priority;
  if (a.sum_priority != b.sum_priority) return a.sum_priority < b.sum_priority;
  if (a.n_victims != b.n_victims) return a.n_victims < b.n_victims;
  if (a.earliest_start != b.earliest_start) return a.earliest_start > b.earliest_start;  // the latest start wins
  return na < nb;
}

struct QuotaUsed {
  int64_t u[KOORDHIP_PREEMPT_QRES];
};

// RemovePod / AddPod of one listed pod: the row and, for a pod the quota
// counts, the quota's used (SubtractWithNonNegativeResult / Add, plugin.go:296-305)
__device__ __forceinline__ void move_pod(NV &w, QuotaUsed &q, const DevAsg &a, int sign) {
  apply_delta(w, a.pod, sign);
  if (a.flags & KOORDHIP_ASG_IN_QUOTA) {
#pragma unroll
    for (int r = 0; r < KOORDHIP_PREEMPT_QRES; r++)
      q.u[r] = sign > 0 ? q.u[r] + a.qreq[r] : (q.u[r] > a.qreq[r] ? q.u[r] - a.qreq[r] : 0);
  }
}

// What the sequential dry run lays over one node: the list positions that are
// gone and the node's nominated preemptors (entries of nom chained from head).
struct NodeOverlay {
  uint64_t g0, g1;
  const NomEntry *nom;
  int32_t head;
};

constexpr int EMIT_NONE = 0, EMIT_IDX = 1, EMIT_POS = 2;

// SelectVictimsOnNode of preemptor P on the node whose row is v and whose
// listed pods are list[0, len).  EMIT_IDX: the victims' table indices go to
// vout[0, vmax) in append order; EMIT_POS: their list positions.  OVL: on the
// row without the gone pods and with the nominated pods of P's priority and
// above, over the list without the gone positions.  NUMA: NodeNUMAResource is
// in the Filter; fcode is the frozen verdict of its Filter without
// filterAmplifiedCPUs (NUMA_F_*, 0: passes), which moves with the row and is
// part of every fit test here (of nr it reads cls, cnt and amp).
//
// RS > 0 (KOORDHIP_PREEMPT_RESV): the context has Reservation state, nr holds
// the node's RS reservation slots.  The walk starts from the row after the
// cycle's restore for P (the reference's PostFilter runs on the NodeInfo
// BeforePreFilter restored), the slots and nodeRState.podRequested stay as they
// are and every move of a listed pod also moves the plugin's AddPod /
// RemovePod state (resv.hpp ResvPre), which filterWithReservations reads in
// every fit test.
//
// OVL with RS > 0 (koordhip_preempt_stream_resv), in this order: the gone pods come off the row
// and off the walk's copy of the slots (resv_unassign); the restore and the frozen podRequested are those of the
// lowered slots, taken before any nominated pod is on the row; then the nominated pods of P's priority and above
// join the row.  On a node with such a pod every fit test is RunFilterPluginsWithNominatedPods' two passes: the row
// with them and preemptible[node] lowered by their requests (AddPod on the cloned state), then the row without
// them (NomSum) and the walk's own state.
constexpr uint32_t NUMA_F_FAIL = 1u, NUMA_F_UNRESOLVABLE = 2u;

// What a node's qualifying nominated pods add to its row, summed (n: how many), so that the second pass can
// take them off again.  Every amount is an integer below 2^53 held as f64: the sums are exact in any order.  (The
// LoadAware estimates apply_delta also moves are not kept: the Filter reads the row's threshold bits, never them.)
struct NomSum {
  double r[KOORDHIP_NRES];
  double nz_cpu, nz_mem;
  int32_t n;
};

__device__ __forceinline__ void nom_add(NomSum &s, const DevPod &p) {
#pragma unroll
  for (int k = 0; k < KOORDHIP_NRES; k++) s.r[k] += p.req[k];
  s.nz_cpu += p.nz_cpu_m;
  s.nz_mem += p.nz_mem;
  s.n++;
}

// apply_delta(-1) of all of them at once, for a Filter
__device__ __forceinline__ void nom_off(NV &v, const NomSum &s) {
#pragma unroll
  for (int k = 0; k < KOORDHIP_NRES; k++) v.r[k] -= s.r[k];
  v.nz_cpu -= s.nz_cpu;
  v.nz_mem -= s.nz_mem;
  v.npods -= s.n;
  uint32_t f = v.flags & ~(NF_OVER_CPU | NF_OVER_MEM | NF_OVER_EPH);
  if (v.r[KOORDHIP_RES_CPU] > v.a[KOORDHIP_RES_CPU]) f |= NF_OVER_CPU;
  if (v.r[KOORDHIP_RES_MEM] > v.a[KOORDHIP_RES_MEM]) f |= NF_OVER_MEM;
  if (v.r[KOORDHIP_RES_EPH] > v.a[KOORDHIP_RES_EPH]) f |= NF_OVER_EPH;
  v.flags = f;
}

template <int RS>
using WalkRow = NumaRowRS<(RS > 0 ? RS : 1)>;

// the reservation slot of its node a listed pod is bound to, -1: none
__device__ __forceinline__ int asg_slot(const DevAsg &a) { return (int)((a.flags >> 8) & 15u) - 1; }

// What the DEVICE mode adds to one (preemptor, node): the node's device columns, the list's second table, P's
// koordhip_pod_ext record and the thread's column of the walk's device state (DEV = 2): u[((t * DS + s) * DR
// + r) * stride] is used - Pd of slot s of type t, kept for the types P requests.
struct DevSide {
  const DevDev *dv;
  const DevAsgX *xlist;
  const DevPodX *x;
  int64_t *u;
  int32_t stride;
  int32_t i, n;
  const DevPodX *px;  // the call's records (the stream: nominated preemptor e's scalars are px[e]'s; else NULL)
};

__device__ __forceinline__ int64_t &dev_u(const DevSide &ds, int t, int s, int r) {
  return ds.u[(size_t)((t * DS + s) * DR + r) * ds.stride];
}

// The DeviceShare Filter of a device preemptor on a nodeDevice node with the walk's preemptible devices
// (plugin.go:284-323 with preemptible, device_cache.go:316-365): dev_eval's rule with the free amounts of a
// slot taken as max0(total - max0(used - Pd)) (calcFreeWithPreemptible, :454-482; with Pd = 0 that is
// deviceFree, so the one formula serves the minors the map does not list).  tm: the types P requests.
__device__ __forceinline__ bool dev_filter_pre(const DevSide &ds, uint32_t tm) {
  const DevDev &dv = *ds.dv;
  bool ok = true;
#pragma unroll 1
  for (int t = 0; t < DT; t++) {
    if (!((tm >> t) & 1u)) continue;
    int64_t q[DR];
    dev_requests(*ds.x, t, q);
    DevRow w;
    const size_t a0 = dev_at(dv, ds.i, t, 0);
#pragma unroll
    for (int s = 0; s < DS; s++) {
      const bool on = s < dv.slots;
      w.minor[s] = on ? dv.minor[a0 + s] : -1;
#pragma unroll
      for (int r = 0; r < DR; r++) {
        const int64_t tt = on ? dv.total[(a0 + s) * DR + r] : 0;
        const int64_t uu = on ? dev_u(ds, t, s, r) : 0;
        const int64_t f = tt - (uu > 0 ? uu : 0);
        w.tot[s][r] = tt;
        w.fr[s][r] = f > 0 ? f : 0;
      }
    }
    if (!dev_has_type(w) || (t == KOORDHIP_DEV_GPU && !dev_fill_gpu(w, q))) {
      ok = false;
      continue;
    }
    int64_t per[DR];
    const int64_t want = dev_wanted(t, q, per);
    int64_t cnt = 0;
#pragma unroll
    for (int s = 0; s < DS; s++) cnt += (w.minor[s] >= 0 && !dev_zero(w.fr[s]) && dev_fits(per, w.fr[s])) ? 1 : 0;
    ok &= cnt >= want;
  }
  return ok;
}

// some pod of the list is a potential victim of P
template <bool OVL>
__device__ __forceinline__ bool any_potential(const DevAsg *__restrict__ list, int32_t len, const NodeOverlay &ov,
                                              int32_t pprio, int32_t pquota) {
  bool any = false;
  for (int32_t k = 0; k < len && !any; k++) {
    if constexpr (OVL) {
      if (((k < 64 ? ov.g0 : ov.g1) >> (k & 63)) & 1ull) continue;
    }
    const DevAsg &a = list[k];
    any = !((a.flags & KOORDHIP_ASG_NONPREEMPTIBLE) || a.prio >= pprio || a.quota != pquota);
  }
  return any;
}

//
// DEV > 0 (KOORDHIP_PREEMPT_DEVICE; ds): NodeResourcesFit also tests P's extended scalars on xrequested, which
// moves with every listed pod that holds some (its DevAsgX record, read for ASG_HAS_EXT records only).  DEV = 2:
// and for a device preemptor on a nodeDevice node every move of a listed pod moves the devices it holds into /
// out of preemptibleDevices, which the DeviceShare Filter of every fit test frees (dev_filter_pre).
// With OVL (koordhip_preempt_stream_ext): a gone pod's scalars are off xrequested and its devices off used for
// the whole walk; a nominated preemptor of P's priority and above has its scalars on xrequested (ds.px) and
// holds no device.
template <int EMIT, bool OVL, bool NUMA, int RS = 0, int DEV = 0>
__device__ __forceinline__ koordhip_preempt_node preempt_node(const DevCfg &c, const DevNumaClass *classes, const NV &v,
                                                              const WalkRow<RS> &nr, const DevAsg *__restrict__ list,
                                                              int32_t len, const PdbAllowed &pdb, const DevPre &P,
                                                              int32_t *vout, int32_t vmax, const NodeOverlay &ov,
                                                              uint32_t fcode, const DevSide &ds = DevSide{}) {
  static_assert(!(OVL && RS > 0 && DEV > 0), "the sequential dry run: not under DeviceShare beside Reservation state");
  constexpr bool SEQ_RS = OVL && RS > 0;  // koordhip_preempt_stream_resv
  constexpr bool BOTH = RS > 0 && DEV > 0;  // KOORDHIP_PREEMPT_DEVICE_RESV
  koordhip_preempt_node r{};
  const DevPod pod = P.pod;
  // SEQ_RS: the walk's own copies, v0 the loaded row without the gone pods and sl the slots they have left
  // (elsewhere the caller's, untouched)
  std::conditional_t<SEQ_RS, NV, const NV &> v0 = v;
  std::conditional_t<SEQ_RS, WalkRow<RS>, const WalkRow<RS> &> sl = nr;
  NomSum ns{};
  // xfree[j] = Allocatable - Requested of extended scalar j, for P's scalars (DEV > 0); tm: the device types of P
  // whose preemptible state the walk keeps (DEV = 2; 0: DeviceShare passes whatever is removed)
  int64_t xfree[KOORDHIP_NXRES] = {};
  uint32_t xm = 0u, tm = 0u;
  if constexpr (DEV > 0) {
    xm = (c.filt & KOORDHIP_PLUGIN_FIT) ? ds.x->xmask : 0u;
#pragma unroll
    for (int j = 0; j < KOORDHIP_NXRES; j++)
      if ((xm >> j) & 1u)
        xfree[j] = (ds.dv->xalloc ? ds.dv->xalloc[(size_t)j * ds.n + ds.i] : 0) - ds.dv->xreq[(size_t)j * ds.n + ds.i];
  }
  auto xfit_ok = [&]() {
    bool ok = true;
    if constexpr (DEV > 0) {
#pragma unroll
      for (int j = 0; j < KOORDHIP_NXRES; j++)
        if ((xm >> j) & 1u) ok &= ds.x->xreq[j] <= xfree[j];
    }
    return ok;
  };
  auto dev_ok = [&]() {
    if constexpr (DEV == 2) return tm == 0u || dev_filter_pre(ds, tm);
    return true;
  };
  auto amp_ok = [&](const NV &x) {
    if constexpr (NUMA) return !c.amp || amp_filter_ok(pod, x, nr);
    return true;
  };
  // the Filter without the Reservation plugin (which reads the walk's state: resv_ok below)
  auto base_status = [&](const NV &x) {
    if constexpr (RS > 0) {
      DevCfg cb = c;
      cb.filt &= ~(uint32_t)KOORDHIP_PLUGIN_RESERVATION;
      return filter_status(cb, pod, x, nr, classes, 0, 0u);
    } else {
      return filter_status(c, pod, x, nr, classes, 0, 0u);
    }
  };
  if (base_status(v) & KOORDHIP_ST_STATIC_FAIL) {
    r.status = KOORDHIP_PREEMPT_UNRESOLVABLE;
    return r;
  }
  const int32_t pprio = P.prio, pquota = P.quota;
  NV w = v;
  int nmatch = 0;
  uint32_t mm = 0u;
  ResvPre<(RS > 0 ? RS : 1), BOTH> rp;
  if constexpr (SEQ_RS) {
    // the gone pods come off the row and the slots before the restore: class, restore and podRequested are those
    // of the lowered slots
    for (int h = 0; h < 2; h++) {
      uint64_t g = h ? ov.g1 : ov.g0;
      while (g) {
        const int32_t k = (int32_t)__ffsll((unsigned long long)g) - 1 + 64 * h;
        g &= g - 1;
        if (k >= len) continue;
        apply_delta(v0, list[k].pod, -1);
        resv_unassign(sl, list[k].pod, asg_slot(list[k]));
      }
    }
    w = v0;
  }
  if constexpr (RS > 0) {
    if (c.resv) nmatch = resv_restore(w, sl, pod, mm);
    if constexpr (BOTH) {
      // the restore of cpu / memory-only reservations moves no scalar: podRequested's are the loaded ones
      int64_t xa[KOORDHIP_NXRES], xq[KOORDHIP_NXRES];
#pragma unroll
      for (int j = 0; j < KOORDHIP_NXRES; j++) {
        xa[j] = ds.dv->xalloc ? ds.dv->xalloc[(size_t)j * ds.n + ds.i] : 0;
        xq[j] = ds.dv->xreq ? ds.dv->xreq[(size_t)j * ds.n + ds.i] : 0;
      }
      resv_pre_init(rp, w, sl, pod, mm, xa, xq);
    } else {
      resv_pre_init(rp, w, sl, pod, mm);
    }
  }
  // first: the pass on the row with the nominated pods, whose AddPod lowered the clone's preemptible[node]
  auto resv_ok = [&](const NV &x, bool first = true) {
    if constexpr (RS > 0) {
      if (!(c.filt & KOORDHIP_PLUGIN_RESERVATION)) return true;
      if constexpr (SEQ_RS) {
        if (first) {
          double pe[KOORDHIP_NRES];
#pragma unroll
          for (int k = 0; k < KOORDHIP_NRES; k++) pe[k] = rp.pn[k] > ns.r[k] ? rp.pn[k] - ns.r[k] : 0.0;
          return resv_filter_pre(pod, x, v0, sl, mm, nmatch, rp, pe);
        }
      }
      if constexpr (BOTH)  // fitsNode also tests P's scalars, on the frozen podRequested and the maps' scalars
        return resv_filter_pre(pod, x, v0, sl, mm, nmatch, rp, ds.x->xreq, ds.x->xmask);
      else
        return resv_filter_pre(pod, x, v0, sl, mm, nmatch, rp);
    }
    return true;
  };
  // RunFilterPluginsWithNominatedPods' second pass: the row and the plugin's state without the nominated pods
  auto second_ok = [&]() {
    if constexpr (SEQ_RS) {
      if (ns.n == 0) return true;
      NV x = w;
      nom_off(x, ns);
      return base_status(x) == 0u && amp_ok(x) && resv_ok(x, false);
    }
    return true;
  };
  if constexpr (OVL) {
    for (int h = 0; h < 2 && !SEQ_RS; h++) {
      uint64_t g = h ? ov.g1 : ov.g0;
      while (g) {
        const int32_t k = (int32_t)__ffsll((unsigned long long)g) - 1 + 64 * h;
        g &= g - 1;
        if (k >= len) continue;
        apply_delta(w, list[k].pod, -1);
        if constexpr (DEV > 0) {  // NodeInfo.RemovePod took a gone pod's scalars off Requested as well
          if ((list[k].flags & ASG_HAS_EXT) && xm) {
            const DevAsgX &ax = ds.xlist[k];
#pragma unroll
            for (int j = 0; j < KOORDHIP_NXRES; j++)
              if (((xm & ax.xmask) >> j) & 1u) xfree[j] += ax.xreq[j];
          }
        }
      }
    }
    // (SEQ_RS: the nominated pods only now, the frozen podRequested is the snapshot NodeInfo's, which holds none)
    for (int32_t e = ov.head; e >= 0; e = ov.nom[e].next) {
      if (ov.nom[e].prio < pprio) continue;
      apply_delta(w, ov.nom[e].pod, +1);
      if constexpr (SEQ_RS) nom_add(ns, ov.nom[e].pod);
      if constexpr (DEV > 0) {  // NodeInfo.AddPod counts a nominated pod's scalars (entry e is preemptor e's)
        const DevPodX &nx = ds.px[e];
#pragma unroll
        for (int j = 0; j < KOORDHIP_NXRES; j++)
          if (((xm & nx.xmask) >> j) & 1u) xfree[j] -= nx.xreq[j];
      }
    }
  }
  if constexpr (NUMA) {
    if (fcode) {
      // the first failing plugin in Filter order decides whether preemption might help
      if ((fcode & NUMA_F_UNRESOLVABLE) && base_status(w) == 0u && xfit_ok() && amp_ok(w)) {
        r.status = KOORDHIP_PREEMPT_UNRESOLVABLE;
        return r;
      }
      // no removal changes the verdict: UNFIT with a potential victim, NO_VICTIMS without
      r.status = any_potential<OVL>(list, len, ov, pprio, pquota) ? KOORDHIP_PREEMPT_UNFIT : KOORDHIP_PREEMPT_NO_VICTIMS;
      return r;
    }
  }
  if constexpr (DEV == 2) {
    // the state of the types P requests: used - Pd with Pd empty
    const DevDev &dv = *ds.dv;
    if ((c.filt & KOORDHIP_PLUGIN_DEVICESHARE) && (ds.x->flags & KOORDHIP_PODX_DEVICE) && dev_present(dv, ds.i)) {
#pragma unroll
      for (int t = 0; t < DT; t++) {
        int64_t q[DR];
        if (!dev_requests(*ds.x, t, q)) continue;
        tm |= 1u << t;
        const size_t a0 = dev_at(dv, ds.i, t, 0) * DR;
#pragma unroll
        for (int s = 0; s < DS; s++)
#pragma unroll
          for (int rr = 0; rr < DR; rr++) dev_u(ds, t, s, rr) = s < dv.slots ? dv.used[a0 + (size_t)s * DR + rr] : 0;
      }
    }
    if constexpr (OVL) {
      // the gone pods hold no device any more: used - Pd starts lower, for the whole walk.  A nominated pod holds
      // none either (DeviceShare's AddPod finds no allocation of it in the node's device cache).
      for (int h = 0; h < 2 && tm; h++) {
        uint64_t g = h ? ov.g1 : ov.g0;
        while (g) {
          const int32_t k = (int32_t)__ffsll((unsigned long long)g) - 1 + 64 * h;
          g &= g - 1;
          if (k >= len || !(list[k].flags & ASG_HAS_EXT)) continue;
          const DevAsgX &ax = ds.xlist[k];
#pragma unroll
          for (int t = 0; t < DT; t++) {
            const uint32_t sl = ((tm >> t) & 1u) ? ax.dev_slots[t] : 0u;
            if (!sl) continue;
#pragma unroll
            for (int s = 0; s < DS; s++)
              if ((sl >> s) & 1u)
#pragma unroll
                for (int rr = 0; rr < DR; rr++) dev_u(ds, t, s, rr) -= ax.dev_per[t][rr];
          }
        }
      }
    }
  }
  if constexpr (RS > 0) {
    // a required reservation affinity without a matched reservation (plugin.go:378-381) fails whatever is removed;
    // as the first failing plugin of the start row it is unresolvable
    if ((c.filt & KOORDHIP_PLUGIN_RESERVATION) && nmatch == 0 && (pod.flags & KOORDHIP_POD_RESV_AFFINITY)) {
      bool first = base_status(w) == 0u && amp_ok(w);
      // DeviceShare precedes Reservation in the Filter order: it has to pass on the unmoved device state too
      if constexpr (DEV > 0) first = first && xfit_ok() && dev_ok();
      if (first)
        r.status = KOORDHIP_PREEMPT_UNRESOLVABLE;
      else
        r.status = any_potential<OVL>(list, len, ov, pprio, pquota) ? KOORDHIP_PREEMPT_UNFIT : KOORDHIP_PREEMPT_NO_VICTIMS;
      return r;
    }
  }
  // list[k] leaves (-1) or rejoins (+1)
  auto move = [&](QuotaUsed &qu, const DevAsg &a, int32_t k, int sign) {
    move_pod(w, qu, a, sign);
    if constexpr (BOTH) {
      // The maps are whole ResourceLists: the pod's scalars move with its five resources
      int64_t axr[KOORDHIP_NXRES];
#pragma unroll
      for (int j = 0; j < KOORDHIP_NXRES; j++)
        axr[j] = (a.flags & ASG_HAS_EXT) && ((ds.xlist[k].xmask >> j) & 1u) ? ds.xlist[k].xreq[j] : 0;
      resv_pre_move(rp, a.pod, axr, asg_slot(a), sign);
    } else if constexpr (RS > 0) {
      resv_pre_move(rp, a.pod, asg_slot(a), sign);
    }
    if constexpr (DEV > 0) {
      if ((a.flags & ASG_HAS_EXT) && (xm | tm)) {
        const DevAsgX &ax = ds.xlist[k];
#pragma unroll
        for (int j = 0; j < KOORDHIP_NXRES; j++)
          if ((xm >> j) & 1u) xfree[j] -= sign * ax.xreq[j];
        if constexpr (DEV == 2) {
          // (BOTH: a bound pod's devices go to DeviceShare's preemptibleInRRs, which nothing reads without a
          // device-holding reservation: Pd moves for a pod that is not bound only; xfree above moves for both)
          const bool bound = BOTH && asg_slot(a) >= 0;
#pragma unroll
          for (int t = 0; t < DT; t++) {
            const uint32_t sl = ((tm >> t) & 1u) && !bound ? ax.dev_slots[t] : 0u;
            if (!sl) continue;
#pragma unroll
            for (int s = 0; s < DS; s++)
              if ((sl >> s) & 1u)
#pragma unroll
                for (int rr = 0; rr < DR; rr++) dev_u(ds, t, s, rr) += sign * ax.dev_per[t][rr];
          }
        }
      }
    }
  };
  QuotaUsed q;
  int32_t pa[KOORDHIP_PREEMPT_PDBS];
#pragma unroll
  for (int k = 0; k < KOORDHIP_PREEMPT_QRES; k++) q.u[k] = P.used[k];
#pragma unroll
  for (int b = 0; b < KOORDHIP_PREEMPT_PDBS; b++) pa[b] = pdb.a[b];
  // remove every pod canPreempt accepts; the PDB split walks the same pods in the same order
  uint64_t pot0 = 0, pot1 = 0, vio0 = 0, vio1 = 0;
  for (int32_t k = 0; k < len; k++) {
    if constexpr (OVL) {
      if (((k < 64 ? ov.g0 : ov.g1) >> (k & 63)) & 1ull) continue;
    }
    const DevAsg &a = list[k];
    if ((a.flags & KOORDHIP_ASG_NONPREEMPTIBLE) || a.prio >= pprio || a.quota != pquota) continue;
    move(q, a, k, -1);
    const uint32_t pm = a.pdb_mask;
    bool bad = false;
#pragma unroll
    for (int b = 0; b < KOORDHIP_PREEMPT_PDBS; b++)
      if ((pm >> b) & 1u) {
        pa[b]--;
        bad = bad || pa[b] < 0;
      }
    const uint64_t bit = 1ull << (k & 63);
    if (k < 64) {
      pot0 |= bit;
      if (bad) vio0 |= bit;
    } else {
      pot1 |= bit;
      if (bad) vio1 |= bit;
    }
  }
  if (!(pot0 | pot1)) {
    r.status = KOORDHIP_PREEMPT_NO_VICTIMS;
    return r;
  }
  if (base_status(w) != 0u || !xfit_ok() || !amp_ok(w) || !resv_ok(w) || !dev_ok() || !second_ok()) {
    r.status = KOORDHIP_PREEMPT_UNFIT;
    return r;
  }
  // reprieve: the violating group first, then the rest, each in list order
  int32_t nv = 0, npdb = 0, top = 0, maxp = 0;
  int64_t sum = 0, es = 0;
  for (int g = 0; g < 4; g++) {
    const bool violating = g < 2;
    uint64_t m = (g & 1) ? pot1 : pot0;
    const uint64_t vm = (g & 1) ? vio1 : vio0;
    m &= violating ? vm : ~vm;
    while (m) {
      const int32_t k = (int32_t)__ffsll((unsigned long long)m) - 1 + ((g & 1) ? 64 : 0);
      m &= m - 1;
      const DevAsg &a = list[k];
      move(q, a, k, +1);
      const bool fits = base_status(w) == 0u && xfit_ok() && amp_ok(w) && resv_ok(w) && dev_ok() && second_ok();
      if (!fits) move(q, a, k, -1);
      bool over = false;
      if (pquota >= 0) {
#pragma unroll
        for (int d = 0; d < KOORDHIP_PREEMPT_QRES; d++)
          if ((P.qmask >> d) & 1u) over = over || q.u[d] + P.req[d] > P.runtime[d];
      }
      if (!fits && over) {  // the second RemovePod of one pod fails: the evaluator drops the node
        koordhip_preempt_node e{};
        e.status = KOORDHIP_PREEMPT_ERROR;
        return e;
      }
      if (fits && !over) continue;  // reprieved
      if (over) move(q, a, k, -1);
      if (!fits && violating) npdb++;
      const int32_t ap = a.prio;
      const int64_t as = a.start;
      if (nv == 0) top = ap;
      if (nv == 0 || ap > maxp) {
        maxp = ap;
        es = as;
      } else if (ap == maxp && as < es) {
        es = as;
      }
      sum += (int64_t)ap + (1ll << 31);
      if constexpr (EMIT == EMIT_IDX) {
        if (nv < vmax) vout[nv] = a.idx;
      }
      if constexpr (EMIT == EMIT_POS) {
        if (nv < vmax) vout[nv] = k;
      }
      nv++;
    }
  }
  r.status = KOORDHIP_PREEMPT_CANDIDATE;
  r.n_victims = nv;
  r.n_pdb_violations = npdb;
  r.top_priority = top;
  r.sum_priority = sum;
  r.earliest_start = es;
  return r;
}

// The dry run's envelope as the compiler sees it: only NodeResourcesFit,
// LoadAware and the static filters can be in the Filter (launch_preempt refuses
// the rest) and no Score is read, so with these masks the NodeNUMAResource and
// Reservation halves of filter_status and their row fields fold away.  NUMA:
// the same masks (the NodeNUMAResource Filter arrives as preempt_node's fcode),
// with amp kept for filterAmplifiedCPUs.  RS > 0: the Reservation Filter bit
// and resv stay (the restore and the walk's own filterWithReservations).
// DEV > 0: and the DeviceShare Filter bit (the walk's own xfit / dev_filter_pre read it).
template <bool NUMA, int RS = 0, int DEV = 0>
__device__ __forceinline__ DevCfg envelope(DevCfg c) {
  c.filt &= KOORDHIP_PLUGIN_FIT | KOORDHIP_PLUGIN_LOADAWARE | KOORDHIP_PLUGIN_NODE_STATIC |
            (RS > 0 ? KOORDHIP_PLUGIN_RESERVATION : 0u) | (DEV > 0 ? KOORDHIP_PLUGIN_DEVICESHARE : 0u);
  c.score = 0;
  if constexpr (RS == 0) c.resv = 0;
  c.zones = 0;
  if constexpr (!NUMA) c.amp = 0;
  return c;
}

// The walk's NUMA row.  Without NUMA: what load_numa leaves under the envelope
// (nothing is read).  With it: the three fields filterAmplifiedCPUs reads.
// RS > 0: and the node's reservation slots.
template <bool NUMA, int RS = 0>
__device__ __forceinline__ void load_walk_numa(WalkRow<RS> &nr, const DevCfg &c, const DevNodes &d, int32_t i,
                                               const Need &all) {
  load_numa<true>(nr, d, i, all);
  if constexpr (NUMA) {
    if (c.amp) {
      nr.cls = d.nu.node_cls[i];
      nr.amp = d.nu.amp[i];
      nr.cnt = d.nu.cnt[i];
    }
  }
  if constexpr (RS > 0) {
    if (c.resv) load_resv(nr, d.rv, i);
  }
}

// The frozen verdicts of one call: plane[p][2][nw] u64, bit b of word w is node
// 64 w + b; [p][0]: the NodeNUMAResource Filter fails, [p][1]: with an
// UnschedulableAndUnresolvable reason.
struct NumaPlane {
  const uint64_t *w;  // preemptor 0's words
  int32_t nw;         // words per row: ceil(n / 64)
};

// node i's code for preemptor p (the wave reads one word per row)
__device__ __forceinline__ uint32_t plane_code(const NumaPlane &pl, int32_t p, int32_t i) {
  const int32_t word = i >> 6;
  if (word >= pl.nw) return 0u;
  const uint64_t *row = pl.w + (size_t)p * 2 * pl.nw + word;
  const uint32_t b = (uint32_t)i & 63u;
  return (uint32_t)((row[0] >> b) & 1ull) * NUMA_F_FAIL | (uint32_t)((row[pl.nw] >> b) & 1ull) * NUMA_F_UNRESOLVABLE;
}

// One node as preempt_node reads it: the row, the walk's NUMA row and the node's listed pods.
template <int RS>
struct WalkNode {
  NV v{};
  WalkRow<RS> nr{};
  const DevAsg *list;
  int32_t len;
  const DevAsgX *xlist;  // the list's records of the second table (the DEVICE mode; NULL: none)
};

// Node i under the envelope c.  live = false: a tail lane, which reads the last row and walks an empty list.
template <bool NUMA, int RS>
__device__ __forceinline__ WalkNode<RS> load_walk_node(const DevCfg &c, const DevNodes &d,
                                                       const DevAsg *__restrict__ tab, const int32_t *__restrict__ off,
                                                       int32_t i, bool live = true, const DevAsgX *xtab = nullptr) {
  const int32_t il = live ? i : d.n - 1;
  WalkNode<RS> x;
  const Need all = need_all(c);
  load_node(x.v, d, il, all, c);
  load_walk_numa<NUMA, RS>(x.nr, c, d, il, all);
  const int32_t lo = off[il];
  x.len = live ? min(off[il + 1] - lo, (int32_t)KOORDHIP_PREEMPT_NODE_PODS) : 0;
  x.list = tab + lo;
  x.xlist = xtab ? xtab + lo : nullptr;
  return x;
}

// The preemptors pre[p0, p0 + np) of a workgroup's tile into LDS, 8-B words over all threads; the caller's
// __syncthreads() publishes them.
__device__ __forceinline__ const DevPre *stage_pre(const DevPre *__restrict__ pre, int32_t p0, int32_t np) {
  __shared__ __attribute__((aligned(16))) uint64_t spw[PRE_PT * PRE_WORDS];
  const uint64_t *src = reinterpret_cast<const uint64_t *>(pre + p0);
  for (int32_t w = threadIdx.x; w < np * PRE_WORDS; w += PREEMPT_THREADS) spw[w] = src[w];
  return reinterpret_cast<const DevPre *>(spw);
}

// The DEV = 2 walk's device state of a workgroup of THREADS threads: DT x DS x DR int64 per thread do not fit the
// register file beside the row, so they live in LDS, [t][s][r][thread]: a thread's words are its own (no
// barrier), a wave's 64 consecutive words of one (t, s, r) go to distinct banks.  At 256 threads that is 144 KB:
// one workgroup per CU, one wave per SIMD, which is what the walk's 200+ registers allow anyway.
template <int DEV, int THREADS>
__device__ __forceinline__ int64_t *dev_state() {
  if constexpr (DEV == 2) {
    __shared__ __attribute__((aligned(16))) int64_t su[DT * DS * DR * THREADS];
    return su + threadIdx.x;
  } else {
    return nullptr;
  }
}

template <int THREADS>
__device__ __forceinline__ DevSide dev_side(const DevNodes &d, const DevAsgX *xlist, const DevPodX *x, int64_t *u,
                                            int32_t i) {
  DevSide ds;
  ds.dv = &d.dv;
  ds.xlist = xlist;
  ds.x = x;
  ds.u = u;
  ds.stride = THREADS;
  ds.i = i;
  ds.n = d.n;
  ds.px = nullptr;
  return ds;
}

// ---------------------------------------------------------------------------
// k_preempt_numa

// One thread per node, 32 preemptors per workgroup: numa_reason without the
// amplification exit on the loaded NUMA row.  A preemptor the plugin does not
// act on (no cpuset, no topology-policy node in the snapshot) gets zero words.
__global__ __launch_bounds__(PREEMPT_THREADS) void k_preempt_numa(DevCfg cfg, DevNodes d,
                                                                  const DevPre *__restrict__ pre, int32_t n_pre,
                                                                  uint64_t *__restrict__ plane, int32_t nw) {
  DevCfg c = cfg;
  c.amp = 0;  // filterAmplifiedCPUs reads the row: it is the walk's
  const int t = threadIdx.x, lane = __lane_id();
  const int32_t p0 = (int32_t)blockIdx.y * PRE_PT;
  const int32_t np = min(PRE_PT, n_pre - p0);
  const DevPre *sp = stage_pre(pre, p0, np);
  __syncthreads();
  const int32_t i = (int32_t)blockIdx.x * PREEMPT_THREADS + t;
  const bool live = i < d.n;
  const int32_t il = live ? i : d.n - 1;  // tail lanes read the last row and set no bit
  const int32_t word = i >> 6;            // 256-node blocks are 64-aligned: a ballot is a plane word
  Need all{};
  all.numa = all.numa_masks = true;
  all.zones = c.zones != 0;
  NumaRow nr{};
  load_numa<true>(nr, d, il, all);
  const NV v{};  // read by the amplification exit only
  for (int32_t q = 0; q < np; q++) {
    const DevPod &pod = sp[q].pod;
    uint64_t fail = 0, unres = 0;
    if (numa_active(pod, c)) {  // wave-uniform
      const uint32_t m = live ? numa_reason(c, pod, v, nr, d.nu.cls) : 0u;
      fail = __ballot(m != 0u);
      unres = __ballot((m & KOORDHIP_REASON_UNRESOLVABLE_MASK) != 0u);
    }
    if (lane == 0 && word < nw) {
      uint64_t *row = plane + (size_t)(p0 + q) * 2 * nw + word;
      row[0] = fail;
      row[nw] = unres;
    }
  }
}

// ---------------------------------------------------------------------------
// k_preempt

// the wave's best candidate (r of node bn, -1: none) into every lane
__device__ __forceinline__ void wave_best(koordhip_preempt_node &r, int32_t &bn) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    koordhip_preempt_node x;
    x.status = KOORDHIP_PREEMPT_CANDIDATE;
    x.n_victims = __shfl_xor(r.n_victims, o, 64);
    x.n_pdb_violations = __shfl_xor(r.n_pdb_violations, o, 64);
    x.top_priority = __shfl_xor(r.top_priority, o, 64);
    x.sum_priority = __shfl_xor((long long)r.sum_priority, o, 64);
    x.earliest_start = __shfl_xor((long long)r.earliest_start, o, 64);
    const int32_t xn = __shfl_xor(bn, o, 64);
    if (pick_before(x, xn, r, bn)) {
      r = x;
      bn = xn;
    }
  }
}

// One preemptor's vote of a wave: node i's verdict r (live = false: a tail lane, counted nowhere) into the
// workgroup's status counters cnt [5] (LDS), the wave's best candidate into *best.
__device__ __forceinline__ void wave_vote(koordhip_preempt_node r, int32_t i, bool live, int32_t *cnt,
                                          PreemptPartial *best) {
  const int lane = __lane_id();
  const int32_t st = live ? r.status : -1;
#pragma unroll
  for (int s = 0; s < KOORDHIP_PREEMPT_STATUSES; s++) {
    const uint64_t mk = __ballot(st == s);
    if (lane == 0 && mk) atomicAdd(&cnt[s], (int32_t)__popcll(mk));
  }
  int32_t bn = st == KOORDHIP_PREEMPT_CANDIDATE ? i : -1;
  wave_best(r, bn);
  if (lane == 0) {
    PreemptPartial b{};
    if (bn >= 0) b.v = r;
    b.node = bn;
    *best = b;
  }
}

// the workgroup's best candidate of one preemptor: the best of its waves' sb [PRE_WAVES]
__device__ __forceinline__ PreemptPartial block_best(const PreemptPartial *sb) {
  PreemptPartial b = sb[0];
#pragma unroll
  for (int w = 1; w < PRE_WAVES; w++) {
    const PreemptPartial x = sb[w];
    if (pick_before(x.v, x.node, b.v, b.node)) b = x;
  }
  return b;
}

// the answer of one preemptor: its pick (node -1: none) and its nodes per status
__device__ __forceinline__ koordhip_preempt_result pick_result(const koordhip_preempt_node &best, int32_t node,
                                                               const int32_t *cnt) {
  koordhip_preempt_result r{};
  r.node = node;
  for (int s = 0; s < KOORDHIP_PREEMPT_STATUSES; s++) r.count[s] = cnt[s];
  if (node >= 0) {
    r.best = best;
    r.best.status = KOORDHIP_PREEMPT_CANDIDATE;
  }
  return r;
}

// BLK: the workgroup's counts go to bcnt [n_pre][gridDim.x][5] instead of
// being summed into count (the sequential dry run replaces single blocks).
// NUMA: pl holds the frozen verdicts of pre[0, n_pre).  RS, DEV: preempt_node's (dw: the DEVICE mode's inputs).
template <bool BLK, bool NUMA, int RS = 0, int DEV = 0>
__device__ __forceinline__ void preempt_tiles(const DevCfg &cfg, const DevNodes &d, const DevAsg *__restrict__ tab,
                                              const int32_t *__restrict__ off, const PdbAllowed &pdb,
                                              const DevPre *__restrict__ pre, int32_t n_pre,
                                              int32_t *__restrict__ count, PreemptPartial *__restrict__ part,
                                              koordhip_preempt_node *__restrict__ per_node,
                                              int32_t *__restrict__ bcnt, const NumaPlane &pl,
                                              const DevWalk &dw = DevWalk{}) {
  const DevCfg c = envelope<NUMA, RS, DEV>(cfg);
  int64_t *su = dev_state<DEV, PREEMPT_THREADS>();
  __shared__ int32_t scnt[PRE_PT * KOORDHIP_PREEMPT_STATUSES];
  __shared__ PreemptPartial sbest[PRE_PT][PRE_WAVES];
  const int t = threadIdx.x, wave = t >> 6;
  const int32_t p0 = (int32_t)blockIdx.y * PRE_PT;
  const int32_t np = min(PRE_PT, n_pre - p0);
  const DevPre *sp = stage_pre(pre, p0, np);
  for (int32_t w = t; w < np * KOORDHIP_PREEMPT_STATUSES; w += PREEMPT_THREADS) scnt[w] = 0;
  __syncthreads();
  const int32_t i = (int32_t)blockIdx.x * PREEMPT_THREADS + t;
  const bool live = i < d.n;
  const WalkNode<RS> nd = load_walk_node<NUMA, RS>(c, d, tab, off, i, live, DEV > 0 ? dw.xtab : nullptr);
  for (int32_t q = 0; q < np; q++) {
    koordhip_preempt_node r{};
    uint32_t fcode = 0u;
    if constexpr (NUMA) fcode = plane_code(pl, p0 + q, i);
    if (live) {
      if constexpr (DEV > 0)
        r = preempt_node<EMIT_NONE, false, NUMA, RS, DEV>(
            c, d.nu.cls, nd.v, nd.nr, nd.list, nd.len, pdb, sp[q], nullptr, 0, NodeOverlay{}, fcode,
            dev_side<PREEMPT_THREADS>(d, nd.xlist, static_cast<const DevPodX *>(dw.px) + p0 + q, su, i));
      else
        r = preempt_node<EMIT_NONE, false, NUMA, RS>(c, d.nu.cls, nd.v, nd.nr, nd.list, nd.len, pdb, sp[q], nullptr, 0,
                                                      NodeOverlay{}, fcode);
    }
    if (per_node && live) per_node[(size_t)q * d.n + i] = r;
    wave_vote(r, i, live, &scnt[q * KOORDHIP_PREEMPT_STATUSES], &sbest[q][wave]);
  }
  __syncthreads();
  if (t < np) part[(size_t)(p0 + t) * gridDim.x + blockIdx.x] = block_best(sbest[t]);
  for (int32_t w = t; w < np * KOORDHIP_PREEMPT_STATUSES; w += PREEMPT_THREADS) {
    const int32_t x = scnt[w];
    if constexpr (BLK) {
      const int32_t q = w / KOORDHIP_PREEMPT_STATUSES, s = w - q * KOORDHIP_PREEMPT_STATUSES;
      bcnt[((size_t)(p0 + q) * gridDim.x + blockIdx.x) * KOORDHIP_PREEMPT_STATUSES + s] = x;
    } else {
      if (x) atomicAdd(&count[(size_t)p0 * KOORDHIP_PREEMPT_STATUSES + w], x);
    }
  }
}

// pl: k_preempt_numa's plane for pre[0, n_pre) (NUMA), else empty
template <bool NUMA, int RS>
__global__ __launch_bounds__(PREEMPT_THREADS) void k_preempt(DevCfg cfg, DevNodes d, const DevAsg *__restrict__ tab,
                                                             const int32_t *__restrict__ off, PdbAllowed pdb,
                                                             const DevPre *__restrict__ pre, int32_t n_pre,
                                                             int32_t *__restrict__ count,
                                                             PreemptPartial *__restrict__ part,
                                                             koordhip_preempt_node *__restrict__ per_node,
                                                             NumaPlane pl) {
  preempt_tiles<false, NUMA, RS>(cfg, d, tab, off, pdb, pre, n_pre, count, part, per_node, nullptr, pl);
}

// ... in the DEVICE mode (DEV = 1: no device preemptor in the call, 2: some)
template <bool NUMA, int DEV>
__global__ __launch_bounds__(PREEMPT_THREADS) void k_preempt_dev(DevCfg cfg, DevNodes d,
                                                                 const DevAsg *__restrict__ tab,
                                                                 const int32_t *__restrict__ off, PdbAllowed pdb,
                                                                 const DevPre *__restrict__ pre, int32_t n_pre,
                                                                 int32_t *__restrict__ count,
                                                                 PreemptPartial *__restrict__ part,
                                                                 koordhip_preempt_node *__restrict__ per_node,
                                                                 NumaPlane pl, DevWalk dw) {
  preempt_tiles<false, NUMA, 0, DEV>(cfg, d, tab, off, pdb, pre, n_pre, count, part, per_node, nullptr, pl, dw);
}

// ... under DeviceShare beside Reservation state (KOORDHIP_PREEMPT_DEVICE_RESV): the walk with the node's RS
// reservation slots, the plugin's maps with their scalars and the DEVICE mode's state, over the same tiles
template <bool NUMA, int RS, int DEV>
__global__ __launch_bounds__(PREEMPT_THREADS) void k_preempt_dev_resv(DevCfg cfg, DevNodes d,
                                                                      const DevAsg *__restrict__ tab,
                                                                      const int32_t *__restrict__ off, PdbAllowed pdb,
                                                                      const DevPre *__restrict__ pre, int32_t n_pre,
                                                                      int32_t *__restrict__ count,
                                                                      PreemptPartial *__restrict__ part,
                                                                      koordhip_preempt_node *__restrict__ per_node,
                                                                      NumaPlane pl, DevWalk dw) {
  static_assert(RS > 0 && DEV > 0, "both states");
  preempt_tiles<false, NUMA, RS, DEV>(cfg, d, tab, off, pdb, pre, n_pre, count, part, per_node, nullptr, pl, dw);
}

// Phase 1 of the sequential dry run: one tile of preemptors on the loaded
// state (pl: the tile's first preemptor's words).  Once the budgets have
// changed (or with the A/B knob) every block evaluates every later preemptor
// again and nothing reads this tile: skip it.
template <bool NUMA>
__global__ __launch_bounds__(PREEMPT_THREADS) void k_preempt_blk(DevCfg cfg, DevNodes d, const DevAsg *__restrict__ tab,
                                                                 const int32_t *__restrict__ off, PdbAllowed pdb,
                                                                 const DevPre *__restrict__ pre, int32_t n_pre,
                                                                 PreemptPartial *__restrict__ part,
                                                                 int32_t *__restrict__ bcnt,
                                                                 const StreamFlags *__restrict__ flags, NumaPlane pl) {
  if (flags->pdb | flags->full) return;
  preempt_tiles<true, NUMA>(cfg, d, tab, off, pdb, pre, n_pre, nullptr, part, nullptr, bcnt, pl);
}

// one wave per preemptor over its nb partials
__global__ __launch_bounds__(64) void k_preempt_pick(const PreemptPartial *__restrict__ part, int32_t nb,
                                                     const int32_t *__restrict__ count,
                                                     koordhip_preempt_result *__restrict__ res) {
  const int32_t p = (int32_t)blockIdx.x;
  const int lane = threadIdx.x;
  PreemptPartial b{};
  b.node = -1;
  for (int32_t k = lane; k < nb; k += 64) {
    const PreemptPartial x = part[(size_t)p * nb + k];
    if (pick_before(x.v, x.node, b.v, b.node)) b = x;
  }
  wave_best(b.v, b.node);
  if (lane == 0) res[p] = pick_result(b.v, b.node, count + (size_t)p * KOORDHIP_PREEMPT_STATUSES);
}

// one thread per preemptor: its chosen node again, writing the victims (vout is -1 filled by the caller).
// NUMA: a chosen node is a CANDIDATE, so its frozen verdict is "passes" and only filterAmplifiedCPUs is left.
template <bool NUMA, int RS>
__global__ __launch_bounds__(64) void k_preempt_victims(DevCfg cfg, DevNodes d, const DevAsg *__restrict__ tab,
                                                        const int32_t *__restrict__ off, PdbAllowed pdb,
                                                        const DevPre *__restrict__ pre, int32_t n_pre,
                                                        const koordhip_preempt_result *__restrict__ res,
                                                        int32_t *__restrict__ vout, int32_t vmax) {
  const DevCfg c = envelope<NUMA, RS>(cfg);
  const int32_t p = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (p >= n_pre) return;
  const int32_t i = res[p].node;
  if (i < 0 || i >= d.n) return;
  const WalkNode<RS> nd = load_walk_node<NUMA, RS>(c, d, tab, off, i);
  const DevPre P = pre[p];
  (void)preempt_node<EMIT_IDX, false, NUMA, RS>(c, d.nu.cls, nd.v, nd.nr, nd.list, nd.len, pdb, P,
                                                vout + (size_t)p * vmax, vmax, NodeOverlay{}, 0u);
}

// ... in the DEVICE mode: the chosen node again with the same function
template <bool NUMA, int DEV>
__global__ __launch_bounds__(64) void k_preempt_victims_dev(DevCfg cfg, DevNodes d, const DevAsg *__restrict__ tab,
                                                            const int32_t *__restrict__ off, PdbAllowed pdb,
                                                            const DevPre *__restrict__ pre, int32_t n_pre,
                                                            const koordhip_preempt_result *__restrict__ res,
                                                            int32_t *__restrict__ vout, int32_t vmax, DevWalk dw) {
  const DevCfg c = envelope<NUMA, 0, DEV>(cfg);
  int64_t *su = dev_state<DEV, 64>();
  const int32_t p = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (p >= n_pre) return;
  const int32_t i = res[p].node;
  if (i < 0 || i >= d.n) return;
  const WalkNode<0> nd = load_walk_node<NUMA, 0>(c, d, tab, off, i, true, dw.xtab);
  const DevPre P = pre[p];
  (void)preempt_node<EMIT_IDX, false, NUMA, 0, DEV>(
      c, d.nu.cls, nd.v, nd.nr, nd.list, nd.len, pdb, P, vout + (size_t)p * vmax, vmax, NodeOverlay{}, 0u,
      dev_side<64>(d, nd.xlist, static_cast<const DevPodX *>(dw.px) + p, su, i));
}

// ... under DeviceShare beside Reservation state
template <bool NUMA, int RS, int DEV>
__global__ __launch_bounds__(64) void k_preempt_victims_dev_resv(DevCfg cfg, DevNodes d, const DevAsg *__restrict__ tab,
                                                                 const int32_t *__restrict__ off, PdbAllowed pdb,
                                                                 const DevPre *__restrict__ pre, int32_t n_pre,
                                                                 const koordhip_preempt_result *__restrict__ res,
                                                                 int32_t *__restrict__ vout, int32_t vmax, DevWalk dw) {
  static_assert(RS > 0 && DEV > 0, "both states");
  const DevCfg c = envelope<NUMA, RS, DEV>(cfg);
  int64_t *su = dev_state<DEV, 64>();
  const int32_t p = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (p >= n_pre) return;
  const int32_t i = res[p].node;
  if (i < 0 || i >= d.n) return;
  const WalkNode<RS> nd = load_walk_node<NUMA, RS>(c, d, tab, off, i, true, dw.xtab);
  const DevPre P = pre[p];
  (void)preempt_node<EMIT_IDX, false, NUMA, RS, DEV>(
      c, d.nu.cls, nd.v, nd.nr, nd.list, nd.len, pdb, P, vout + (size_t)p * vmax, vmax, NodeOverlay{}, 0u,
      dev_side<64>(d, nd.xlist, static_cast<const DevPodX *>(dw.px) + p, su, i));
}

// ---------------------------------------------------------------------------
// the sequential dry run: preemptor k on the state its predecessors left

__global__ void k_stream_init(PdbAllowed pdb, StreamFlags fl, StreamState st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    *st.pdb = pdb;
    *st.flags = fl;
  }
}

__device__ __forceinline__ NodeOverlay overlay_of(const StreamState &st, int32_t i) {
  NodeOverlay ov;
  ov.g0 = st.gone[2 * (size_t)i];
  ov.g1 = st.gone[2 * (size_t)i + 1];
  ov.nom = st.nom;
  ov.head = st.head[i];
  return ov;
}

// preemptor k as it stands now: its quota's used without what its predecessors freed
__device__ __forceinline__ DevPre stream_pre(const DevPre *__restrict__ pre, const StreamState &st, int32_t k) {
  DevPre P = pre[k];
#pragma unroll
  for (int r = 0; r < KOORDHIP_PREEMPT_QRES; r++) {
    const int64_t f = st.freed[(size_t)k * KOORDHIP_PREEMPT_QRES + r];
    P.used[r] = P.used[r] > f ? P.used[r] - f : 0;
  }
  return P;
}

// Block b evaluates preemptor k again iff its rows / lists changed, the
// budgets changed or k's quota was freed; a block none of this holds for keeps
// the partial and the counts phase 1 wrote (they depend on nothing else).
// pl: the plane of all the call's preemptors.  RS > 0 (koordhip_preempt_stream_resv): the walk with the node's
// reservation slots, run as the per-preemptor chain (StreamFlags::full is set: every block, every preemptor).
template <bool NUMA, int RS>
__global__ __launch_bounds__(PREEMPT_THREADS) void k_preempt_seq(DevCfg cfg, DevNodes d, const DevAsg *__restrict__ tab,
                                                                 const int32_t *__restrict__ off,
                                                                 const DevPre *__restrict__ pre, int32_t k,
                                                                 StreamState st, NumaPlane pl) {
  const int t = threadIdx.x, wave = t >> 6;
  const int32_t b = (int32_t)blockIdx.x, nb = (int32_t)gridDim.x;
  const StreamFlags fl = *st.flags;
  if (!(fl.full | fl.pdb | st.qflag[k] | st.touched[b])) {
    if (t == 0) atomicAdd(reinterpret_cast<unsigned long long *>(&st.stats->blocks_skipped), 1ull);
    return;
  }
  if (t == 0) atomicAdd(reinterpret_cast<unsigned long long *>(&st.stats->block_recomputes), 1ull);
  const DevCfg c = envelope<NUMA, RS>(cfg);
  __shared__ int32_t scnt[KOORDHIP_PREEMPT_STATUSES];
  __shared__ PreemptPartial sbest[PRE_WAVES];
  if (t < KOORDHIP_PREEMPT_STATUSES) scnt[t] = 0;
  __syncthreads();
  const DevPre P = stream_pre(pre, st, k);
  const PdbAllowed pdb = *st.pdb;
  const int32_t i = b * PREEMPT_THREADS + t;
  const bool live = i < d.n;
  const WalkNode<RS> nd = load_walk_node<NUMA, RS>(c, d, tab, off, i, live);
  koordhip_preempt_node r{};
  uint32_t fcode = 0u;
  if constexpr (NUMA) fcode = plane_code(pl, k, i);
  if (live)
    r = preempt_node<EMIT_NONE, true, NUMA, RS>(c, d.nu.cls, nd.v, nd.nr, nd.list, nd.len, pdb, P, nullptr, 0,
                                                overlay_of(st, i), fcode);
  wave_vote(r, i, live, scnt, &sbest[wave]);
  __syncthreads();
  if (t == 0) st.part[(size_t)k * nb + b] = block_best(sbest);
  if (t < KOORDHIP_PREEMPT_STATUSES) st.bcnt[((size_t)k * nb + b) * KOORDHIP_PREEMPT_STATUSES + t] = scnt[t];
}

// one wave: preemptor k's nb partials and counts -> res[k]
__global__ __launch_bounds__(64) void k_preempt_seq_pick(int32_t nb, int32_t k, StreamState st) {
  const int lane = threadIdx.x;
  PreemptPartial b{};
  b.node = -1;
  int32_t cnt[KOORDHIP_PREEMPT_STATUSES] = {};
  for (int32_t j = lane; j < nb; j += 64) {
    const PreemptPartial x = st.part[(size_t)k * nb + j];
    if (pick_before(x.v, x.node, b.v, b.node)) b = x;
#pragma unroll
    for (int s = 0; s < KOORDHIP_PREEMPT_STATUSES; s++)
      cnt[s] += st.bcnt[((size_t)k * nb + j) * KOORDHIP_PREEMPT_STATUSES + s];
  }
  koordhip_preempt_node r = b.v;
  int32_t bn = b.node;
  wave_best(r, bn);
#pragma unroll
  for (int s = 0; s < KOORDHIP_PREEMPT_STATUSES; s++)
    for (int o = 32; o >= 1; o >>= 1) cnt[s] += __shfl_xor(cnt[s], o, 64);
  if (lane == 0) {
    st.res[k] = pick_result(r, bn, cnt);
    if (st.flags->pdb | st.qflag[k]) st.stats->full_recomputes += 1;
  }
}

// One wave: the chosen node of preemptor k again, its victims written out and
// taken off the state every later preemptor sees.  RS > 0: what the victims held of their reservations needs no
// state of its own, every later walk lowers its slots by the gone positions' records.
template <bool NUMA, int RS>
__global__ __launch_bounds__(64) void k_preempt_apply(DevCfg cfg, DevNodes d, const DevAsg *__restrict__ tab,
                                                      const int32_t *__restrict__ off, const DevPre *__restrict__ pre,
                                                      int32_t n_pre, int32_t k, StreamState st, int32_t vmax) {
  const DevCfg c = envelope<NUMA, RS>(cfg);
  const int lane = threadIdx.x;
  const int32_t i = st.res[k].node;
  if (i < 0 || i >= d.n) return;
  const WalkNode<RS> nd = load_walk_node<NUMA, RS>(c, d, tab, off, i);  // i is the wave's: scalar loads
  // the node's list into LDS with the whole wave: lane 0's walk is a chain of dependent loads
  __shared__ uint4 slist[KOORDHIP_PREEMPT_NODE_PODS * ASG_VEC];
  const uint4 *src = reinterpret_cast<const uint4 *>(nd.list);
  for (int32_t w = lane; w < nd.len * ASG_VEC; w += 64) slist[w] = src[w];
  __syncthreads();
  const DevAsg *list = reinterpret_cast<const DevAsg *>(slist);
  const DevPre P = stream_pre(pre, st, k);
  __shared__ int32_t sfreed;
  __shared__ int64_t ssum[KOORDHIP_PREEMPT_QRES];
  if (lane == 0) {
    PdbAllowed pdb = *st.pdb;
    const koordhip_preempt_node r = preempt_node<EMIT_POS, true, NUMA, RS>(c, d.nu.cls, nd.v, nd.nr, list, nd.len, pdb,
                                                                           P, st.vpos, KOORDHIP_PREEMPT_NODE_PODS,
                                                                           overlay_of(st, i), 0u);
    const int32_t nv = r.status == KOORDHIP_PREEMPT_CANDIDATE ? min(r.n_victims, (int32_t)KOORDHIP_PREEMPT_NODE_PODS) : 0;
    uint64_t g0 = 0, g1 = 0;
    int64_t sum[KOORDHIP_PREEMPT_QRES] = {};
    bool moved = false;
    for (int32_t e = 0; e < nv; e++) {
      const int32_t pos = st.vpos[e];
      const DevAsg &a = list[pos];
      if (st.victims && e < vmax) st.victims[(size_t)k * vmax + e] = a.idx;
      if (pos < 64) g0 |= 1ull << pos; else g1 |= 1ull << (pos - 64);
      const uint32_t pm = a.pdb_mask;
      for (int bb = 0; bb < KOORDHIP_PREEMPT_PDBS; bb++)
        if (((pm >> bb) & 1u) && pdb.a[bb] > 0) {
          pdb.a[bb]--;
          moved = true;
        }
      if (a.flags & KOORDHIP_ASG_IN_QUOTA)
        for (int q = 0; q < KOORDHIP_PREEMPT_QRES; q++) sum[q] += a.qreq[q];
    }
    st.gone[2 * (size_t)i] |= g0;
    st.gone[2 * (size_t)i + 1] |= g1;
    NomEntry ne;
    ne.pod = P.pod;
    ne.prio = P.prio;
    ne.next = st.head[i];
    st.nom[k] = ne;
    st.head[i] = k;
    st.touched[i / PREEMPT_THREADS] = 1;
    if (moved) {
      *st.pdb = pdb;
      st.flags->pdb = 1;
    }
    int64_t any = 0;
    for (int q = 0; q < KOORDHIP_PREEMPT_QRES; q++) {
      ssum[q] = sum[q];
      any |= sum[q];
    }
    sfreed = any != 0;
  }
  __syncthreads();
  // what the victims held in k's quota is free for every later preemptor of that quota
  const int32_t quota = P.quota;
  if (quota < 0 || !sfreed) return;
  for (int32_t j = k + 1 + lane; j < n_pre; j += 64) {
    if (pre[j].quota != quota) continue;
    for (int q = 0; q < KOORDHIP_PREEMPT_QRES; q++) st.freed[(size_t)j * KOORDHIP_PREEMPT_QRES + q] += ssum[q];
    st.qflag[j] = 1;
  }
}

// ... in the DEVICE mode (koordhip_preempt_stream_ext): the per-preemptor chain only, every block evaluates
// preemptor k on the state its predecessors left (there is no phase 1 and nothing is skipped; StreamFlags::full
// is set, touched is written and never read).  DEV = 2 keeps the 256-thread block and dev_state's
// su[t][s][r][thread]: one partial per 256 nodes, so k_preempt_seq_pick and the carve are the plain stream's.
template <bool NUMA, int DEV>
__global__ __launch_bounds__(PREEMPT_THREADS) void k_preempt_seq_dev(DevCfg cfg, DevNodes d,
                                                                     const DevAsg *__restrict__ tab,
                                                                     const int32_t *__restrict__ off,
                                                                     const DevPre *__restrict__ pre, int32_t k,
                                                                     StreamState st, NumaPlane pl, DevWalk dw) {
  const int t = threadIdx.x, wave = t >> 6;
  const int32_t b = (int32_t)blockIdx.x, nb = (int32_t)gridDim.x;
  if (t == 0) atomicAdd(reinterpret_cast<unsigned long long *>(&st.stats->block_recomputes), 1ull);
  const DevCfg c = envelope<NUMA, 0, DEV>(cfg);
  int64_t *su = dev_state<DEV, PREEMPT_THREADS>();
  __shared__ int32_t scnt[KOORDHIP_PREEMPT_STATUSES];
  __shared__ PreemptPartial sbest[PRE_WAVES];
  if (t < KOORDHIP_PREEMPT_STATUSES) scnt[t] = 0;
  __syncthreads();
  const DevPre P = stream_pre(pre, st, k);
  const PdbAllowed pdb = *st.pdb;
  const int32_t i = b * PREEMPT_THREADS + t;
  const bool live = i < d.n;
  const WalkNode<0> nd = load_walk_node<NUMA, 0>(c, d, tab, off, i, live, dw.xtab);
  koordhip_preempt_node r{};
  uint32_t fcode = 0u;
  if constexpr (NUMA) fcode = plane_code(pl, k, i);
  if (live) {
    const DevPodX *px = static_cast<const DevPodX *>(dw.px);
    DevSide ds = dev_side<PREEMPT_THREADS>(d, nd.xlist, px + k, su, i);
    ds.px = px;
    r = preempt_node<EMIT_NONE, true, NUMA, 0, DEV>(c, d.nu.cls, nd.v, nd.nr, nd.list, nd.len, pdb, P, nullptr, 0,
                                                    overlay_of(st, i), fcode, ds);
  }
  wave_vote(r, i, live, scnt, &sbest[wave]);
  __syncthreads();
  if (t == 0) st.part[(size_t)k * nb + b] = block_best(sbest);
  if (t < KOORDHIP_PREEMPT_STATUSES) st.bcnt[((size_t)k * nb + b) * KOORDHIP_PREEMPT_STATUSES + t] = scnt[t];
}

// One wave: k_preempt_apply with the DEVICE mode's walk (DEV = 2: the 64-thread dev_state beside the staged
// list; lane 0 reads the chosen node's second-table records where they lie).  What the victims held of scalars
// and devices needs no state of its own: every later walk reads it off the gone positions' records.
template <bool NUMA, int DEV>
__global__ __launch_bounds__(64) void k_preempt_apply_dev(DevCfg cfg, DevNodes d, const DevAsg *__restrict__ tab,
                                                          const int32_t *__restrict__ off,
                                                          const DevPre *__restrict__ pre, int32_t n_pre, int32_t k,
                                                          StreamState st, int32_t vmax, DevWalk dw) {
  const DevCfg c = envelope<NUMA, 0, DEV>(cfg);
  int64_t *su = dev_state<DEV, 64>();
  const int lane = threadIdx.x;
  const int32_t i = st.res[k].node;
  if (i < 0 || i >= d.n) return;
  const WalkNode<0> nd = load_walk_node<NUMA, 0>(c, d, tab, off, i, true, dw.xtab);
  __shared__ uint4 slist[KOORDHIP_PREEMPT_NODE_PODS * ASG_VEC];
  const uint4 *src = reinterpret_cast<const uint4 *>(nd.list);
  for (int32_t w = lane; w < nd.len * ASG_VEC; w += 64) slist[w] = src[w];
  __syncthreads();
  const DevAsg *list = reinterpret_cast<const DevAsg *>(slist);
  const DevPre P = stream_pre(pre, st, k);
  __shared__ int32_t sfreed;
  __shared__ int64_t ssum[KOORDHIP_PREEMPT_QRES];
  if (lane == 0) {
    PdbAllowed pdb = *st.pdb;
    const DevPodX *px = static_cast<const DevPodX *>(dw.px);
    DevSide ds = dev_side<64>(d, nd.xlist, px + k, su, i);
    ds.px = px;
    // Entry k (preemptor k's: its scalars are px[k]'s) is written before the walk and linked after it: the walk
    // follows head[i], which does not reach it, and P.pod kept over the DEV = 2 walk would be a scratch frame.
    NomEntry ne;
    ne.pod = P.pod;
    ne.prio = P.prio;
    ne.next = st.head[i];
    st.nom[k] = ne;
    const koordhip_preempt_node r = preempt_node<EMIT_POS, true, NUMA, 0, DEV>(
        c, d.nu.cls, nd.v, nd.nr, list, nd.len, pdb, P, st.vpos, KOORDHIP_PREEMPT_NODE_PODS, overlay_of(st, i), 0u, ds);
    const int32_t nv = r.status == KOORDHIP_PREEMPT_CANDIDATE ? min(r.n_victims, (int32_t)KOORDHIP_PREEMPT_NODE_PODS) : 0;
    uint64_t g0 = 0, g1 = 0;
    int64_t sum[KOORDHIP_PREEMPT_QRES] = {};
    bool moved = false;
    for (int32_t e = 0; e < nv; e++) {
      const int32_t pos = st.vpos[e];
      const DevAsg &a = list[pos];
      if (st.victims && e < vmax) st.victims[(size_t)k * vmax + e] = a.idx;
      if (pos < 64) g0 |= 1ull << pos; else g1 |= 1ull << (pos - 64);
      const uint32_t pm = a.pdb_mask;
      for (int bb = 0; bb < KOORDHIP_PREEMPT_PDBS; bb++)
        if (((pm >> bb) & 1u) && pdb.a[bb] > 0) {
          pdb.a[bb]--;
          moved = true;
        }
      if (a.flags & KOORDHIP_ASG_IN_QUOTA)
        for (int q = 0; q < KOORDHIP_PREEMPT_QRES; q++) sum[q] += a.qreq[q];
    }
    st.gone[2 * (size_t)i] |= g0;
    st.gone[2 * (size_t)i + 1] |= g1;
    st.head[i] = k;
    st.touched[i / PREEMPT_THREADS] = 1;
    if (moved) {
      *st.pdb = pdb;
      st.flags->pdb = 1;
    }
    int64_t any = 0;
    for (int q = 0; q < KOORDHIP_PREEMPT_QRES; q++) {
      ssum[q] = sum[q];
      any |= sum[q];
    }
    sfreed = any != 0;
  }
  __syncthreads();
  const int32_t quota = P.quota;
  if (quota < 0 || !sfreed) return;
  for (int32_t j = k + 1 + lane; j < n_pre; j += 64) {
    if (pre[j].quota != quota) continue;
    for (int q = 0; q < KOORDHIP_PREEMPT_QRES; q++) st.freed[(size_t)j * KOORDHIP_PREEMPT_QRES + q] += ssum[q];
    st.qflag[j] = 1;
  }
}

// ---------------------------------------------------------------------------
// host-side launch wrappers

size_t preempt_ws_ints(int32_t n, int32_t m) { return 2 * ((size_t)n + 1) + (size_t)std::max(m, 0) + 1; }

hipError_t launch_preempt_lists(const DevAsg *raw, DevAsg *sorted, int32_t m, int32_t n, int32_t *ws, hipStream_t s,
                                const void *xraw, void *xsorted) {
  int32_t *cnt = ws, *off = preempt_off(ws, n), *nl = off + n + 1, *tot = nl + std::max(m, 0);
  hipError_t e = hipMemsetAsync(cnt, 0, ((size_t)n + 1) * sizeof(int32_t), s);
  if (e != hipSuccess) return e;
  if (m <= 0) return hipMemsetAsync(off, 0, ((size_t)n + 1) * sizeof(int32_t), s);
  const dim3 mg((m + 255) / 256), blk(256);
  hipLaunchKernelGGL(k_pre_count, mg, blk, 0, s, raw, m, n, cnt);
  e = launch_scan(cnt, off, n + 1, tot, s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(cnt, 0, ((size_t)n + 1) * sizeof(int32_t), s);  // now the fill's cursors
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_pre_fill, mg, blk, 0, s, raw, m, n, off, cnt, nl);
  if (n > 0) hipLaunchKernelGGL(k_pre_sort, dim3((n + 255) / 256), blk, 0, s, raw, off, nl, n);
  const int64_t words = (int64_t)m * ASG_VEC;
  hipLaunchKernelGGL(k_pre_permute, dim3((unsigned)((words + 255) / 256)), blk, 0, s, raw, sorted, nl, m);
  if (xraw && xsorted)  // the second table by the same order: its records are DevAsg's size, copied as 16-B words
    hipLaunchKernelGGL(k_pre_permute, dim3((unsigned)((words + 255) / 256)), blk, 0, s,
                       static_cast<const DevAsg *>(xraw), static_cast<DevAsg *>(xsorted), nl, m);
  return hipGetLastError();
}

size_t preempt_plane_words(int32_t n, int32_t n_pre) { return (size_t)std::max(n_pre, 0) * 2 * (((size_t)n + 63) / 64); }

// The launchers' argument check: m is the walk of every state the profile has (the mode with every flag
// accepted: NodeNUMAResource in the Filter needs the plane, Reservation state the walk with its slots).
static bool preempt_profile_ok(const DevCfg &c, WalkMode m, const uint64_t *plane, const DevWalk &dw) {
  const WalkMode all = preempt_walk_mode(c, KOORDHIP_PREEMPT_NUMA_FROZEN | KOORDHIP_PREEMPT_RESV |
                                                KOORDHIP_PREEMPT_DEVICE | KOORDHIP_PREEMPT_DEVICE_RESV);
  if ((m.dev > 0) != (all.dev > 0) || m.dev > 2) return false;
  // DEVICE: P's records, and Reservation state only where the host accepted both (then with the walk's slots)
  if (m.dev > 0 && (!dw.px || (m.both ? m.rs == 0 : (m.rs != 0 || m.resv)))) return false;
  return m.numa == all.numa && m.rs == all.rs && m.numa == (plane != nullptr);
}

// The one place a WalkMode becomes template arguments: f(std::bool_constant<NUMA>, std::integral_constant<int, RS>).
template <class F>
static void with_walk(WalkMode m, F f) {
  auto slots = [&](auto numa) {
    if (m.rs > 1)
      f(numa, std::integral_constant<int, KOORDHIP_RESV_SLOTS>{});
    else if (m.rs == 1)
      f(numa, std::integral_constant<int, 1>{});
    else
      f(numa, std::integral_constant<int, 0>{});
  };
  if (m.numa)
    slots(std::true_type{});
  else
    slots(std::false_type{});
}

// ... of the DEVICE mode: f(std::bool_constant<NUMA>, std::integral_constant<int, DEV>), DEV = m.dev in {1, 2}.
template <class F>
static void with_walk_dev(WalkMode m, F f) {
  auto devs = [&](auto numa) {
    if (m.dev > 1)
      f(numa, std::integral_constant<int, 2>{});
    else
      f(numa, std::integral_constant<int, 1>{});
  };
  if (m.numa)
    devs(std::true_type{});
  else
    devs(std::false_type{});
}

// ... under both states (m.both): f(std::bool_constant<NUMA>, std::integral_constant<int, RS>,
// std::integral_constant<int, DEV>), RS in {1, KOORDHIP_RESV_SLOTS}, DEV in {1, 2}.
template <class F>
static void with_walk_dev_resv(WalkMode m, F f) {
  with_walk_dev(m, [&](auto numa, auto dev) {
    if (m.rs > 1)
      f(numa, std::integral_constant<int, KOORDHIP_RESV_SLOTS>{}, dev);
    else
      f(numa, std::integral_constant<int, 1>{}, dev);
  });
}

hipError_t launch_preempt_numa(const DevCfg &c, const DevNodes &d, const DevPre *pre, int32_t n_pre, uint64_t *plane,
                               hipStream_t s) {
  if (n_pre <= 0 || d.n <= 0) return hipSuccess;
  if (!(c.filt & KOORDHIP_PLUGIN_NUMA) || !plane) return hipErrorInvalidValue;
  const dim3 grid(preempt_blocks(d.n), (n_pre + PRE_PT - 1) / PRE_PT);
  if (grid.y > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_preempt_numa, grid, dim3(PREEMPT_THREADS), 0, s, c, d, pre, n_pre, plane, (d.n + 63) / 64);
  return hipGetLastError();
}

hipError_t launch_preempt(const DevCfg &c, const DevNodes &d, const DevAsg *tab, const int32_t *off,
                          const PdbAllowed &pdb, const DevPre *pre, int32_t n_pre, int32_t *count,
                          PreemptPartial *part, koordhip_preempt_node *per_node, const uint64_t *plane, WalkMode m,
                          hipStream_t s, DevWalk dw) {
  if (n_pre <= 0 || d.n <= 0) return hipSuccess;
  if (!preempt_profile_ok(c, m, plane, dw)) return hipErrorInvalidValue;
  if (per_node && n_pre != 1) return hipErrorInvalidValue;
  const dim3 grid(preempt_blocks(d.n), (n_pre + PRE_PT - 1) / PRE_PT);
  if (grid.y > 65535u) return hipErrorInvalidValue;
  const NumaPlane pl{plane, (d.n + 63) / 64};
  if (m.both) {
    with_walk_dev_resv(m, [&](auto numa, auto rs, auto dev) {
      hipLaunchKernelGGL((k_preempt_dev_resv<decltype(numa)::value, decltype(rs)::value, decltype(dev)::value>), grid,
                         dim3(PREEMPT_THREADS), 0, s, c, d, tab, off, pdb, pre, n_pre, count, part, per_node, pl, dw);
    });
    return hipGetLastError();
  }
  if (m.dev > 0) {
    with_walk_dev(m, [&](auto numa, auto dev) {
      hipLaunchKernelGGL((k_preempt_dev<decltype(numa)::value, decltype(dev)::value>), grid, dim3(PREEMPT_THREADS), 0, s,
                         c, d, tab, off, pdb, pre, n_pre, count, part, per_node, pl, dw);
    });
    return hipGetLastError();
  }
  with_walk(m, [&](auto numa, auto rs) {
    hipLaunchKernelGGL((k_preempt<decltype(numa)::value, decltype(rs)::value>), grid, dim3(PREEMPT_THREADS), 0, s, c, d,
                       tab, off, pdb, pre, n_pre, count, part, per_node, pl);
  });
  return hipGetLastError();
}

hipError_t launch_preempt_stream(const DevCfg &c, const DevNodes &d, const DevAsg *tab, const int32_t *off,
                                 const PdbAllowed &pdb, const DevPre *pre, int32_t n_pre, const StreamState &st,
                                 int32_t max_victims, bool full, const uint64_t *plane, WalkMode m, hipStream_t s) {
  if (n_pre <= 0 || d.n <= 0) return hipSuccess;
  if (m.devp || m.both || !preempt_profile_ok(c, m, plane, DevWalk{})) return hipErrorInvalidValue;
  const int32_t nb = preempt_blocks(d.n);
  const NumaPlane pl{plane, (d.n + 63) / 64};
  StreamFlags fl{};
  fl.full = full || m.rs > 0 ? 1 : 0;  // with Reservation state: the chain, every block, every preemptor
  hipLaunchKernelGGL(k_stream_init, dim3(1), dim3(64), 0, s, pdb, fl, st);
  with_walk(m, [&](auto numa, auto rs) {
    constexpr bool NUMA = decltype(numa)::value;
    constexpr int RS = decltype(rs)::value;
    const dim3 blocks(nb), threads(PREEMPT_THREADS), wave(64);
    for (int32_t k = 0; k < n_pre; k++) {
      // phase 1 a tile ahead of its first preemptor, not all at once: the loaded state does not change, and a tile
      // launched after the budgets changed costs an empty kernel
      if constexpr (RS == 0) {
        if (k % PRE_PT == 0)
          hipLaunchKernelGGL(k_preempt_blk<NUMA>, blocks, threads, 0, s, c, d, tab, off, pdb, pre + k,
                             std::min(PRE_PT, n_pre - k), st.part + (size_t)k * nb,
                             st.bcnt + (size_t)k * nb * KOORDHIP_PREEMPT_STATUSES, st.flags,
                             NUMA ? NumaPlane{plane + (size_t)k * 2 * pl.nw, pl.nw} : pl);
      }
      hipLaunchKernelGGL((k_preempt_seq<NUMA, RS>), blocks, threads, 0, s, c, d, tab, off, pre, k, st, pl);
      hipLaunchKernelGGL(k_preempt_seq_pick, dim3(1), wave, 0, s, nb, k, st);
      hipLaunchKernelGGL((k_preempt_apply<NUMA, RS>), dim3(1), wave, 0, s, c, d, tab, off, pre, n_pre, k, st,
                         max_victims);
    }
  });
  return hipGetLastError();
}

hipError_t launch_preempt_stream_dev(const DevCfg &c, const DevNodes &d, const DevAsg *tab, const int32_t *off,
                                     const PdbAllowed &pdb, const DevPre *pre, int32_t n_pre, const StreamState &st,
                                     int32_t max_victims, const uint64_t *plane, WalkMode m, hipStream_t s, DevWalk dw) {
  if (n_pre <= 0 || d.n <= 0) return hipSuccess;
  if (m.dev <= 0 || m.both || !preempt_profile_ok(c, m, plane, dw)) return hipErrorInvalidValue;
  const int32_t nb = preempt_blocks(d.n);
  const NumaPlane pl{plane, (d.n + 63) / 64};
  StreamFlags fl{};
  fl.full = 1;  // the chain: every block, every preemptor
  hipLaunchKernelGGL(k_stream_init, dim3(1), dim3(64), 0, s, pdb, fl, st);
  with_walk_dev(m, [&](auto numa, auto dev) {
    constexpr bool NUMA = decltype(numa)::value;
    constexpr int DEV = decltype(dev)::value;
    const dim3 blocks(nb), threads(PREEMPT_THREADS), wave(64);
    for (int32_t k = 0; k < n_pre; k++) {
      hipLaunchKernelGGL((k_preempt_seq_dev<NUMA, DEV>), blocks, threads, 0, s, c, d, tab, off, pre, k, st, pl, dw);
      hipLaunchKernelGGL(k_preempt_seq_pick, dim3(1), wave, 0, s, nb, k, st);
      hipLaunchKernelGGL((k_preempt_apply_dev<NUMA, DEV>), dim3(1), wave, 0, s, c, d, tab, off, pre, n_pre, k, st,
                         max_victims, dw);
    }
  });
  return hipGetLastError();
}

hipError_t launch_preempt_pick(const DevCfg &c, const DevNodes &d, const DevAsg *tab, const int32_t *off,
                               const PdbAllowed &pdb, const DevPre *pre, int32_t n_pre, const int32_t *count,
                               const PreemptPartial *part, koordhip_preempt_result *res, int32_t *victims,
                               int32_t max_victims, WalkMode m, hipStream_t s, DevWalk dw) {
  if (n_pre <= 0 || d.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_preempt_pick, dim3(n_pre), dim3(64), 0, s, part, preempt_blocks(d.n), count, res);
  if (victims && max_victims > 0 && m.both)
    with_walk_dev_resv(m, [&](auto numa, auto rs, auto dev) {
      hipLaunchKernelGGL(
          (k_preempt_victims_dev_resv<decltype(numa)::value, decltype(rs)::value, decltype(dev)::value>),
          dim3((n_pre + 63) / 64), dim3(64), 0, s, c, d, tab, off, pdb, pre, n_pre, res, victims, max_victims, dw);
    });
  else if (victims && max_victims > 0 && m.dev > 0)
    with_walk_dev(m, [&](auto numa, auto dev) {
      hipLaunchKernelGGL((k_preempt_victims_dev<decltype(numa)::value, decltype(dev)::value>),
                         dim3((n_pre + 63) / 64), dim3(64), 0, s, c, d, tab, off, pdb, pre, n_pre, res, victims,
                         max_victims, dw);
    });
  else if (victims && max_victims > 0)
    with_walk(m, [&](auto numa, auto rs) {
      hipLaunchKernelGGL((k_preempt_victims<decltype(numa)::value, decltype(rs)::value>), dim3((n_pre + 63) / 64),
                         dim3(64), 0, s, c, d, tab, off, pdb, pre, n_pre, res, victims, max_victims);
    });
  return hipGetLastError();
}

}  // namespace kh
