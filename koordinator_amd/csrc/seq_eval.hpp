// seq_eval.hpp -- one (pod, node) of the sequential cycle: seq_eval, the
// Filter of every plugin evaluated per node (its status bits), the weighted
// total of the per-node plugins and the raw normalized scores, with the
// side-row modes it is compiled for.  Shared by seq.hip (the cycle and the
// parity evaluator) and diag_ext.hip (the diagnosis of these profiles).
#pragma once
#include <hip/hip_runtime.h>

#include "dev.hpp"

namespace kh {

// SM: the compiled side-row mode -- 0 none (Fit / LoadAware / static /
// balanced), 1 + NodeNUMAResource (with the zone code), 2 + Reservation (the
// 4-slot rows, with NUMA when enabled), 3 the same with the 8-slot rows
// (more than KOORDHIP_RESV_SLOTS reservations on a node).  The plain build
// keeps no side row at all: a zero-initialised ~0.5 KB row per lane would live
// in scratch.
__host__ __device__ constexpr int seq_mode(const DevCfg &c) {
  return c.resv ? (c.resv_slots > KOORDHIP_RESV_SLOTS ? 3 : 2) : (((c.filt | c.score) & KOORDHIP_PLUGIN_NUMA) ? 1 : 0);
}
// k_seq's instantiation: the Reservation builds without DeviceShare and
// without a reservation holding devices or extended scalars take 4 / 5
static inline int seq_launch_mode(const DevCfg &c, const DevNodes &d) {
  const int sm = seq_mode(c);
  const bool nodev = !((c.filt | c.score) & KOORDHIP_PLUGIN_DEVICESHARE) && !d.dv.rslot && !d.dv.rxa;
  return (sm >= 2 && nodev) ? sm + 2 : sm;
}
// k_seq only: SM 4 / 5 = SM 2 / 3 without DeviceShare and without a
// reservation holding devices (the device and device-reservation code compiled
// out: the Reservation + NodeNUMAResource profiles keep their registers)
template <int SM>
constexpr int kSeqSlots = (SM == 3 || SM == 5) ? KOORDHIP_RESV_SLOTS_MAX : KOORDHIP_RESV_SLOTS;
template <int SM>
constexpr bool kSeqDev = SM < 4;
template <int SM>
using SeqResvRow = NumaRowRS<kSeqSlots<SM>>;

// The node's reservation holding devices, for a device pod under DeviceShare
// (KH_POD_DEVSHARE): its DevRC (dev.hpp; h -1: none) and DeviceShare's
// FilterReservation of it, recorded in its slot's rdev -- the nomination's only
// possible candidate for the pod (resv_nominate).
template <int S>
__device__ __forceinline__ DevRC seq_dev_resv(const DevCfg &c, const DevDev &dv, const DevPod &p, const DevPodX &x,
                                              NumaRowRS<S> &r, int32_t i) {
  DevRC rc{-1, 0, 0, 0u};
  if (!dv.rslot || !c.resv || !(p.flags & KH_POD_DEVSHARE)) return rc;
  const int32_t h = dv.rslot[i];
  if (h < 0 || h >= S) return rc;
  int32_t cls = 0;
  uint32_t rf = 0u;
#pragma unroll
  for (int q = 0; q < S; q++)
    if (q == h) {
      cls = resv_class(r.rs[q], p);
      rf = r.rs[q].rf;
    }
  rc = rc_of(c, dv, i, h, cls, rf);
  if (rc.h >= 0 && rc.cls == 1 && rc_filter_reservation(c, dv, x, i, rc))
#pragma unroll
    for (int q = 0; q < S; q++)
      if (q == h) r.rs[q].rdev = 1;
  return rc;
}

// ABI 14: resv.hpp's ResvXS for pod (p, x) on node i, whose reservation
// holding devices is slot h with restore class `cls` (1 matched, 2 unmatched
// with assigned pods, 0 neither), from its extended scalars (Allocatable A,
// Allocated D, remainder max0(A - D); a listed key has A > 0) and the node's
// scalar Allocatable / Requested.  Rare (a node whose reservation lists
// extended scalars), so out of line: the common path keeps its registers.
__device__ __noinline__ ResvXS resv_scalars(const DevDev &dv, const DevPodX &x, int32_t i, int32_t n, int32_t h,
                                            int cls) {
  ResvXS rx{h, RX_FIT_H | RX_FIT_O | RX_LE | RX_XFIT, 0, 0};
  for (int j = 0; j < KOORDHIP_NXRES; j++) {
    const size_t at = (size_t)j * n + i;
    const int64_t A = dv.rxa[at], D = dv.rxd[at];
    const int64_t rem = A - D > 0 ? A - D : 0;
    const bool key = (x.xmask >> j) & 1u;
    const int64_t px = key ? x.xreq[j] : 0;
    if (rem > 0) rx.f |= RX_REM;
    if (A != 0) {  // RemoveZeros(Allocatable) / ResourceNames
      rx.xw++;
      const int64_t req = px + D;  // scoreReservation: PodRequestsAndLimits + Allocated
      if (req <= A) rx.xs += (int32_t)(100 * req / A);
      if (key) {
        rx.f |= RX_INTER | (rem > 0 ? RX_NZ : 0u);
        if (px > rem) rx.f &= ~RX_LE;
      }
    }
    if (!key) continue;
    const int64_t alloc = dv.xalloc ? dv.xalloc[at] : 0, xr = dv.xreq[at];
    // NodeResourcesFit on the restored NodeInfo: the reserve pod leaves, an
    // unmatched reservation's remainder comes back (transformer.go:227-293)
    if (px > alloc - (xr - (cls != 0 ? A : 0) + (cls == 2 ? rem : 0))) rx.f &= ~RX_XFIT;
    // fitsNode: podRequested after the unmatched restore, allRAllocated = D when matched
    const int64_t preq = xr + (cls == 2 ? rem - A : 0), rall = cls == 1 ? D : 0;
    if (px > alloc - (preq - rem - rall)) rx.f &= ~RX_FIT_H;
    if (px > alloc - (preq - rall)) rx.f &= ~RX_FIT_O;
  }
  return rx;
}

// the ResvXS of node i's reservation holding devices for the pod (h -1: none)
template <int S>
__device__ __forceinline__ ResvXS seq_resv_x(const DevNodes &d, const DevPod &p, const DevPodX &x,
                                             const NumaRowRS<S> &r, int32_t i) {
  if (!d.dv.rxa) return no_rx();
  const int32_t h = d.dv.rslot[i];
  if (h < 0 || h >= S) return no_rx();
  int cls = 0;
#pragma unroll
  for (int q = 0; q < S; q++)
    if (q == h) cls = resv_class(r.rs[q], p);
  return resv_scalars(d.dv, x, i, d.n, h, cls);
}

// The diagnosis' reasons-only sibling of resv_scalars: which extended scalars
// fail its RX_XFIT term (NodeResourcesFit on the restored NodeInfo), bit j =
// scalar j; 0 iff resv_scalars leaves RX_XFIT set.  Out of line for the same
// reason (`inline` for the linkage only: a unit that never asks gets no copy).
inline __device__ __noinline__ uint32_t resv_xfit_reasons(const DevDev &dv, const DevPodX &x, int32_t i, int32_t n, int cls) {
  uint32_t m = 0u;
  for (int j = 0; j < KOORDHIP_NXRES; j++) {
    if (!((x.xmask >> j) & 1u)) continue;
    const size_t at = (size_t)j * n + i;
    const int64_t A = dv.rxa[at], D = dv.rxd[at];
    const int64_t rem = A - D > 0 ? A - D : 0;
    const int64_t alloc = dv.xalloc ? dv.xalloc[at] : 0, xr = dv.xreq[at];
    if (x.xreq[j] > alloc - (xr - (cls != 0 ? A : 0) + (cls == 2 ? rem : 0))) m |= 1u << j;
  }
  return m;
}

// NodeResourcesFit's failing extended scalars for the pod on node i as
// seq_eval's XFIT bit sees them: on the restored scalars where the node's
// reservation holds devices (seq_resv_x names a slot), else xfit_reasons
template <int S>
__device__ __forceinline__ uint32_t seq_xfit_reasons(const DevNodes &d, const DevPod &p, const DevPodX &x,
                                                     const NumaRowRS<S> &r, int32_t i) {
  const int32_t h = d.dv.rxa ? d.dv.rslot[i] : -1;
  if (h < 0 || h >= S) return xfit_reasons(d.dv, x, i, d.n);
  int cls = 0;
#pragma unroll
  for (int q = 0; q < S; q++)
    if (q == h) cls = resv_class(r.rs[q], p);
  return resv_xfit_reasons(d.dv, x, i, d.n, cls);
}

// One node for one pod: the total of the per-node plugins (-1: some Filter
// fails; with the Reservation plugin the ranking total of resv.hpp) and the
// raw normalized scores.  Every column is read (the parity evaluator's rows,
// like k_eval_full).  Inlined once per kernel: a call keeps its frame (the
// config and column descriptors, the NV row) in scratch, kilobytes per lane.
// EARLY (k_ext_pre / k_ext_final: no status, no raw planes of infeasible nodes): a node
// whose extended scalars do not fit returns -1 before any other load.
template <int SM, bool EARLY = false>
__device__ __forceinline__ int32_t seq_eval(const DevCfg &c, const DevNodes &d, const DevPod &p, const DevPodX &x,
                                            int32_t i, bool rs, int32_t raw[KOORDHIP_NEXT_PLUGINS],
                                            uint8_t *status) {
  if constexpr (EARLY)
    if ((c.filt & KOORDHIP_PLUGIN_FIT) && !xfit_filter(d.dv, x, i, d.n)) return -1;
  NV v{};
  const Need all = need_all(c);
  load_node(v, d, i, all, c);
  // the reads that do not depend on the node row next, so their round trips
  // overlap the row's: the extended scalars, the static Scores and (without
  // the Reservation build, whose nomination needs the reservation rows) the
  // device rows
  bool xfr = EARLY || !(c.filt & KOORDHIP_PLUGIN_FIT) || xfit_filter(d.dv, x, i, d.n);
  raw[1] = (c.score & KOORDHIP_PLUGIN_AFFINITY_SCORE) ? static_raw(d.dv, 0, p.sclass, i, d.n) : 0;
  raw[2] = (c.score & KOORDHIP_PLUGIN_TAINT_SCORE) ? static_raw(d.dv, 1, p.sclass, i, d.n) : 0;
  int32_t t;
  bool df = true, rfail = false;
  if constexpr (SM >= 2) {
    constexpr int S = kSeqSlots<SM>;
    SeqResvRow<SM> nr{};
    load_numa<false>(nr, d, i, all);  // (the zone row shares the reserved CPUs' bytes: eval_total_resv<.., Z> reads it)
    load_resv(nr, d.rv, i);
    DevRC rc{-1, 0, 0, 0u};
    ResvXS rx = no_rx();
    if constexpr (kSeqDev<SM>) {
      rc = seq_dev_resv(c, d.dv, p, x, nr, i);
      rx = seq_resv_x(d, p, x, nr, i);
      if (rx.h >= 0 && (c.filt & KOORDHIP_PLUGIN_FIT)) xfr = (rx.f & RX_XFIT) != 0u;  // on the restored scalars
    }
    t = c.zones       ? eval_total_resv<S, true, true>(p, v, nr, d.nu.cls, c, &d, i, rx)
        : c.resv_cpus ? eval_total_resv<S, true>(p, v, nr, d.nu.cls, c, nullptr, 0, rx)
                      : eval_total_resv<S, false>(p, v, nr, d.nu.cls, c, nullptr, 0, rx);
    if constexpr (kSeqDev<SM>) {
      const int32_t nq = (rs && (x.flags & KOORDHIP_PODX_DEVICE)) ? resv_nominate(p, nr, resv_matched(nr, p), rx) : -1;
      if (rc.h >= 0)
        df = rc_eval(c, d.dv, x, i, rc, nq, (c.filt & KOORDHIP_PLUGIN_DEVICESHARE) != 0,
                     (c.score & KOORDHIP_PLUGIN_DEVICESHARE) != 0, &raw[0]);
      else
        df = dev_eval(c, d.dv, x, i, nq >= 0, (c.filt & KOORDHIP_PLUGIN_DEVICESHARE) != 0,
                      (c.score & KOORDHIP_PLUGIN_DEVICESHARE) != 0, &raw[0]);
    }
    if ((p.flags & (KOORDHIP_POD_RESERVE | KOORDHIP_POD_RESV_OPERATING)) && (c.filt & KOORDHIP_PLUGIN_RESERVATION) &&
        !reserve_pod_ok(p, (p.flags & KOORDHIP_POD_RESERVE) ? x.reserve_node : 0, nr, i))
      rfail = true;
  } else {
    df = dev_eval(c, d.dv, x, i, false, (c.filt & KOORDHIP_PLUGIN_DEVICESHARE) != 0,
                  (c.score & KOORDHIP_PLUGIN_DEVICESHARE) != 0, &raw[0]);
    if constexpr (SM == 1) {
      NumaRow nr{};
      load_numa<true>(nr, d, i, all);
      t = eval_total_numa<true>(p, v, nr, d.nu.cls, c);
    } else {
      t = eval_total(p, v, c);
    }
  }
  const bool xf = xfr;
  if (status)
    *status = (xf ? 0 : KOORDHIP_ST_XFIT_FAIL) | (df ? 0 : KOORDHIP_ST_DEVICE_FAIL) | (rfail ? KOORDHIP_ST_RESV_FAIL : 0);
  if (!xf || !df || rfail) t = -1;
  raw[3] = 0;  // PodTopologySpread: its own phases (pts.hpp)
  raw[4] = 0;  // InterPodAffinity: ipa.hpp
  return t;
}

}  // namespace kh
