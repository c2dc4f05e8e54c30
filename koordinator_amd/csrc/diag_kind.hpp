// diag_kind.hpp -- what the diagnosis kernels share.  For diag.hip, reasons.hip
// and diag_ext.hip: the tile shape, the pod-tile stager, the load of the row
// the Filter reads, the status counting, the reason counting (reasons.hip and
// diag_ext.hip's reason kind) and the LDS-table flush.  For diag.hip
// and reasons.hip also their two kernels, parameterised on what they evaluate
// and count per (pod, node):
//   k_diag_current<K, S>   pods against the current state
//   k_diag_replay<K>       the unplaced pods of the last place call at their decision states
//
// A kind K supplies
//   K::WORDS                                  int32 counters of one pod's record
//   K::Plane                                  a node's value in the single-pod form
//   K::slots(c)                               the counters the profile can produce (wave-uniform)
//   K::eval(c, pod, v, nr, cls, nmatch, mm)   the (pod, node) value on the restored row; nr any NumaRowRS<S>
//   K::count(x, live, slots, rec)             one wave's 64 values into a pod's LDS record
// diag.hip instantiates them with the KOORDHIP_ST_* status (koordhip_diag),
// reasons.hip with the KOORDHIP_REASON_* mask (koordhip_reasons).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "diag.h"
#include "eval.hpp"

namespace kh {

constexpr int DIAG_THREADS = 256;
constexpr int DIAG_PT = 32;                 // pods per LDS tile
constexpr int DIAG_ANY = (int)(offsetof(koordhip_diag, any) / sizeof(int32_t));
constexpr int DIAG_FIRST = (int)(offsetof(koordhip_diag, first) / sizeof(int32_t));
constexpr int DIAG_STATUS_BITS = 9;         // status bits 0..8: FIT, LA, NUMA, RESV, STATIC, DEVICE, XFIT, PTS, IPA
static_assert(KOORDHIP_ST_IPA_FAIL == 1u << (DIAG_STATUS_BITS - 1) && DIAG_STATUS_BITS <= KOORDHIP_DIAG_BITS,
              "the status bits are bits 0..8");

// a pod record as the 8-B words it is staged in
template <class T>
constexpr int tile_words() {
  static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % sizeof(uint64_t) == 0,
                "pod records are staged as 8-B words");
  return (int)(sizeof(T) / sizeof(uint64_t));
}

// np contiguous records src[0, np) -> the workgroup's LDS tile (a barrier follows at the caller)
template <class T>
__device__ __forceinline__ void stage_tile(uint64_t *lds, const T *src, int32_t np) {
  const uint64_t *s = reinterpret_cast<const uint64_t *>(src);
  for (int32_t w = threadIdx.x; w < np * tile_words<T>(); w += DIAG_THREADS) lds[w] = s[w];
}

// node il's row as the Filter reads it: every column the profile enables and,
// with reservation columns (S > 1), the node's reservations
template <int S>
__device__ __forceinline__ void load_filter_row(const DevCfg &c, const DevNodes &d, int32_t il, NV &v,
                                                NumaRowRS<S> &nr) {
  const Need all = need_all(c);
  load_node(v, d, il, all, c);
  load_numa<true>(nr, d, il, all);
  if constexpr (S > 1) {
    if (c.resv) {
      load_resv(nr, d.rv, il);
      // a topology-policy node's zone row shares the reserved CPUs' bytes (the Filter reads the zones only)
      if (c.zones && topo_policy(nr.nflags) != 0) load_zones(nr, d, il);
    }
  }
}

// The first failing plugin in the framework's Filter order (koordhip.h):
// STATIC -> FIT -> XFIT -> PTS -> IPA -> LA -> NUMA -> DEVICE -> RESV.
constexpr uint32_t first_fail(uint32_t st) {
  constexpr uint32_t order[DIAG_STATUS_BITS] = {KOORDHIP_ST_STATIC_FAIL, KOORDHIP_ST_FIT_FAIL,    KOORDHIP_ST_XFIT_FAIL,
                                                KOORDHIP_ST_PTS_FAIL,    KOORDHIP_ST_IPA_FAIL,    KOORDHIP_ST_LA_FAIL,
                                                KOORDHIP_ST_NUMA_FAIL,   KOORDHIP_ST_DEVICE_FAIL, KOORDHIP_ST_RESV_FAIL};
  uint32_t f = 0u;
  for (int k = DIAG_STATUS_BITS - 1; k >= 0; k--) f = (st & order[k]) ? order[k] : f;
  return f;
}

// on the five bits of the profiles outside the sequential cycle (bits 0..4): the static bit, else the lowest set bit
constexpr bool first_fail_five_bit_rule() {
  for (uint32_t st = 0; st < 32u; st++)
    if (first_fail(st) != ((st & KOORDHIP_ST_STATIC_FAIL) ? (uint32_t)KOORDHIP_ST_STATIC_FAIL : (st & (0u - st))))
      return false;
  return true;
}
static_assert(first_fail_five_bit_rule(), "STATIC -> FIT -> LA -> NUMA -> RESV on status bits 0..4");

// One wave's 64 nodes into a pod's LDS koordhip_diag record: status bits
// 0..NBITS-1, of which the profile can produce `bits`; first = first_fail(st).
// Called by every lane of the wave (the ballots are wave-wide); lanes that are
// not `live` count nowhere.
template <int NBITS>
__device__ __forceinline__ void status_count(uint32_t st, uint32_t first, bool live, uint32_t bits, int32_t *rec) {
  const bool l0 = __lane_id() == 0;
  const uint64_t ok = __ballot(live && st == 0u);
  if (l0 && ok) atomicAdd(&rec[0], (int32_t)__popcll(ok));
#pragma unroll
  for (int b = 0; b < NBITS; b++) {
    if (!((bits >> b) & 1u)) continue;
    const uint64_t ma = __ballot(live && ((st >> b) & 1u) != 0u);
    const uint64_t mf = __ballot(live && first == (1u << b));
    if (l0 && ma) atomicAdd(&rec[DIAG_ANY + b], (int32_t)__popcll(ma));
    if (l0 && mf) atomicAdd(&rec[DIAG_FIRST + b], (int32_t)__popcll(mf));
  }
}

// the workgroup's LDS records of np pods -> out (np contiguous records of W words)
template <int W>
__device__ __forceinline__ void diag_flush(const int32_t *tab, int32_t np, int32_t *out) {
  for (int32_t w = threadIdx.x; w < np * W; w += DIAG_THREADS) {
    const int32_t x = tab[w];
    if (x) atomicAdd(&out[w], x);
  }
}

// ---------------------------------------------------------------------------
// the reason kind's counting (reasons.hip, and diag_ext.hip's reason variant)

constexpr int RS_UNRES = (int)(offsetof(koordhip_reasons, unresolvable) / sizeof(int32_t));
constexpr int RS_FIRST = (int)(offsetof(koordhip_reasons, first) / sizeof(int32_t));
constexpr int RS_ANY = (int)(offsetof(koordhip_reasons, any) / sizeof(int32_t));

// The reasons of the first failing plugin in the framework's Filter order
// STATIC -> FIT -> LA -> NUMA -> RESV (koordhip.h): the plugins' slots lie in
// that order, so it is the group of the lowest set bit.
__device__ __forceinline__ uint32_t first_reasons(uint32_t m) {
  const uint32_t low = m & (0u - m);
  const uint32_t g = (low & KOORDHIP_REASONS_OF_STATIC) ? KOORDHIP_REASONS_OF_STATIC
                     : (low & KOORDHIP_REASONS_OF_FIT)  ? KOORDHIP_REASONS_OF_FIT
                     : (low & KOORDHIP_REASONS_OF_LA)   ? KOORDHIP_REASONS_OF_LA
                     : (low & KOORDHIP_REASONS_OF_NUMA) ? KOORDHIP_REASONS_OF_NUMA
                                                        : KOORDHIP_REASONS_OF_RESV;
  return m & g;
}

// ... with the sequential cycle's plugins, first_fail's order: STATIC -> FIT u
// XFIT (one plugin) -> PTS -> IPA -> LA -> NUMA -> DEVICE -> RESV.  The slots
// 19-31 do not lie in that order, so the groups are walked.
constexpr uint32_t first_reasons_ext(uint32_t m) {
  constexpr uint32_t order[8] = {KOORDHIP_REASONS_OF_STATIC, KOORDHIP_REASONS_OF_FIT | KOORDHIP_REASONS_OF_XFIT,
                                 KOORDHIP_REASONS_OF_PTS,    KOORDHIP_REASONS_OF_IPA,
                                 KOORDHIP_REASONS_OF_LA,     KOORDHIP_REASONS_OF_NUMA,
                                 KOORDHIP_REASONS_OF_DEVICE, KOORDHIP_REASONS_OF_RESV};
  uint32_t f = 0u;
  for (int k = 7; k >= 0; k--) f = (m & order[k]) ? (m & order[k]) : f;
  return f;
}

// restricted to slots 0..18 it is first_reasons' rule (checked on one reason per group and on pairs of groups)
constexpr bool first_reasons_ext_base_rule() {
  constexpr uint32_t g[5] = {KOORDHIP_REASONS_OF_STATIC, KOORDHIP_REASONS_OF_FIT, KOORDHIP_REASONS_OF_LA,
                             KOORDHIP_REASONS_OF_NUMA, KOORDHIP_REASONS_OF_RESV};
  for (int a = 0; a < 5; a++)
    for (int b = a; b < 5; b++)
      if (first_reasons_ext(g[a] | g[b]) != g[a]) return false;
  return true;
}
static_assert(first_reasons_ext_base_rule(), "STATIC -> FIT -> LA -> NUMA -> RESV on reason slots 0..18");

// the reason slots the profile's Filter plugins can set (wave-uniform)
__device__ __forceinline__ uint32_t reason_slots(const DevCfg &c) {
  uint32_t numa = KOORDHIP_REASONS_OF_NUMA;
  if (!c.amp) numa &= ~reason_bit(KOORDHIP_REASON_NUMA_AMP_CPU);
  if (!c.zones) numa &= ~(reason_bit(KOORDHIP_REASON_NUMA_NO_ZONES) | reason_bit(KOORDHIP_REASON_NUMA_POLICY));
  // without reservation columns no node has a matched reservation: only the affinity exit is left
  const uint32_t resv = c.resv ? KOORDHIP_REASONS_OF_RESV : reason_bit(KOORDHIP_REASON_RESV_AFFINITY);
  return ((c.filt & KOORDHIP_PLUGIN_NODE_STATIC) ? KOORDHIP_REASONS_OF_STATIC : 0u) |
         ((c.filt & KOORDHIP_PLUGIN_FIT) ? KOORDHIP_REASONS_OF_FIT : 0u) |
         ((c.filt & KOORDHIP_PLUGIN_LOADAWARE) ? KOORDHIP_REASONS_OF_LA : 0u) |
         ((c.filt & KOORDHIP_PLUGIN_NUMA) ? numa : 0u) |
         ((c.filt & KOORDHIP_PLUGIN_RESERVATION) ? resv : 0u);
}

// ... with the sequential cycle's plugins: the extended scalars belong to
// NodeResourcesFit; DeviceShare's verdict comes from dev_eval / rc_eval, which
// also answer for a Score-only DeviceShare; pts / ipa: their Filter is on and
// the snapshot has their tables (k_diag_ext's pts_on / ipa_on)
__device__ __forceinline__ uint32_t reason_slots_ext(const DevCfg &c, bool pts, bool ipa) {
  return reason_slots(c) | ((c.filt & KOORDHIP_PLUGIN_FIT) ? KOORDHIP_REASONS_OF_XFIT : 0u) |
         (((c.filt | c.score) & KOORDHIP_PLUGIN_DEVICESHARE) ? KOORDHIP_REASONS_OF_DEVICE : 0u) |
         (pts ? KOORDHIP_REASONS_OF_PTS : 0u) | (ipa ? KOORDHIP_REASONS_OF_IPA : 0u);
}

// One wave's 64 nodes into a pod's LDS koordhip_reasons record: reason slots
// 0..NSLOTS-1, of which the profile can produce `slots`; f = the reasons of the
// node's first failing plugin, uu = the UnschedulableAndUnresolvable reasons.
// The ballots of slots the profile cannot produce, and the first-ballot of a
// reason no lane of the wave has, are skipped.  Called by every lane of the
// wave (the ballots are wave-wide); lanes that are not `live` count nowhere.
template <int NSLOTS>
__device__ __forceinline__ void reasons_count(uint32_t m, uint32_t f, uint32_t uu_mask, bool live, uint32_t slots,
                                              int32_t *rec) {
  const bool l0 = __lane_id() == 0;
  const uint64_t ok = __ballot(live && m == 0u);
  const uint64_t uu = __ballot(live && (f & uu_mask) != 0u);
  if (l0 && ok) atomicAdd(&rec[0], (int32_t)__popcll(ok));
  if (l0 && uu) atomicAdd(&rec[RS_UNRES], (int32_t)__popcll(uu));
#pragma unroll
  for (int b = 0; b < NSLOTS; b++) {
    if (!((slots >> b) & 1u)) continue;
    const uint64_t ma = __ballot(live && ((m >> b) & 1u) != 0u);
    if (!ma) continue;  // wave-uniform: no lane has the reason, so none has it first
    const uint64_t mf = __ballot(live && ((f >> b) & 1u) != 0u);
    if (l0) atomicAdd(&rec[RS_ANY + b], (int32_t)__popcll(ma));
    if (l0 && mf) atomicAdd(&rec[RS_FIRST + b], (int32_t)__popcll(mf));
  }
}

// k_diag_current: 256-node tiles x 32-pod tiles; S = the reservation slots of
// the side row (1: no reservation columns).  A thread loads its node's row once
// and, per pod of the tile (staged in LDS), restores on a copy and evaluates.
// Per counter one ballot + popcount per wave, lane 0 adds into an LDS table of
// whole records, the workgroup flushes its non-zero entries with atomics on
// consecutive words.  With a plane pointer (one pod): the node's value instead
// of a record.
template <class K, int S>
__global__ __launch_bounds__(DIAG_THREADS) void k_diag_current(DevCfg c, DevNodes d, const DevPod *__restrict__ pods,
                                                               int32_t n_pods, int32_t *__restrict__ out,
                                                               typename K::Plane *__restrict__ plane) {
  __shared__ __attribute__((aligned(16))) uint64_t spw[DIAG_PT * tile_words<DevPod>()];
  __shared__ int32_t tab[DIAG_PT * K::WORDS];
  const int t = threadIdx.x;
  const int32_t p0 = (int32_t)blockIdx.y * DIAG_PT;
  const int32_t np = min(DIAG_PT, n_pods - p0);
  stage_tile(spw, pods + p0, np);
  for (int32_t w = t; w < np * K::WORDS; w += DIAG_THREADS) tab[w] = 0;
  __syncthreads();
  const DevPod *sp = reinterpret_cast<const DevPod *>(spw);
  const int32_t i = (int32_t)blockIdx.x * DIAG_THREADS + t;
  const bool live = i < d.n;
  const int32_t il = live ? i : d.n - 1;  // tail lanes read the last row and count nowhere
  NV v{};
  NumaRowRS<S> nr{};
  load_filter_row(c, d, il, v, nr);
  const uint32_t slots = K::slots(c);
  for (int32_t q = 0; q < np; q++) {
    const DevPod pod = sp[q];
    NV w = v;
    int nmatch = 0;
    uint32_t mm = 0;
    if constexpr (S > 1) {
      if (c.resv) nmatch = resv_restore(w, nr, pod, mm);  // the cycle's restore: every plugin sees the restored node
    }
    const uint32_t x = K::eval(c, pod, w, nr, d.nu.cls, nmatch, mm);
    if (plane) {
      if (live) plane[i] = (typename K::Plane)x;
    } else {
      K::count(x, live, slots, tab + q * K::WORDS);
    }
  }
  __syncthreads();
  if (!plane) diag_flush<K::WORDS>(tab, np, out + (size_t)p0 * K::WORDS);
}

template <class K>
hipError_t launch_current(const DevCfg &c, const DevNodes &d, const DevPod *pods, int32_t n_pods, int32_t *out,
                          typename K::Plane *plane, hipStream_t s) {
  if (n_pods <= 0 || d.n <= 0) return hipSuccess;
  if ((plane && n_pods != 1) || (!plane && !out)) return hipErrorInvalidValue;
  const dim3 grid((d.n + DIAG_THREADS - 1) / DIAG_THREADS, (n_pods + DIAG_PT - 1) / DIAG_PT);
  if (grid.y > 65535u) return hipErrorInvalidValue;
  if (c.resv)
    hipLaunchKernelGGL((k_diag_current<K, KOORDHIP_RESV_SLOTS_MAX>), grid, dim3(DIAG_THREADS), 0, s, c, d, pods, n_pods,
                       out, plane);
  else
    hipLaunchKernelGGL((k_diag_current<K, 1>), grid, dim3(DIAG_THREADS), 0, s, c, d, pods, n_pods, out, plane);
  return hipGetLastError();
}

// k_diag_replay: a commit is exactly invertible (apply_delta / numa_apply with
// sign -1, integers held in f64, order-independent), so no copy of the table is
// kept: a thread loads its node's FINAL row, walks the unplaced pods in
// descending order and, before it evaluates pod u, un-applies its node's
// commits with a pod index > u.  Workgroup (x, y) takes nodes [256 x, 256 x +
// 256) and the tiles [y tpb, (y + 1) tpb) of the unplaced list, last tile
// first.  The loop over the unplaced pods is wave-uniform (the ballots are
// valid); only the walk over a node's commits diverges.
template <class K>
__global__ __launch_bounds__(DIAG_THREADS) void k_diag_replay(DevCfg c, DevNodes d, const DevPod *__restrict__ pods,
                                                              const uint64_t *__restrict__ cpus,
                                                              const int32_t *__restrict__ off,
                                                              const int32_t *__restrict__ nl,
                                                              const int32_t *__restrict__ ul, int32_t U, int32_t single,
                                                              int32_t tpb, int32_t *__restrict__ out,
                                                              typename K::Plane *__restrict__ plane) {
  constexpr int POD_WORDS = tile_words<DevPod>();
  __shared__ __attribute__((aligned(16))) uint64_t spw[DIAG_PT * POD_WORDS];
  __shared__ int32_t su[DIAG_PT];
  __shared__ int32_t tab[DIAG_PT * K::WORDS];
  const int t = threadIdx.x;
  const int32_t i = (int32_t)blockIdx.x * DIAG_THREADS + t;
  const bool live = i < d.n;
  const int32_t il = live ? i : d.n - 1;
  NV v{};
  NumaRowR nr{};
  load_filter_row(c, d, il, v, nr);
  const int32_t lo = live ? off[il] : 0;
  int32_t ptr = live ? off[il + 1] : 0;  // this node's commits nl[ptr ..) are un-applied
  const bool numa = numa_on(c) && cpus != nullptr;
  const uint32_t slots = K::slots(c);
  const DevPod *sp = reinterpret_cast<const DevPod *>(spw);
  const int32_t ntiles = (U + DIAG_PT - 1) / DIAG_PT;
  const int32_t ty0 = (int32_t)blockIdx.y * tpb, ty1 = min(ntiles, ty0 + tpb);
  for (int32_t tile = ty1 - 1; tile >= ty0; tile--) {
    const int32_t k0 = tile * DIAG_PT, nk = min(DIAG_PT, U - k0);
    __syncthreads();  // the previous tile's flush has read tab
    if (t < nk) su[t] = single >= 0 ? single : ul[k0 + t];
    for (int32_t w = t; w < nk * K::WORDS; w += DIAG_THREADS) tab[w] = 0;
    __syncthreads();
    for (int32_t w = t; w < nk * POD_WORDS; w += DIAG_THREADS) {  // a gather: the tile's pods are ul's, not contiguous
      const int32_t q = w / POD_WORDS;
      spw[w] = reinterpret_cast<const uint64_t *>(pods + su[q])[w - q * POD_WORDS];
    }
    __syncthreads();
    for (int32_t q = nk - 1; q >= 0; q--) {
      const int32_t pu = su[q];
      while (ptr > lo) {  // Unreserve this node's commits made after pod pu's decision
        const int32_t j = nl[ptr - 1];
        if (j < pu) break;
        ptr--;
        const DevPod pj = pods[j];
        apply_delta(v, pj, -1);
        if (numa && is_cpuset(pj)) {
          uint64_t m[NW];
#pragma unroll
          for (int w = 0; w < NW; w++) m[w] = cpus[(size_t)j * NW + w];
          numa_apply(nr, pj, m, -1);
        }
      }
      const DevPod pod = sp[q];
      const uint32_t x = K::eval(c, pod, v, nr, d.nu.cls, 0, 0u);  // no reservation columns in the replay's envelope
      if (plane) {
        if (live) plane[i] = (typename K::Plane)x;
      } else {
        K::count(x, live, slots, tab + q * K::WORDS);
      }
    }
    __syncthreads();
    if (!plane) diag_flush<K::WORDS>(tab, nk, out + (size_t)k0 * K::WORDS);
  }
}

template <class K>
hipError_t launch_replay(const DevCfg &c, const DevNodes &d, const DevPod *pods, const uint64_t *cpus,
                         const DiagLists &l, int32_t U, int32_t single, int32_t *out, typename K::Plane *plane,
                         hipStream_t s) {
  if (U <= 0 || d.n <= 0) return hipSuccess;
  if (c.resv || c.zones) return hipErrorInvalidValue;  // their Reserve is not invertible from what the engine keeps
  if ((single >= 0 && U != 1) || (plane && single < 0) || (!plane && !out)) return hipErrorInvalidValue;
  const int32_t gx = (d.n + DIAG_THREADS - 1) / DIAG_THREADS;
  const int32_t ntiles = (U + DIAG_PT - 1) / DIAG_PT;
  // enough workgroups to fill the device; a workgroup's later tiles go on from the row state of its earlier ones
  const int32_t gy = std::max(1, std::min(ntiles, std::min(65535, (1024 + gx - 1) / gx)));
  const int32_t tpb = (ntiles + gy - 1) / gy;
  hipLaunchKernelGGL(k_diag_replay<K>, dim3(gx, (ntiles + tpb - 1) / tpb), dim3(DIAG_THREADS), 0, s, c, d, pods, cpus,
                     l.off, l.nl, l.ul, U, single, tpb, out, plane);
  return hipGetLastError();
}

}  // namespace kh
