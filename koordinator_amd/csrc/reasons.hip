// reasons.hip -- why a pod is unschedulable, one step past diag.hip: per
// Status reason (KOORDHIP_REASON_*) the node counts FitError.Error() prints,
// and how many of the failing nodes are UnschedulableAndUnresolvable
// (koordhip_reasons), reduced on device.
//
//   k_reasons         k_diag's shape: 256-node tiles x 32-pod tiles; a thread
//                     loads its node row once and, per pod (staged in LDS),
//                     restores on a copy and evaluates filter_reasons.  Per
//                     counter one ballot + popcount per wave, lane 0 adds into
//                     an LDS table of whole records (32 x 66 words), the
//                     workgroup flushes its non-zero entries with atomics on
//                     consecutive words.  The ballots of slots the profile
//                     cannot produce are skipped.  With a mask pointer and one
//                     pod: the node's 32 reason bits instead of a record.
//   k_diag_replay     (diag_replay.hpp, here with the reason kind) the unplaced
//                     pods of the last place call at their decision states.
#include <hip/hip_runtime.h>

#include "diag_replay.hpp"
#include "reasons.h"

namespace kh {

constexpr int RS_UNRES = (int)(offsetof(koordhip_reasons, unresolvable) / sizeof(int32_t));
constexpr int RS_FIRST = (int)(offsetof(koordhip_reasons, first) / sizeof(int32_t));
constexpr int RS_ANY = (int)(offsetof(koordhip_reasons, any) / sizeof(int32_t));
static_assert(sizeof(koordhip_reasons) == 264 && kReasonWords == 2 + 2 * KOORDHIP_REASON_SLOTS, "record layout");
static_assert(offsetof(koordhip_reasons, feasible) == 0, "record layout");
static_assert((KOORDHIP_REASONS_OF_STATIC | KOORDHIP_REASONS_OF_FIT | KOORDHIP_REASONS_OF_LA | KOORDHIP_REASONS_OF_NUMA |
               KOORDHIP_REASONS_OF_RESV) == (1u << KOORDHIP_REASON_COUNT) - 1u,
              "every reason belongs to one plugin");

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

// One wave's 64 nodes into a pod's LDS record.  Called by every lane of the
// wave (the ballots are wave-wide); lanes that are not `live` count nowhere.
__device__ __forceinline__ void reasons_count(uint32_t m, bool live, uint32_t slots, int32_t *rec) {
  const uint32_t f = first_reasons(m);
  const bool l0 = __lane_id() == 0;
  const uint64_t ok = __ballot(live && m == 0u);
  const uint64_t uu = __ballot(live && (f & KOORDHIP_REASON_UNRESOLVABLE_MASK) != 0u);
  if (l0 && ok) atomicAdd(&rec[0], (int32_t)__popcll(ok));
  if (l0 && uu) atomicAdd(&rec[RS_UNRES], (int32_t)__popcll(uu));
#pragma unroll
  for (int b = 0; b < KOORDHIP_REASON_COUNT; b++) {
    if (!((slots >> b) & 1u)) continue;
    const uint64_t ma = __ballot(live && ((m >> b) & 1u) != 0u);
    if (!ma) continue;  // wave-uniform: no lane has the reason, so none has it first
    const uint64_t mf = __ballot(live && ((f >> b) & 1u) != 0u);
    if (l0) atomicAdd(&rec[RS_ANY + b], (int32_t)__popcll(ma));
    if (l0 && mf) atomicAdd(&rec[RS_FIRST + b], (int32_t)__popcll(mf));
  }
}

// ---------------------------------------------------------------------------
// k_reasons: S = the reservation slots of the side row (1: no reservation columns)

template <int S>
__global__ __launch_bounds__(DIAG_THREADS) void k_reasons(DevCfg c, DevNodes d, const DevPod *__restrict__ pods,
                                                          int32_t n_pods, int32_t *__restrict__ out,
                                                          uint32_t *__restrict__ mask) {
  __shared__ __attribute__((aligned(16))) uint64_t spw[DIAG_PT * DIAG_POD_WORDS];
  __shared__ int32_t tab[DIAG_PT * kReasonWords];
  const int t = threadIdx.x;
  const int32_t p0 = (int32_t)blockIdx.y * DIAG_PT;
  const int32_t np = min(DIAG_PT, n_pods - p0);
  const uint64_t *src = reinterpret_cast<const uint64_t *>(pods + p0);
  for (int32_t w = t; w < np * DIAG_POD_WORDS; w += DIAG_THREADS) spw[w] = src[w];
  for (int32_t w = t; w < np * kReasonWords; w += DIAG_THREADS) tab[w] = 0;
  __syncthreads();
  const DevPod *sp = reinterpret_cast<const DevPod *>(spw);
  const int32_t i = (int32_t)blockIdx.x * DIAG_THREADS + t;
  const bool live = i < d.n;
  const int32_t il = live ? i : d.n - 1;  // tail lanes read the last row and count nowhere
  NV v{};
  const Need all = need_all(c);
  load_node(v, d, il, all, c);
  NumaRowRS<S> nr{};
  load_numa<true>(nr, d, il, all);
  if constexpr (S > 1) {
    if (c.resv) {
      load_resv(nr, d.rv, il);
      // a topology-policy node's zone row shares the reserved CPUs' bytes (the Filter reads the zones only)
      if (c.zones && topo_policy(nr.nflags) != 0) load_zones(nr, d, il);
    }
  }
  const uint32_t slots = reason_slots(c);
  for (int32_t q = 0; q < np; q++) {
    const DevPod pod = sp[q];
    NV w = v;
    int nmatch = 0;
    uint32_t mm = 0;
    if constexpr (S > 1) {
      if (c.resv) nmatch = resv_restore(w, nr, pod, mm);  // the cycle's restore: every plugin sees the restored node
    }
    const uint32_t m = filter_reasons(c, pod, w, nr, d.nu.cls, nmatch, mm);
    if (mask) {
      if (live) mask[i] = m;
    } else {
      reasons_count(m, live, slots, tab + q * kReasonWords);
    }
  }
  __syncthreads();
  if (!mask) diag_flush<kReasonWords>(tab, np, out + (size_t)p0 * kReasonWords);
}

// the replay's kind (diag_replay.hpp): the reason bits into a koordhip_reasons, or one pod's masks
struct DiagReasons {
  static constexpr int WORDS = kReasonWords;
  using Plane = uint32_t;
  static __device__ __forceinline__ uint32_t slots(const DevCfg &c) { return reason_slots(c); }
  static __device__ __forceinline__ uint32_t eval(const DevCfg &c, const DevPod &pod, const NV &v, const NumaRowR &nr,
                                                  const DevNumaClass *classes) {
    return filter_reasons(c, pod, v, nr, classes, 0, 0u);
  }
  static __device__ __forceinline__ void count(uint32_t m, bool live, uint32_t slots, int32_t *rec) {
    reasons_count(m, live, slots, rec);
  }
};

// ---------------------------------------------------------------------------
// host-side launch wrappers

hipError_t launch_reasons(const DevCfg &c, const DevNodes &d, const DevPod *pods, int32_t n_pods, int32_t *out,
                          uint32_t *mask, hipStream_t s) {
  if (n_pods <= 0 || d.n <= 0) return hipSuccess;
  if ((mask && n_pods != 1) || (!mask && !out)) return hipErrorInvalidValue;
  const dim3 grid((d.n + DIAG_THREADS - 1) / DIAG_THREADS, (n_pods + DIAG_PT - 1) / DIAG_PT);
  if (grid.y > 65535u) return hipErrorInvalidValue;
  if (c.resv)
    hipLaunchKernelGGL(k_reasons<KOORDHIP_RESV_SLOTS_MAX>, grid, dim3(DIAG_THREADS), 0, s, c, d, pods, n_pods, out, mask);
  else
    hipLaunchKernelGGL(k_reasons<1>, grid, dim3(DIAG_THREADS), 0, s, c, d, pods, n_pods, out, mask);
  return hipGetLastError();
}

hipError_t launch_reasons_replay(const DevCfg &c, const DevNodes &d, const DevPod *pods, const uint64_t *cpus,
                                 const DiagLists &l, int32_t U, int32_t single, int32_t *out, uint32_t *mask,
                                 hipStream_t s) {
  return launch_replay<DiagReasons>(c, d, pods, cpus, l, U, single, out, mask, s);
}

}  // namespace kh
