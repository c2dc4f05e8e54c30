// reasons.hip -- why a pod is unschedulable, one step past diag.hip: per
// Status reason (KOORDHIP_REASON_*) the node counts FitError.Error() prints,
// and how many of the failing nodes are UnschedulableAndUnresolvable
// (koordhip_reasons), reduced on device.
//
//   DiagReasons       the reason kind of diag_kind.hpp's two kernels: the
//                     32 reason bits of filter_reasons into records of 66
//                     words, with the unresolvable counter.  The ballots of
//                     slots the profile cannot produce, and the first-ballot of
//                     a reason no lane of the wave has, are skipped.
//                     k_diag_current with it answers for pods against the
//                     current state, k_diag_replay for the unplaced pods of
//                     the last place call at their decision states.
#include <hip/hip_runtime.h>

#include "diag_kind.hpp"
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

// the kind (diag_kind.hpp): the reason bits into a koordhip_reasons, or one pod's masks
struct DiagReasons {
  static constexpr int WORDS = kReasonWords;
  using Plane = uint32_t;
  static __device__ __forceinline__ uint32_t slots(const DevCfg &c) { return reason_slots(c); }
  template <int S>
  static __device__ __forceinline__ uint32_t eval(const DevCfg &c, const DevPod &pod, const NV &v,
                                                  const NumaRowRS<S> &nr, const DevNumaClass *classes, int nmatch,
                                                  uint32_t mm) {
    return filter_reasons(c, pod, v, nr, classes, nmatch, mm);
  }
  static __device__ __forceinline__ void count(uint32_t m, bool live, uint32_t slots, int32_t *rec) {
    reasons_count(m, live, slots, rec);
  }
};

// ---------------------------------------------------------------------------
// host-side launch wrappers

hipError_t launch_reasons(const DevCfg &c, const DevNodes &d, const DevPod *pods, int32_t n_pods, int32_t *out,
                          uint32_t *mask, hipStream_t s) {
  return launch_current<DiagReasons>(c, d, pods, n_pods, out, mask, s);
}

hipError_t launch_reasons_replay(const DevCfg &c, const DevNodes &d, const DevPod *pods, const uint64_t *cpus,
                                 const DiagLists &l, int32_t U, int32_t single, int32_t *out, uint32_t *mask,
                                 hipStream_t s) {
  return launch_replay<DiagReasons>(c, d, pods, cpus, l, U, single, out, mask, s);
}

}  // namespace kh
