// reasons.hip -- why a pod is unschedulable, one step past diag.hip: per
// Status reason (KOORDHIP_REASON_*) the node counts FitError.Error() prints,
// and how many of the failing nodes are UnschedulableAndUnresolvable
// (koordhip_reasons), reduced on device.
//
//   DiagReasons       the reason kind of diag_kind.hpp's two kernels: the
//                     32 reason bits of filter_reasons into records of 66
//                     words, with the unresolvable counter (the counting and
//                     the slots a profile can produce are diag_kind.hpp's,
//                     shared with diag_ext.hip).
//                     k_diag_current with it answers for pods against the
//                     current state, k_diag_replay for the unplaced pods of
//                     the last place call at their decision states.
#include <hip/hip_runtime.h>

#include "diag_kind.hpp"
#include "reasons.h"

namespace kh {

static_assert(sizeof(koordhip_reasons) == 264 && kReasonWords == 2 + 2 * KOORDHIP_REASON_SLOTS, "record layout");
static_assert(offsetof(koordhip_reasons, feasible) == 0, "record layout");
static_assert((KOORDHIP_REASONS_OF_STATIC | KOORDHIP_REASONS_OF_FIT | KOORDHIP_REASONS_OF_LA | KOORDHIP_REASONS_OF_NUMA |
               KOORDHIP_REASONS_OF_RESV) == (1u << KOORDHIP_REASON_COUNT) - 1u,
              "every reason belongs to one plugin");

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
    reasons_count<KOORDHIP_REASON_COUNT>(m, first_reasons(m), KOORDHIP_REASON_UNRESOLVABLE_MASK, live, slots, rec);
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
