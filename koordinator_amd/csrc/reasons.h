// reasons.h -- launch wrappers of reasons.hip (host side): the FitError reasons
// of a pod's nodes, counted on device (koordhip_reasons).
#pragma once
#include <hip/hip_runtime.h>

#include "diag.h"
#include "eval.hpp"

namespace kh {

constexpr int kReasonWords = (int)(sizeof(koordhip_reasons) / sizeof(int32_t));  // a record as int32 counters

// k_diag_current with the reason kind: launch_diag's arguments, records of
// kReasonWords words, and with `mask` (n_pods == 1) node i's reason bits.
hipError_t launch_reasons(const DevCfg &c, const DevNodes &d, const DevPod *pods, int32_t n_pods, int32_t *out,
                          uint32_t *mask, hipStream_t s);

// k_diag_replay with the reason kind: launch_diag_replay's arguments, records
// of kReasonWords words, and with `mask` one pod's [n] reason bits.
hipError_t launch_reasons_replay(const DevCfg &c, const DevNodes &d, const DevPod *pods, const uint64_t *cpus,
                                 const DiagLists &l, int32_t U, int32_t single, int32_t *out, uint32_t *mask,
                                 hipStream_t s);

}  // namespace kh
