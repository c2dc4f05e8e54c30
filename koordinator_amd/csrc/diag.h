// diag.h -- launch wrappers of diag.hip (host side): the unschedulable-pod
// diagnosis, per-plugin node counts reduced on device (koordhip_diag).
#pragma once
#include <hip/hip_runtime.h>

#include "eval.hpp"

namespace kh {

constexpr int kDiagWords = (int)(sizeof(koordhip_diag) / sizeof(int32_t));  // a record as int32 counters

// k_diag_current with the status kind: out[p] += the record of pods[p] on the
// current state (out zeroed by the caller).  With `status` (n_pods == 1): node
// i's status byte instead.
hipError_t launch_diag(const DevCfg &c, const DevNodes &d, const DevPod *pods, int32_t n_pods, int32_t *out,
                       uint8_t *status, hipStream_t s);

// The replay's lists, built on device from a place call's out_node [P] in one
// int32 workspace of diag_ws_ints(n, P) words:
//   off [n + 1]  node i's committed pods are nl[off[i] .. off[i + 1]), ascending pod index
//   nl  [P]      (off[n] entries used)
//   ul  [P]      the unplaced pods (out_node < 0), ascending; tot[1] of them
struct DiagLists {
  int32_t *cnt, *off, *uf, *upos, *nl, *ul, *tot;
};
size_t diag_ws_ints(int32_t n, int32_t P);
DiagLists diag_lists(int32_t *ws, int32_t n, int32_t P);
hipError_t launch_diag_lists(int32_t *ws, const int32_t *out_node, int32_t P, int32_t n, hipStream_t s);

// k_diag_scan on its own (preempt.hip's list build): out[j] = in[0] + .. + in[j - 1] for j < m, *total = the sum
hipError_t launch_scan(const int32_t *in, int32_t *out, int32_t m, int32_t *total, hipStream_t s);

// k_diag_replay: the records of the unplaced pods ul[0, U) at their decision
// states, out [U][kDiagWords] (zeroed by the caller).  single >= 0: that one
// unplaced pod instead (U = 1), and with `status` its [n] status bytes rather
// than a record.  cpus: the place call's cpusets [P][NW] (NULL without NodeNUMAResource).
hipError_t launch_diag_replay(const DevCfg &c, const DevNodes &d, const DevPod *pods, const uint64_t *cpus,
                              const DiagLists &l, int32_t U, int32_t single, int32_t *out, uint8_t *status,
                              hipStream_t s);

}  // namespace kh
