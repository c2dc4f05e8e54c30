// diag_ext.h -- launch wrapper of diag_ext.hip (host side): the
// unschedulable-pod diagnosis for the profiles and snapshots of the
// sequential cycle (koordhip_diagnose_ext / koordhip_node_status_ext).
#pragma once
#include <hip/hip_runtime.h>

#include "dev.hpp"
#include "ipa.hpp"
#include "pts.hpp"

namespace kh {

constexpr int DIAGX_PT = 32;  // pods per workgroup (abi.DIAG_EXT_POD_TILE)

// The pod-independent part of PtsLds PodTopologySpread's Filter reads, summed
// over every node once per call (k_diag_pts_sums) instead of once per workgroup.
struct PtsSums {
  int32_t fsum[PC][PD];
  uint32_t fpres[PS][PK][2];
};

// the call's device workspace: the PtsSums, then one hostname minimum per pod
constexpr size_t diag_ext_ws_bytes(int32_t n_pods) {
  return sizeof(PtsSums) + (size_t)(n_pods > 0 ? n_pods : 0) * sizeof(int32_t);
}

// The pre-passes (InterPodAffinity's sums into ipa.sums, PodTopologySpread's
// into ws, the hostname minima of the pods with a hard hostname constraint when
// `hhost` says some pod has one), then k_diag_ext: out[p] += the record of
// (pods[p], podx[p]) on the current state (out zeroed by the caller), or, with
// `status` and n_pods == 1, that pod's [n] status words instead.  podx NULL:
// no pod carries an ext record.  rs: the Reservation plugin scores.
hipError_t launch_diag_ext(const DevCfg &c, const DevNodes &d, const DevPod *pods, const DevPodX *podx, int32_t n_pods,
                           int32_t rs, const PtsArgs &pts, const IpaArgs &ipa, void *ws, bool hhost, int32_t *out,
                           uint16_t *status, hipStream_t s);

// The same pre-passes and kernel with the reason kind: out[p] += pod p's
// koordhip_reasons record (kReasonWords words, slots 19-31 filled), or, with
// `mask` and n_pods == 1, that pod's [n] KOORDHIP_REASON_* masks.
hipError_t launch_reasons_ext(const DevCfg &c, const DevNodes &d, const DevPod *pods, const DevPodX *podx, int32_t n_pods,
                              int32_t rs, const PtsArgs &pts, const IpaArgs &ipa, void *ws, bool hhost, int32_t *out,
                              uint32_t *mask, hipStream_t s);

}  // namespace kh
