// diag_ext.hip -- why a pod is unschedulable under the profiles and snapshots
// of the sequential cycle (DeviceShare, the extended scalars, PodTopologySpread,
// InterPodAffinity, the 8-slot / device-holding Reservation rows): koordhip_diag
// records over the nine status bits, reduced on device like diag.hip's -- no
// [pods][n] plane exists anywhere.
//
//   k_diag_pts_sums   once per call: the pod-independent counters
//                     PodTopologySpread's Filter reads (PtsSums: what pts_init
//                     rebuilds per workgroup by sweeping every node), summed
//                     over the grid; resets the pods' hostname minima.
//   k_diag_hmin       once per call, when a pod has a hard hostname constraint:
//                     hmin[p] = the minimum of pts_host_match over the eligible
//                     nodes (k_pts_eval's, as a grid reduction).
//   (k_ipa_sums)      InterPodAffinity's domain sums, seq.hip's kernel.
//   k_diag_ext<SM>    256-node tiles x pod tiles, SM as in seq_mode.  A thread
//                     owns one node: it loads the row filter_status reads once
//                     and loops over the tile's pods, whose DevPod / DevPodX
//                     records are staged in LDS.  Per pod the workgroup derives
//                     the hard keys' pair counters and minima from the sums
//                     (pts_prep: 256 threads and a barrier); the status is
//                     filter_status on the restored row | seq_eval's bits |
//                     pts_filter | ipa_filter, each the one definition the
//                     cycle and koordhip_eval_ext use.  The tile staging, the
//                     row load, the counting (one ballot + popcount per wave
//                     and counter into an LDS table of whole records) and the
//                     flush are diag_kind.hpp's, shared with k_diag_current;
//                     the kernel itself is not that template: it has its own
//                     LDS, barriers inside the pod loop and another restore.
//                     With a status pointer (one pod) the node's 16-bit status
//                     is stored instead.
//   k_diag_ext<SM, ExtReasons>
//                     the same kernel counting FitError reasons
//                     (koordhip_reasons, all 32 slots): filter_reasons on the
//                     same restored row | the failing extended scalars
//                     (xfit_reasons / seq_xfit_reasons) | seq_eval's DEVICE bit
//                     | pts_reason | ipa_reason, counted by reasons_count with
//                     `first` in the Filter order above (first_reasons_ext);
//                     with a plane pointer the node's 32-bit reason mask.
//
// None of this is cached across calls: every Reserve advances pts_cnt / ipa_cnt.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "diag.h"
#include "diag_ext.h"
#include "diag_kind.hpp"
#include "reasons.h"
#include "seq.h"
#include "seq_eval.hpp"

namespace kh {

constexpr int DIAGX_PODX_WORDS = tile_words<DevPodX>();
static_assert(DIAGX_PT == DIAG_PT, "one pod tile for every diagnosis kernel");
static_assert(offsetof(DevPodX, req) == 0 && DT >= 1 && DR == 3, "the empty record: req[0][0..2] = -1 are words 0..2");
static_assert(PK * 64 <= DIAG_THREADS, "pts_prep: one wave per topology key");

// ---------------------------------------------------------------------------
// the pre-passes

// sums zeroed by the caller; one workgroup-local table per block, then one
// global atomic per nonzero cell (the arithmetic of pts_init's fsum / fpres)
__global__ __launch_bounds__(DIAG_THREADS) void k_diag_pts_sums(PtsArgs pa, int32_t n, PtsSums *__restrict__ sums,
                                                                 int32_t *__restrict__ hmin, int32_t n_pods) {
  __shared__ PtsSums s;
  constexpr int NF = PC * PD, NP = PS * PK * 2;
  int32_t *sf = &s.fsum[0][0];
  uint32_t *sp = &s.fpres[0][0][0];
  const int t = threadIdx.x;
  const int32_t gid = (int32_t)(blockIdx.x * blockDim.x) + t, gsz = (int32_t)(gridDim.x * blockDim.x);
  for (int32_t p = gid; p < n_pods; p += gsz) hmin[p] = INT32_MAX;
  for (int x = t; x < NF; x += DIAG_THREADS) sf[x] = 0;
  for (int x = t; x < NP; x += DIAG_THREADS) sp[x] = 0u;
  __syncthreads();
  for (int32_t i = gid; i < n; i += gsz) {
    const uint32_t el = pa.elig[i];
    for (int k = 0; k < pa.keys; k++) {
      if ((pa.host >> k) & 1u) continue;
      const int32_t d = pa.dom[(size_t)k * n + i];
      if (d < 0 || d >= PD) continue;
      for (int c = 0; c < pa.classes; c++)
        if ((el >> (2 * c)) & 1u) atomicOr(&s.fpres[c][k][d >> 5], 1u << (d & 31));
    }
    for (int c = 0; c < pa.cons; c++) {
      const int k = pa.cons_key[c];
      if ((pa.host >> k) & 1u) continue;
      const int32_t d = pa.dom[(size_t)k * n + i];
      const int32_t v = pa.cnt[(size_t)c * n + i];
      if (d < 0 || d >= PD || v == 0) continue;
      atomicAdd(&s.fsum[c][d], v);
    }
  }
  __syncthreads();
  for (int x = t; x < NF; x += DIAG_THREADS)
    if (sf[x]) atomicAdd(&sums->fsum[0][0] + x, sf[x]);
  for (int x = t; x < NP; x += DIAG_THREADS)
    if (sp[x]) atomicOr(&sums->fpres[0][0][0] + x, sp[x]);
}

// workgroup (p, y): pod p over the nodes y 256, (y + gridDim.y) 256, ...
__global__ __launch_bounds__(DIAG_THREADS) void k_diag_hmin(PtsArgs pa, int32_t n, const DevPodX *__restrict__ podx,
                                                             int32_t *__restrict__ hmin) {
  const int32_t p = (int32_t)blockIdx.x;
  const PtsPod q = pts_pod(pa, podx[p]);
  if (!q.hhost) return;
  int32_t m = INT32_MAX;
  for (int32_t i = (int32_t)blockIdx.y * DIAG_THREADS + (int32_t)threadIdx.x; i < n;
       i += (int32_t)gridDim.y * DIAG_THREADS)
    for (int k = 0; k < PK; k++)
      if (((q.hkeys & pa.host) >> k) & 1u) {
        const int32_t v = pts_host_match(pa, q, k, n, i);
        if (v >= 0) m = min(m, v);
      }
  m = pts_wave_min(m);
  if (__lane_id() == 0 && m != INT32_MAX) atomicMin(&hmin[p], m);
}

// ---------------------------------------------------------------------------
// k_diag_ext

// What k_diag_ext evaluates and counts per (pod, node): the KOORDHIP_ST_* status
// into koordhip_diag records / 16-bit words, or the KOORDHIP_REASON_* mask into
// koordhip_reasons records / 32-bit words.
struct ExtStatus {
  static constexpr bool REASONS = false;
  static constexpr int WORDS = kDiagWords;
  using Plane = uint16_t;
};
struct ExtReasons {
  static constexpr bool REASONS = true;
  static constexpr int WORDS = kReasonWords;
  using Plane = uint32_t;
};
static_assert(KOORDHIP_REASON_FIT_X0 + KOORDHIP_NXRES == KOORDHIP_REASON_DEVICE_INSUFFICIENT &&
                  KOORDHIP_REASONS_OF_XFIT == ((1u << KOORDHIP_NXRES) - 1u) << KOORDHIP_REASON_FIT_X0,
              "one FIT_X slot per extended scalar");
static_assert((KOORDHIP_REASONS_OF_XFIT | KOORDHIP_REASONS_OF_DEVICE | KOORDHIP_REASONS_OF_PTS | KOORDHIP_REASONS_OF_IPA) ==
                      ~((1u << KOORDHIP_REASON_COUNT) - 1u) &&
                  KOORDHIP_REASON_EXT_COUNT == KOORDHIP_REASON_SLOTS,
              "slots 19-31 belong to the sequential cycle's plugins");
static_assert(KOORDHIP_REASON_EXT_UNRESOLVABLE_MASK ==
                  (KOORDHIP_REASON_UNRESOLVABLE_MASK | reason_bit(KOORDHIP_REASON_PTS_MISSING_LABEL) |
                   reason_bit(KOORDHIP_REASON_IPA_AFFINITY)),
              "the UnschedulableAndUnresolvable reasons");

template <int SM, class K>
__global__ __launch_bounds__(DIAG_THREADS) void k_diag_ext(DevCfg c, DevNodes d, const DevPod *__restrict__ pods,
                                                            const DevPodX *__restrict__ podx, int32_t n_pods,
                                                            int32_t rs, PtsArgs pa, IpaArgs ia,
                                                            const PtsSums *__restrict__ psum,
                                                            const int32_t *__restrict__ hmin, int32_t *__restrict__ out,
                                                            typename K::Plane *__restrict__ status) {
  constexpr int S = SM >= 2 ? kSeqSlots<SM> : 1;  // the reservation slots of filter_status' side row
  __shared__ __attribute__((aligned(16))) uint64_t spw[DIAG_PT * tile_words<DevPod>()];
  __shared__ __attribute__((aligned(16))) uint64_t sxw[DIAG_PT * DIAGX_PODX_WORDS];
  __shared__ int32_t tab[DIAG_PT * K::WORDS];
  __shared__ PtsLds L;   // fsum / fpres from the call's sums; fmatch / fmin per pod (ssum: Score only, never read)
  __shared__ IpaLds IL;
  const int t = threadIdx.x;
  const int32_t p0 = (int32_t)blockIdx.y * DIAG_PT;
  const int32_t np = min(DIAG_PT, n_pods - p0);
  stage_tile(spw, pods + p0, np);
  if (podx) {
    stage_tile(sxw, podx + p0, np);
  } else {  // the record of a pod without koordhip_pod_ext (no device request: gpu -1 = key absent)
    for (int32_t w = t; w < np * DIAGX_PODX_WORDS; w += DIAG_THREADS) sxw[w] = (w % DIAGX_PODX_WORDS) < DR ? ~0ull : 0ull;
  }
  for (int32_t w = t; w < np * K::WORDS; w += DIAG_THREADS) tab[w] = 0;
  const bool pts_on = pa.filt && pa.keys > 0;
  const bool ipa_on = ia.filt && ia.ents > 0;
  if (pts_on) {
    for (int x = t; x < PC * PD; x += DIAG_THREADS) (&L.fsum[0][0])[x] = (&psum->fsum[0][0])[x];
    for (int x = t; x < PS * PK * 2; x += DIAG_THREADS) (&L.fpres[0][0][0])[x] = (&psum->fpres[0][0][0])[x];
  }
  if (ipa_on) ipa_load(ia, IL, t, DIAG_THREADS);
  __syncthreads();
  const DevPod *sp = reinterpret_cast<const DevPod *>(spw);
  const DevPodX *sx = reinterpret_cast<const DevPodX *>(sxw);
  const int32_t i = (int32_t)blockIdx.x * DIAG_THREADS + t;
  const bool live = i < d.n;
  const int32_t il = live ? i : d.n - 1;  // tail lanes read the last row and count nowhere
  NV v{};
  NumaRowRS<S> nr{};
  load_filter_row(c, d, il, v, nr);
  // the status counters: every one, whatever the profile; the reason slots: those the profile can produce
  const uint32_t bits = K::REASONS ? reason_slots_ext(c, pts_on, ipa_on) : (1u << DIAG_STATUS_BITS) - 1u;
  for (int32_t q = 0; q < np; q++) {  // wave-uniform: the ballots and the barriers are valid
    const DevPod &pod = sp[q];
    const DevPodX &x = sx[q];
    NV w = v;
    int nmatch = 0;
    uint32_t mm = 0;
    ResvXS rx = no_rx();
    uint32_t xm = 0u;  // (reasons) the failing extended scalars, as seq_eval's XFIT bit sees them
    if constexpr (K::REASONS) xm = xfit_reasons(d.dv, x, il, d.n);
    if constexpr (S > 1) {
      if (c.resv) {
        // the cycle's restore: every plugin sees the restored node, with the extended
        // scalars of a reservation holding devices (what eval_total_resv restores and filters with)
        rx = seq_resv_x(d, pod, x, nr, il);
        nmatch = resv_restore(w, nr, pod, mm, rx);
        // filterWithReservations' fitsNode covers the pod's extended scalars on every node.  Where no
        // reservation holds devices they are the node's own: a node failing xfit_filter fails the fit of
        // every matched Aligned / Restricted reservation -- a ResvXS naming no slot (h = S) without RX_FIT_O.
        if constexpr (K::REASONS) {
          if (rx.h >= 0) xm = seq_xfit_reasons(d, pod, x, nr, il);  // on the restored scalars
          else if (xm) rx = ResvXS{S, RX_FIT_H | RX_LE | RX_XFIT, 0, 0};
        } else {
          if (rx.h < 0 && !xfit_filter(d.dv, x, il, d.n)) rx = ResvXS{S, RX_FIT_H | RX_LE | RX_XFIT, 0, 0};
        }
      }
    }
    // the base plugins on the same restored row and ResvXS, as status bits or as reasons
    uint32_t st;
    if constexpr (K::REASONS)
      st = filter_reasons(c, pod, w, nr, d.nu.cls, nmatch, mm, rx);
    else
      st = filter_status(c, pod, w, nr, d.nu.cls, nmatch, mm, rx);
    int32_t raw[KOORDHIP_NEXT_PLUGINS];
    uint8_t sq = 0;
    (void)seq_eval<SM>(c, d, pod, x, il, rs != 0, raw, &sq);  // XFIT, DEVICE, RESV of a reserve pod
    if constexpr (K::REASONS) {
      // NodeResourcesFit reports every failing scalar; DeviceShare one slot for seq_eval's verdict
      if (c.filt & KOORDHIP_PLUGIN_FIT) st |= xm << KOORDHIP_REASON_FIT_X0;
      if (sq & KOORDHIP_ST_DEVICE_FAIL) st |= reason_bit(KOORDHIP_REASON_DEVICE_INSUFFICIENT);
    } else {
      st |= sq;
    }
    // PodTopologySpread's Filter half only: pts_prep then never reads the Score's ssum
    PtsPod pq = pts_pod(pa, x);
    pq.soft = pq.skeys = 0u;
    pq.ns = 0;
    const bool spread = pts_on && pq.nh > 0;
    if (spread) {
      pts_prep(pa, pq, L, t);  // (ends with a barrier)
      const int32_t hm = pq.hhost ? hmin[p0 + q] : INT32_MAX;
      if constexpr (K::REASONS) {
        const int why = pts_reason(pa, pq, L, hm, d.n, il);
        if (why) st |= reason_bit(why == 1 ? KOORDHIP_REASON_PTS_MISSING_LABEL : KOORDHIP_REASON_PTS_SKEW);
      } else {
        if (!pts_filter(pa, pq, L, hm, d.n, il)) st |= KOORDHIP_ST_PTS_FAIL;
      }
    }
    if (ipa_on && (x.ipa_aff | x.ipa_anti) != 0u) {
      if constexpr (K::REASONS) {
        const int why = ipa_reason(ia, IL, x, d.n, il);
        if (why) st |= reason_bit(why == 1 ? KOORDHIP_REASON_IPA_AFFINITY : KOORDHIP_REASON_IPA_ANTI);
      } else {
        if (!ipa_filter(ia, IL, x, d.n, il)) st |= KOORDHIP_ST_IPA_FAIL;
      }
    }
    if (status) {
      if (live) status[i] = (typename K::Plane)st;
    } else if constexpr (K::REASONS) {
      reasons_count<KOORDHIP_REASON_EXT_COUNT>(st, first_reasons_ext(st), KOORDHIP_REASON_EXT_UNRESOLVABLE_MASK, live, bits,
                                               tab + q * K::WORDS);
    } else {
      status_count<DIAG_STATUS_BITS>(st, first_fail(st), live, bits, tab + q * K::WORDS);
    }
    if (spread) __syncthreads();  // the next pod's pts_prep overwrites fmatch / fmin
  }
  __syncthreads();
  if (!status) diag_flush<K::WORDS>(tab, np, out + (size_t)p0 * K::WORDS);
}

// ---------------------------------------------------------------------------
// host-side launch wrapper

template <class K>
static hipError_t launch_ext(const DevCfg &c, const DevNodes &d, const DevPod *pods, const DevPodX *podx, int32_t n_pods,
                             int32_t rs, const PtsArgs &pts, const IpaArgs &ipa, void *ws, bool hhost, int32_t *out,
                             typename K::Plane *plane, hipStream_t s) {
  if (n_pods <= 0 || d.n <= 0) return hipSuccess;
  if ((plane && n_pods != 1) || (!plane && !out) || !ws) return hipErrorInvalidValue;
  const dim3 grid((d.n + DIAG_THREADS - 1) / DIAG_THREADS, (n_pods + DIAG_PT - 1) / DIAG_PT);
  if (grid.y > 65535u) return hipErrorInvalidValue;
  PtsSums *psum = static_cast<PtsSums *>(ws);
  int32_t *hmin = reinterpret_cast<int32_t *>(psum + 1);
  const int32_t nblk = std::min<int32_t>(1024, (d.n + DIAG_THREADS - 1) / DIAG_THREADS);
  if (ipa.filt)
    if (hipError_t e = launch_ipa_sums(ipa, d.n, s)) return e;
  if (pts.filt && pts.keys > 0) {
    if (hipError_t e = hipMemsetAsync(psum, 0, sizeof(PtsSums), s)) return e;
    hipLaunchKernelGGL(k_diag_pts_sums, dim3(nblk), dim3(DIAG_THREADS), 0, s, pts, d.n, psum, hmin, n_pods);
    if (hhost && podx)
      hipLaunchKernelGGL(k_diag_hmin, dim3(n_pods, std::min<int32_t>(64, nblk)), dim3(DIAG_THREADS), 0, s, pts, d.n, podx,
                         hmin);
  }
  switch (seq_mode(c)) {
    case 3:
      hipLaunchKernelGGL((k_diag_ext<3, K>), grid, dim3(DIAG_THREADS), 0, s, c, d, pods, podx, n_pods, rs, pts, ipa, psum,
                         hmin, out, plane);
      break;
    case 2:
      hipLaunchKernelGGL((k_diag_ext<2, K>), grid, dim3(DIAG_THREADS), 0, s, c, d, pods, podx, n_pods, rs, pts, ipa, psum,
                         hmin, out, plane);
      break;
    case 1:
      hipLaunchKernelGGL((k_diag_ext<1, K>), grid, dim3(DIAG_THREADS), 0, s, c, d, pods, podx, n_pods, rs, pts, ipa, psum,
                         hmin, out, plane);
      break;
    default:
      hipLaunchKernelGGL((k_diag_ext<0, K>), grid, dim3(DIAG_THREADS), 0, s, c, d, pods, podx, n_pods, rs, pts, ipa, psum,
                         hmin, out, plane);
  }
  return hipGetLastError();
}

hipError_t launch_diag_ext(const DevCfg &c, const DevNodes &d, const DevPod *pods, const DevPodX *podx, int32_t n_pods,
                           int32_t rs, const PtsArgs &pts, const IpaArgs &ipa, void *ws, bool hhost, int32_t *out,
                           uint16_t *status, hipStream_t s) {
  return launch_ext<ExtStatus>(c, d, pods, podx, n_pods, rs, pts, ipa, ws, hhost, out, status, s);
}

hipError_t launch_reasons_ext(const DevCfg &c, const DevNodes &d, const DevPod *pods, const DevPodX *podx, int32_t n_pods,
                              int32_t rs, const PtsArgs &pts, const IpaArgs &ipa, void *ws, bool hhost, int32_t *out,
                              uint32_t *mask, hipStream_t s) {
  return launch_ext<ExtReasons>(c, d, pods, podx, n_pods, rs, pts, ipa, ws, hhost, out, mask, s);
}

}  // namespace kh
