// diag_replay.hpp -- what diag.hip and reasons.hip share: the tile shape, the
// LDS-table flush and the decision-state replay kernel, parameterised on what
// it evaluates and counts per (pod, node).
//
// A kind K supplies
//   K::WORDS                       int32 counters of one pod's record
//   K::Plane                       a node's value in the single-pod form
//   K::slots(c)                    the counters the profile can produce (wave-uniform)
//   K::eval(c, pod, v, nr, cls)    the (pod, node) value on a row without reservation columns
//   K::count(x, live, slots, rec)  one wave's 64 values into a pod's LDS record
// diag.hip instantiates it with the KOORDHIP_ST_* status (koordhip_diag),
// reasons.hip with the KOORDHIP_REASON_* mask (koordhip_reasons).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "diag.h"
#include "eval.hpp"

namespace kh {

constexpr int DIAG_THREADS = 256;
constexpr int DIAG_PT = 32;                 // pods per LDS tile
constexpr int DIAG_POD_WORDS = (int)(sizeof(DevPod) / sizeof(uint64_t));
static_assert(sizeof(DevPod) % sizeof(uint64_t) == 0, "pod records are staged as 8-B words");

// the workgroup's LDS records of np pods -> out (np contiguous records of W words)
template <int W>
__device__ __forceinline__ void diag_flush(const int32_t *tab, int32_t np, int32_t *out) {
  for (int32_t w = threadIdx.x; w < np * W; w += DIAG_THREADS) {
    const int32_t x = tab[w];
    if (x) atomicAdd(&out[w], x);
  }
}

// k_diag_replay: workgroup (x, y) takes nodes [256 x, 256 x + 256) and the
// tiles [y tpb, (y + 1) tpb) of the unplaced list, last tile first.  The loop
// over the unplaced pods is wave-uniform (the ballots are valid); only the
// walk over a node's commits diverges.
template <class K>
__global__ __launch_bounds__(DIAG_THREADS) void k_diag_replay(DevCfg c, DevNodes d, const DevPod *__restrict__ pods,
                                                              const uint64_t *__restrict__ cpus,
                                                              const int32_t *__restrict__ off,
                                                              const int32_t *__restrict__ nl,
                                                              const int32_t *__restrict__ ul, int32_t U, int32_t single,
                                                              int32_t tpb, int32_t *__restrict__ out,
                                                              typename K::Plane *__restrict__ plane) {
  __shared__ __attribute__((aligned(16))) uint64_t spw[DIAG_PT * DIAG_POD_WORDS];
  __shared__ int32_t su[DIAG_PT];
  __shared__ int32_t tab[DIAG_PT * K::WORDS];
  const int t = threadIdx.x;
  const int32_t i = (int32_t)blockIdx.x * DIAG_THREADS + t;
  const bool live = i < d.n;
  const int32_t il = live ? i : d.n - 1;
  NV v{};
  const Need all = need_all(c);
  load_node(v, d, il, all, c);
  NumaRowR nr{};
  load_numa<true>(nr, d, il, all);
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
    for (int32_t w = t; w < nk * DIAG_POD_WORDS; w += DIAG_THREADS) {
      const int32_t q = w / DIAG_POD_WORDS;
      spw[w] = reinterpret_cast<const uint64_t *>(pods + su[q])[w - q * DIAG_POD_WORDS];
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
      const uint32_t x = K::eval(c, pod, v, nr, d.nu.cls);
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
