// diag.hip -- why a pod is unschedulable: per-plugin node counts of its Filter
// result (koordhip_diag), reduced on device.
//
//   DiagStatus        the status kind of diag_kind.hpp's two kernels: the
//                     KOORDHIP_ST_* bits of filter_status, counted per bit and
//                     per first failing plugin.  k_diag_current with it answers
//                     for pods against the current state, k_diag_replay for
//                     the unplaced pods of the last place call at their
//                     decision states.
//   k_diag_mark / k_diag_scan / k_diag_fill / k_diag_sort
//                     the replay's lists from the device-resident out_node:
//                     per node its committed pods (count, exclusive scan,
//                     fill, each list sorted by pod index) and the ascending
//                     list of unplaced pods.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "diag.h"
#include "diag_kind.hpp"
#include "eval.hpp"

namespace kh {

constexpr int DIAG_NBITS = 5;               // the status bits these kernels produce: FIT, LA, NUMA, RESV, STATIC
static_assert(offsetof(koordhip_diag, feasible) == 0 && kDiagWords == 2 + 2 * KOORDHIP_DIAG_BITS, "record layout");
static_assert((KOORDHIP_ST_FIT_FAIL | KOORDHIP_ST_LA_FAIL | KOORDHIP_ST_NUMA_FAIL | KOORDHIP_ST_RESV_FAIL |
               KOORDHIP_ST_STATIC_FAIL) == (1u << DIAG_NBITS) - 1u, "the counted status bits are bits 0..4");

// the status bits the profile's Filter plugins can set (wave-uniform)
__device__ __forceinline__ uint32_t status_bits(const DevCfg &c) {
  return ((c.filt & KOORDHIP_PLUGIN_FIT) ? KOORDHIP_ST_FIT_FAIL : 0u) |
         ((c.filt & KOORDHIP_PLUGIN_LOADAWARE) ? KOORDHIP_ST_LA_FAIL : 0u) |
         ((c.filt & KOORDHIP_PLUGIN_NUMA) ? KOORDHIP_ST_NUMA_FAIL : 0u) |
         ((c.filt & KOORDHIP_PLUGIN_RESERVATION) ? KOORDHIP_ST_RESV_FAIL : 0u) |
         ((c.filt & KOORDHIP_PLUGIN_NODE_STATIC) ? KOORDHIP_ST_STATIC_FAIL : 0u);
}

// the kind (diag_kind.hpp): the status bits into a koordhip_diag, or one pod's status bytes
struct DiagStatus {
  static constexpr int WORDS = kDiagWords;
  using Plane = uint8_t;
  static __device__ __forceinline__ uint32_t slots(const DevCfg &c) { return status_bits(c); }
  template <int S>
  static __device__ __forceinline__ uint32_t eval(const DevCfg &c, const DevPod &pod, const NV &v,
                                                  const NumaRowRS<S> &nr, const DevNumaClass *classes, int nmatch,
                                                  uint32_t mm) {
    return filter_status(c, pod, v, nr, classes, nmatch, mm);
  }
  static __device__ __forceinline__ void count(uint32_t st, bool live, uint32_t bits, int32_t *rec) {
    status_count<DIAG_NBITS>(st, first_fail(st), live, bits, rec);
  }
};

// ---------------------------------------------------------------------------
// the replay's lists

__global__ void k_diag_mark(const int32_t *__restrict__ out_node, int32_t P, int32_t n, int32_t *__restrict__ cnt,
                            int32_t *__restrict__ uf) {
  const int32_t p = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (p >= P) return;
  const int32_t node = out_node[p];
  const bool placed = node >= 0 && node < n;
  uf[p] = placed ? 0 : 1;
  if (placed) atomicAdd(&cnt[node], 1);
}

// out[j] = in[0] + .. + in[j - 1] for j < m, *total = the sum; one workgroup,
// 8 elements per thread per step.
constexpr int SCAN_PER = 8;
__global__ __launch_bounds__(DIAG_THREADS) void k_diag_scan(const int32_t *__restrict__ in, int32_t *__restrict__ out,
                                                            int32_t m, int32_t *__restrict__ total) {
  __shared__ int32_t wsum[DIAG_THREADS / 64];
  const int t = threadIdx.x, lane = __lane_id(), w = t >> 6;
  int32_t carry = 0;
  for (int32_t base = 0; base < m; base += DIAG_THREADS * SCAN_PER) {
    const int32_t j0 = base + t * SCAN_PER;
    int32_t x[SCAN_PER], s = 0;
#pragma unroll
    for (int e = 0; e < SCAN_PER; e++) {
      x[e] = j0 + e < m ? in[j0 + e] : 0;
      s += x[e];
    }
    int32_t incl = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int32_t y = __shfl_up(incl, off, 64);
      if (lane >= off) incl += y;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int32_t wbase = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < DIAG_THREADS / 64; q++) {
      if (q < w) wbase += wsum[q];
      tot += wsum[q];
    }
    __syncthreads();
    int32_t run = carry + wbase + incl - s;
#pragma unroll
    for (int e = 0; e < SCAN_PER; e++) {
      if (j0 + e < m) out[j0 + e] = run;
      run += x[e];
    }
    carry += tot;
  }
  if (t == 0) *total = carry;
}

__global__ void k_diag_fill(const int32_t *__restrict__ out_node, int32_t P, int32_t n, const int32_t *__restrict__ off,
                            int32_t *__restrict__ cur, const int32_t *__restrict__ upos, int32_t *__restrict__ nl,
                            int32_t *__restrict__ ul) {
  const int32_t p = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (p >= P) return;
  const int32_t node = out_node[p];
  if (node >= 0 && node < n)
    nl[off[node] + atomicAdd(&cur[node], 1)] = p;
  else
    ul[upos[p]] = p;
}

// each node's list into ascending pod index (the fill's order is arbitrary; lists are short)
__global__ void k_diag_sort(const int32_t *__restrict__ off, int32_t *__restrict__ nl, int32_t n) {
  const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const int32_t lo = off[i], hi = off[i + 1];
  for (int32_t a = lo + 1; a < hi; a++) {
    const int32_t x = nl[a];
    int32_t b = a;
    for (; b > lo && nl[b - 1] > x; b--) nl[b] = nl[b - 1];
    nl[b] = x;
  }
}

// ---------------------------------------------------------------------------
// host-side launch wrappers

hipError_t launch_diag(const DevCfg &c, const DevNodes &d, const DevPod *pods, int32_t n_pods, int32_t *out,
                       uint8_t *status, hipStream_t s) {
  return launch_current<DiagStatus>(c, d, pods, n_pods, out, status, s);
}

hipError_t launch_scan(const int32_t *in, int32_t *out, int32_t m, int32_t *total, hipStream_t s) {
  hipLaunchKernelGGL(k_diag_scan, dim3(1), dim3(DIAG_THREADS), 0, s, in, out, m, total);
  return hipGetLastError();
}

size_t diag_ws_ints(int32_t n, int32_t P) { return 2 * ((size_t)n + 1) + 4 * (size_t)std::max(P, 0) + 2; }

DiagLists diag_lists(int32_t *ws, int32_t n, int32_t P) {
  DiagLists l;
  const size_t p = (size_t)std::max(P, 0);
  l.cnt = ws;
  l.off = l.cnt + n + 1;
  l.uf = l.off + n + 1;
  l.upos = l.uf + p;
  l.nl = l.upos + p;
  l.ul = l.nl + p;
  l.tot = l.ul + p;
  return l;
}

hipError_t launch_diag_lists(int32_t *ws, const int32_t *out_node, int32_t P, int32_t n, hipStream_t s) {
  const DiagLists l = diag_lists(ws, n, P);
  hipError_t e = hipMemsetAsync(l.cnt, 0, ((size_t)n + 1) * sizeof(int32_t), s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(l.tot, 0, 2 * sizeof(int32_t), s);
  if (e != hipSuccess) return e;
  if (P <= 0) return hipMemsetAsync(l.off, 0, ((size_t)n + 1) * sizeof(int32_t), s);
  const dim3 pg((P + 255) / 256), blk(256);
  hipLaunchKernelGGL(k_diag_mark, pg, blk, 0, s, out_node, P, n, l.cnt, l.uf);
  hipLaunchKernelGGL(k_diag_scan, dim3(1), dim3(DIAG_THREADS), 0, s, l.cnt, l.off, n + 1, l.tot);
  hipLaunchKernelGGL(k_diag_scan, dim3(1), dim3(DIAG_THREADS), 0, s, l.uf, l.upos, P, l.tot + 1);
  e = hipMemsetAsync(l.cnt, 0, ((size_t)n + 1) * sizeof(int32_t), s);  // now the fill's cursors
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_diag_fill, pg, blk, 0, s, out_node, P, n, l.off, l.cnt, l.upos, l.nl, l.ul);
  if (n > 0) hipLaunchKernelGGL(k_diag_sort, dim3((n + 255) / 256), blk, 0, s, l.off, l.nl, n);
  return hipGetLastError();
}

hipError_t launch_diag_replay(const DevCfg &c, const DevNodes &d, const DevPod *pods, const uint64_t *cpus,
                              const DiagLists &l, int32_t U, int32_t single, int32_t *out, uint8_t *status,
                              hipStream_t s) {
  return launch_replay<DiagStatus>(c, d, pods, cpus, l, U, single, out, status, s);
}

}  // namespace kh
