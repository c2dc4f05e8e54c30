// diag.hip -- why a pod is unschedulable: per-plugin node counts of its Filter
// result (koordhip_diag), reduced on device.
//
//   k_diag            stateless: pods against the current state.  256-node
//                     tiles x pod tiles; a thread loads its node row once and
//                     loops over the tile's pods (staged in LDS).  Per pod and
//                     counter one ballot + popcount per wave, lane 0 adds into
//                     an LDS table of whole records, the workgroup flushes its
//                     non-zero entries with one atomic per counter (lanes on
//                     consecutive words of a pod's record).
//   k_diag_replay     (the template of diag_replay.hpp, here with the status
//                     kind) the unplaced pods of the last place call at their
//                     decision states, without a copy of the table: a commit
//                     is exactly invertible (apply_delta / numa_apply with
//                     sign -1, integers held in f64, order-independent), so a
//                     thread loads its node's FINAL row, walks the unplaced
//                     pods in descending order and, before it evaluates pod u,
//                     un-applies its node's commits with a pod index > u.
//   k_diag_mark / k_diag_scan / k_diag_fill / k_diag_sort
//                     the replay's lists from the device-resident out_node:
//                     per node its committed pods (count, exclusive scan,
//                     fill, each list sorted by pod index) and the ascending
//                     list of unplaced pods.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "diag.h"
#include "diag_replay.hpp"
#include "eval.hpp"

namespace kh {

constexpr int DIAG_ANY = (int)(offsetof(koordhip_diag, any) / sizeof(int32_t));
constexpr int DIAG_FIRST = (int)(offsetof(koordhip_diag, first) / sizeof(int32_t));
constexpr int DIAG_NBITS = 5;               // the status bits these kernels produce: FIT, LA, NUMA, RESV, STATIC
static_assert(offsetof(koordhip_diag, feasible) == 0 && kDiagWords == 2 + 2 * KOORDHIP_DIAG_BITS, "record layout");
static_assert((KOORDHIP_ST_FIT_FAIL | KOORDHIP_ST_LA_FAIL | KOORDHIP_ST_NUMA_FAIL | KOORDHIP_ST_RESV_FAIL |
               KOORDHIP_ST_STATIC_FAIL) == (1u << DIAG_NBITS) - 1u, "the counted status bits are bits 0..4");

// The first failing plugin in the framework's Filter order STATIC -> FIT -> LA
// -> NUMA -> RESV (koordhip.h): the static bit, else the lowest set bit.
__device__ __forceinline__ uint32_t first_fail(uint32_t st) {
  return (st & KOORDHIP_ST_STATIC_FAIL) ? (uint32_t)KOORDHIP_ST_STATIC_FAIL : (st & (0u - st));
}

// the status bits the profile's Filter plugins can set (wave-uniform)
__device__ __forceinline__ uint32_t status_bits(const DevCfg &c) {
  return ((c.filt & KOORDHIP_PLUGIN_FIT) ? KOORDHIP_ST_FIT_FAIL : 0u) |
         ((c.filt & KOORDHIP_PLUGIN_LOADAWARE) ? KOORDHIP_ST_LA_FAIL : 0u) |
         ((c.filt & KOORDHIP_PLUGIN_NUMA) ? KOORDHIP_ST_NUMA_FAIL : 0u) |
         ((c.filt & KOORDHIP_PLUGIN_RESERVATION) ? KOORDHIP_ST_RESV_FAIL : 0u) |
         ((c.filt & KOORDHIP_PLUGIN_NODE_STATIC) ? KOORDHIP_ST_STATIC_FAIL : 0u);
}

// One wave's 64 nodes into a pod's LDS record.  Called by every lane of the
// wave (the ballots are wave-wide); lanes that are not `live` count nowhere.
__device__ __forceinline__ void diag_count(uint32_t st, bool live, uint32_t bits, int32_t *rec) {
  const uint32_t f = first_fail(st);
  const bool l0 = __lane_id() == 0;
  const uint64_t ok = __ballot(live && st == 0u);
  if (l0 && ok) atomicAdd(&rec[0], (int32_t)__popcll(ok));
#pragma unroll
  for (int b = 0; b < DIAG_NBITS; b++) {
    if (!((bits >> b) & 1u)) continue;
    const uint64_t ma = __ballot(live && ((st >> b) & 1u) != 0u);
    const uint64_t mf = __ballot(live && f == (1u << b));
    if (l0 && ma) atomicAdd(&rec[DIAG_ANY + b], (int32_t)__popcll(ma));
    if (l0 && mf) atomicAdd(&rec[DIAG_FIRST + b], (int32_t)__popcll(mf));
  }
}

// the replay's kind (diag_replay.hpp): the status bits into a koordhip_diag, or one pod's status bytes
struct DiagStatus {
  static constexpr int WORDS = kDiagWords;
  using Plane = uint8_t;
  static __device__ __forceinline__ uint32_t slots(const DevCfg &c) { return status_bits(c); }
  static __device__ __forceinline__ uint32_t eval(const DevCfg &c, const DevPod &pod, const NV &v, const NumaRowR &nr,
                                                  const DevNumaClass *classes) {
    return filter_status(c, pod, v, nr, classes, 0, 0u);
  }
  static __device__ __forceinline__ void count(uint32_t st, bool live, uint32_t bits, int32_t *rec) {
    diag_count(st, live, bits, rec);
  }
};

// ---------------------------------------------------------------------------
// k_diag: S = the reservation slots of the side row (1: no reservation columns)

template <int S>
__global__ __launch_bounds__(DIAG_THREADS) void k_diag(DevCfg c, DevNodes d, const DevPod *__restrict__ pods,
                                                       int32_t n_pods, int32_t *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint64_t spw[DIAG_PT * DIAG_POD_WORDS];
  __shared__ int32_t tab[DIAG_PT * kDiagWords];
  const int t = threadIdx.x;
  const int32_t p0 = (int32_t)blockIdx.y * DIAG_PT;
  const int32_t np = min(DIAG_PT, n_pods - p0);
  const uint64_t *src = reinterpret_cast<const uint64_t *>(pods + p0);
  for (int32_t w = t; w < np * DIAG_POD_WORDS; w += DIAG_THREADS) spw[w] = src[w];
  for (int32_t w = t; w < np * kDiagWords; w += DIAG_THREADS) tab[w] = 0;
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
  const uint32_t bits = status_bits(c);
  for (int32_t q = 0; q < np; q++) {
    const DevPod pod = sp[q];
    NV w = v;
    int nmatch = 0;
    uint32_t mm = 0;
    if constexpr (S > 1) {
      if (c.resv) nmatch = resv_restore(w, nr, pod, mm);  // the cycle's restore: every plugin sees the restored node
    }
    const uint32_t st = filter_status(c, pod, w, nr, d.nu.cls, nmatch, mm);
    diag_count(st, live, bits, tab + q * kDiagWords);
  }
  __syncthreads();
  diag_flush<kDiagWords>(tab, np, out + (size_t)p0 * kDiagWords);
}

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
                       hipStream_t s) {
  if (n_pods <= 0 || d.n <= 0) return hipSuccess;
  const dim3 grid((d.n + DIAG_THREADS - 1) / DIAG_THREADS, (n_pods + DIAG_PT - 1) / DIAG_PT);
  if (grid.y > 65535u) return hipErrorInvalidValue;
  if (c.resv)
    hipLaunchKernelGGL(k_diag<KOORDHIP_RESV_SLOTS_MAX>, grid, dim3(DIAG_THREADS), 0, s, c, d, pods, n_pods, out);
  else
    hipLaunchKernelGGL(k_diag<1>, grid, dim3(DIAG_THREADS), 0, s, c, d, pods, n_pods, out);
  return hipGetLastError();
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
