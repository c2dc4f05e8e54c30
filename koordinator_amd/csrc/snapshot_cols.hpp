// snapshot_cols.hpp -- the node snapshot's column table and the staging image
// of koordhip_update_nodes.  Host only: no HIP header, any C++17 compiler
// (tests/snapshot_pack_check.cpp builds it alone).
//
// A snapshot column is declared once, where load_snapshot allocates it; the
// record kept in the context is what update rows, checkpoint / restore and
// the release walk.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace kh {

// Resource quantities live on device as exact f64 (eval.hpp): 0 <= v < 2^45.
// A negative one (no Allocatable, Requested, usage or pod request is) would
// score above MaxNodeScore in the reference -- beyond the int32 planes for a
// small capacity, and beyond the totals the ranking bins and keys are sized
// for -- so it is refused like a too large one.
constexpr int64_t kExact = 1ll << 45;

inline bool exact_ok(int64_t v) { return v >= 0 && v < kExact; }

inline std::string exact_msg(const char *what) {
  return std::string(what) + ": quantity outside [0, 2^45), the engine's exact range";
}

constexpr size_t kNoSrc = ~(size_t)0;  // Column::src of a column no koordhip_node_soa slot feeds

// One device column of the loaded snapshot.
struct Column {
  const char *name;    // the ABI name (error text)
  void *dev;           // the device allocation, writable
  size_t esize;        // bytes per node element: 1, 2, 4, 8 or a whole row (ZoneRow, a node's device row)
  int32_t planes;      // [planes][n] elements, device plane stride n (0: `esize` bytes in all, not per node)
  size_t src;          // offset of the source's pointer slot in koordhip_node_soa (kNoSrc: none)
  bool q;              // an int64 quantity stored as exact f64 (the [0, 2^45) gate)
  bool mut;            // a Reserve mutates it: part of a checkpoint
  void *ckpt;          // its checkpoint copy (NULL: none taken)

  size_t bytes(int32_t n) const { return planes ? esize * (size_t)planes * (size_t)n : esize; }
};

// The pointer a koordhip_node_soa keeps in the slot at `off` (NULL: column absent).
inline const void *soa_slot(const void *soa, size_t off) {
  const void *p;
  std::memcpy(&p, static_cast<const char *>(soa) + off, sizeof(p));
  return p;
}

// One plane of update rows on its way to a column: src[j] -> dst[idx[j]].
struct RowSeg {
  void *dst;
  const void *src;
  size_t esize;
  bool q;
  const char *name;
};

// The scatter list of `rows` (m update rows as a koordhip_node_soa, source
// plane stride m) over the loaded columns: a NULL source leaves its column alone.
inline std::vector<RowSeg> row_segments(const std::vector<Column> &cols, const void *rows, int32_t m, int32_t n) {
  std::vector<RowSeg> segs;
  for (const Column &k : cols) {
    const char *src = k.src == kNoSrc ? nullptr : static_cast<const char *>(soa_slot(rows, k.src));
    if (!src) continue;
    for (int32_t p = 0; p < k.planes; p++)
      segs.push_back({static_cast<char *>(k.dev) + (size_t)p * n * k.esize, src + (size_t)p * m * k.esize, k.esize, k.q,
                      k.name});
  }
  return segs;
}

// The host staging image of an update: [idx][segment 0][segment 1]... in 8-byte
// aligned segments (padding zero), quantities converted to the device's exact
// f64, everything else copied.  off[q]: where segment q starts.  Returns false
// with *err set when a quantity is outside the exact range; makes no device call.
inline bool pack_rows(const std::vector<RowSeg> &segs, const int32_t *idx, int32_t m, std::vector<uint8_t> &img,
                      std::vector<size_t> &off, std::string *err) {
  const auto pad8 = [](size_t b) { return (b + 7) & ~(size_t)7; };
  size_t bytes = pad8((size_t)m * sizeof(int32_t));
  off.resize(segs.size());
  for (size_t q = 0; q < segs.size(); q++) {
    off[q] = bytes;
    bytes += pad8((size_t)m * segs[q].esize);
  }
  img.assign(bytes, 0);
  std::memcpy(img.data(), idx, (size_t)m * sizeof(int32_t));
  for (size_t q = 0; q < segs.size(); q++) {
    const RowSeg &k = segs[q];
    if (!k.q) {
      std::memcpy(img.data() + off[q], k.src, (size_t)m * k.esize);
      continue;
    }
    const int64_t *src = static_cast<const int64_t *>(k.src);
    for (int32_t j = 0; j < m; j++) {
      if (!exact_ok(src[j])) {
        *err = exact_msg(k.name);
        return false;
      }
      const double v = (double)src[j];
      std::memcpy(img.data() + off[q] + (size_t)j * sizeof(double), &v, sizeof(v));
    }
  }
  return true;
}

}  // namespace kh
