// Stand-alone check of the host-only part of koordhip_update_nodes
// (koordinator_amd/csrc/snapshot_cols.hpp): the scatter list over a column
// table and the staging image -- offsets, alignment, the f64 conversion with
// its [0, 2^45) gate, zero padding.  tests/test_snapshot_pack.py builds it with
// the host compiler under -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>

#include "../koordinator_amd/csrc/snapshot_cols.hpp"

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

namespace {

struct Row {  // a 24-byte wide row
  int32_t v[6];
};

// rows as update_nodes gets them: a struct of column pointers
struct Soa {
  const int64_t *qty;
  const int32_t *i32;
  const uint16_t *u16;
  const uint8_t *u8;
  const Row *wide;
  const int32_t *planes;  // [3][m]
  const int64_t *absent;
};

template <typename T>
T at(const std::vector<uint8_t> &img, size_t off, size_t j) {
  T v;
  std::memcpy(&v, img.data() + off + j * sizeof(T), sizeof(T));
  return v;
}

size_t pad8(size_t b) { return (b + 7) & ~(size_t)7; }

void check_m(int32_t m) {
  const int32_t n = 40;
  std::vector<int64_t> qty(m);
  std::vector<int32_t> i32(m), planes(3 * (size_t)m), idx(m);
  std::vector<uint16_t> u16(m);
  std::vector<uint8_t> u8(m);
  std::vector<Row> wide(m);
  for (int32_t j = 0; j < m; j++) {
    idx[j] = (j * 7 + 3) % n;
    qty[j] = j == 0 ? kh::kExact - 1 : (int64_t)j * 1000003;
    i32[j] = -j - 1;
    u16[j] = (uint16_t)(0xA000 + j);
    u8[j] = (uint8_t)(j + 1);
    for (int w = 0; w < 6; w++) wide[j].v[w] = j * 10 + w;
    for (int p = 0; p < 3; p++) planes[(size_t)p * m + j] = 100 * p + j;
  }
  const Soa soa{qty.data(), i32.data(), u16.data(), u8.data(), wide.data(), planes.data(), nullptr};
  // device columns stand-ins (never dereferenced here)
  std::vector<char> dev(8 * (size_t)n * 3);
  char *d = dev.data();
  const std::vector<kh::Column> cols = {
      {"qty", d, 8, 1, offsetof(Soa, qty), true, true, nullptr},
      {"i32", d, 4, 1, offsetof(Soa, i32), false, false, nullptr},
      {"u16", d, 2, 1, offsetof(Soa, u16), false, false, nullptr},
      {"u8", d, 1, 1, offsetof(Soa, u8), false, true, nullptr},
      {"wide", d, sizeof(Row), 1, offsetof(Soa, wide), false, false, nullptr},
      {"planes", d, 4, 3, offsetof(Soa, planes), false, true, nullptr},
      {"absent", d, 8, 1, offsetof(Soa, absent), true, false, nullptr},   // NULL source: left alone
      {"flags", d, 1, 1, kh::kNoSrc, false, true, nullptr},               // no source at all
      {"sums", d, 64, 0, kh::kNoSrc, false, false, nullptr},              // not per node
  };
  CHECK(cols[0].bytes(n) == 8u * n && cols[5].bytes(n) == 12u * n && cols[8].bytes(n) == 64);

  const std::vector<kh::RowSeg> segs = kh::row_segments(cols, &soa, m, n);
  CHECK(segs.size() == 8);  // five one-plane columns and three planes
  for (int p = 0; p < 3; p++) {
    CHECK(segs[5 + p].dst == d + (size_t)p * n * 4);                      // device plane stride n
    CHECK(segs[5 + p].src == planes.data() + (size_t)p * m);              // source plane stride m
  }

  std::vector<uint8_t> img(5, 0xEE);  // reused between calls: stale bytes must not survive
  std::vector<size_t> off;
  std::string err;
  CHECK(kh::pack_rows(segs, idx.data(), m, img, off, &err) && err.empty());
  const size_t esz[8] = {8, 4, 2, 1, sizeof(Row), 4, 4, 4};
  size_t at_ = pad8((size_t)m * 4);
  CHECK(off.size() == 8);
  for (int q = 0; q < 8; q++) {
    CHECK(off[q] == at_ && off[q] % 8 == 0);
    at_ += pad8((size_t)m * esz[q]);
  }
  CHECK(img.size() == at_);
  std::vector<bool> data(img.size(), false);
  auto mark = [&](size_t o, size_t b) {
    for (size_t x = 0; x < b; x++) data[o + x] = true;
  };
  mark(0, (size_t)m * 4);
  for (int q = 0; q < 8; q++) mark(off[q], (size_t)m * esz[q]);
  for (size_t x = 0; x < img.size(); x++)
    if (!data[x]) CHECK(img[x] == 0);  // padding
  for (int32_t j = 0; j < m; j++) {
    CHECK(at<int32_t>(img, 0, j) == idx[j]);
    CHECK(at<double>(img, off[0], j) == (double)qty[j] && (int64_t)at<double>(img, off[0], j) == qty[j]);
    CHECK(at<int32_t>(img, off[1], j) == i32[j]);
    CHECK(at<uint16_t>(img, off[2], j) == u16[j]);
    CHECK(at<uint8_t>(img, off[3], j) == u8[j]);
    for (int w = 0; w < 6; w++) CHECK(at<int32_t>(img, off[4], (size_t)j * 6 + w) == wide[j].v[w]);
    for (int p = 0; p < 3; p++) CHECK(at<int32_t>(img, off[5 + p], j) == 100 * p + j);
  }

  // the gate: 2^45 and -1 are refused wherever they stand, and named
  for (int64_t bad : {kh::kExact, (int64_t)-1}) {
    std::vector<int64_t> q2 = qty;
    q2[m - 1] = bad;
    Soa s2 = soa;
    s2.qty = q2.data();
    err.clear();
    CHECK(!kh::pack_rows(kh::row_segments(cols, &s2, m, n), idx.data(), m, img, off, &err));
    CHECK(err.find("qty") == 0 && err.find("2^45") != std::string::npos);
  }
  // ... while a raw 8-byte column takes any bit pattern
  std::vector<kh::Column> raw = {{"raw", d, 8, 1, offsetof(Soa, qty), false, false, nullptr}};
  std::vector<int64_t> q3(m, -1);
  Soa s3 = soa;
  s3.qty = q3.data();
  CHECK(kh::pack_rows(kh::row_segments(raw, &s3, m, n), idx.data(), m, img, off, &err));
  CHECK(at<int64_t>(img, off[0], m - 1) == -1);
}

}  // namespace

int main() {
  CHECK(kh::exact_ok(0) && kh::exact_ok(kh::kExact - 1) && !kh::exact_ok(kh::kExact) && !kh::exact_ok(-1));
  for (int32_t m : {1, 3, 5, 7, 8, 13, 64})  // mostly not multiples of 8
    check_m(m);
  std::puts("snapshot_pack_check ok");
  return 0;
}
