// CPU check of the width of a row record's flags word (csrc/graph_tables.h: record_flag_bits, RowRecordTables::flag_bits),
// built under ASan/UBSan.  A flags word holds one flip bit per edge of the row and the argmin slot, ceil(log2(weight)) bits
// (one bit for a single edge).  The expectation is restated here from that sentence alone:
//   * 16 bits where weight + argmin bits <= 16, which is weight <= 12;
//   * else the decoder's own word, 32 bits in f32 and 64 in f64, as long as the row's flip bits fit it at all;
//   * the record FAMILY (words of the decoder's type per record) is a separate matter and stays what it was: 3 up to 26
//     edges in f32 and 58 in f64 (flip bits and argmin share the third word), 4 beyond.
// Both sides of every boundary -- 12 | 13, 26 | 27, 32 | 33 in f32, 58 | 59, 64 | 65 in f64 -- are checked on the function
// and on the tables of a small staircase graph whose longest row has exactly that weight.
#include <cstdio>

#include "../ldpc_toolbox_amd/csrc/graph_tables.h"

using namespace ldpc;

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) {                                                                          \
      std::fprintf(stderr, "%s:%d: %s failed (weight %u)\n", __FILE__, __LINE__, #c, w); \
      return 1;                                                                          \
    }                                                                                    \
  } while (0)

static uint32_t arg_bits_by_counting(uint32_t w) {
  uint32_t bits = 0;
  for (uint32_t reach = 1; reach < w; reach *= 2) bits++;  // smallest b with 2^b >= w
  return bits == 0 ? 1 : bits;
}
static uint32_t expected_bits(uint32_t w, bool f64) {
  const uint32_t word = f64 ? 64u : 32u;
  if (w > word) return 0;
  return w + arg_bits_by_counting(w) <= 16 ? 16u : word;
}

// [H0 | bidiagonal] with k information columns and m rows: every row takes 3 information columns, cyclically, and row
// `m / 2` as many as make its weight exactly wmax (its two staircase entries included)
static SparseMatrix staircase(uint32_t k, uint32_t m, uint32_t wmax) {
  SparseMatrix h(m, k + m);
  for (uint32_t r = 0; r < m; r++) {
    const uint32_t info = r == m / 2 ? wmax - 2 : 3;
    for (uint32_t j = 0; j < info; j++) h.insert(r, (r * 5 + j) % k);
    if (r) h.insert(r, k + r - 1);
    h.insert(r, k + r);
  }
  return h;
}

int main() {
  for (uint32_t w = 1; w <= 64; w++)
    for (bool f64 : {false, true}) {
      REQUIRE(record_flag_bits(w, f64) == expected_bits(w, f64));
      REQUIRE(record_arg_bits(w) == arg_bits_by_counting(w));
    }
  {
    const uint32_t w = 0;
    REQUIRE(record_flag_bits(0, false) == 0 && record_flag_bits(0, true) == 0 && record_flag_bits(65, true) == 0);
  }
  // the boundaries, spelled out
  {
    const uint32_t w = 12;
    REQUIRE(record_flag_bits(12, false) == 16 && record_flag_bits(12, true) == 16);
    REQUIRE(record_flag_bits(13, false) == 32 && record_flag_bits(13, true) == 64);
    REQUIRE(record_flag_bits(32, false) == 32 && record_flag_bits(33, false) == 0 && record_flag_bits(33, true) == 64);
  }
  for (uint32_t w : {5u, 12u, 13u, 26u, 27u, 32u, 33u, 58u, 59u, 64u, 65u}) {
    const SparseMatrix::Csr g = staircase(70, 30, w).csr();
    REQUIRE(g.max_row_weight == w);
    const LfreeTables lf = build_lfree_tables(g);
    REQUIRE(lf.ready);
    for (bool f64 : {false, true}) {
      const RowRecordTables t = build_row_record_tables(g, lf, f64);
      REQUIRE(t.ready == (w <= (f64 ? 64u : 32u)));
      if (!t.ready) {
        REQUIRE(t.flag_bits == 0 && t.rec_w == 0);
        continue;
      }
      REQUIRE(t.flag_bits == expected_bits(w, f64));
      REQUIRE(t.rec_w == (w <= (f64 ? 58u : 26u) ? 3u : 4u));
      REQUIRE(t.flag_bits != 16 || t.rec_w == 3);  // 16-bit flags only in the three-word family
    }
    std::printf("staircase, longest row %u: ok\n", w);
  }
  std::printf("record flags driver: ok\n");
  return 0;
}
