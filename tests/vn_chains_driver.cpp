// CPU check of the chained kept list (csrc/graph_tables.h: build_vn_chains), built under ASan/UBSan.
// The function permutes the kept list of the variable-node kernel's record form into blocks of W * L entries -- block
// position (t, w) is list index block * W * L + t * W + w, wave w walks t = 0 .. L - 1 -- and marks, in the spare bits of
// keep_rs, the edge whose record an entry takes from the wave's carry and the edge whose record it leaves there.
// Checked on every graph, for W = 1, 2, 3, 4 and L = 2, 4, 8, 16:
//   * the output is a permutation of the kept list, and deterministic;
//   * every entry has its variable's own list_ptr span and keep_rs words, edge for edge in the original order (flag bits
//     aside);
//   * carry consistency: an edge marked kChainFrom names the row that the previous entry of the same wave and block marked
//     kChainLeave; there is never a kChainFrom at t = 0; no entry has more than one kChainFrom or more than one kChainLeave;
//     every kChainLeave is taken up by the next entry; only an entry's first kChainEdges edges are marked;
//   * L = 1 equals build_vn_bundles word for word;
//   * the padding behind the last word;
//   * fetches / carried / issued equal a brute-force recount with std::set.
// Graphs: kept counts that are no multiple of W * L, of W or of L; a variable that shares no row with any other kept
// variable; isolated stars, where every chain must break after a few entries; a variable of more than kChainEdges edges;
// and the built-in DVB-S2 1/2 normal-frame tables, on which W = 4, L = 8 must issue at most 0.83 x 162 000 loads.
#include <algorithm>
#include <cstdio>
#include <map>
#include <set>
#include <string>

#include "../ldpc_toolbox_amd/csrc/codes.h"
#include "../ldpc_toolbox_amd/csrc/graph_tables.h"

using namespace ldpc;

#define REQUIRE(c)                                                                                             \
  do {                                                                                                         \
    if (!(c)) {                                                                                                \
      std::fprintf(stderr, "%s:%d: %s failed (%s, W = %u, L = %u)\n", __FILE__, __LINE__, #c, what, W, L);     \
      return 1;                                                                                                \
    }                                                                                                          \
  } while (0)

// [H0 | bidiagonal]: information column j sits in the rows cols[j]
static SparseMatrix staircase(uint32_t m, const std::vector<std::vector<uint32_t>> &cols) {
  const uint32_t k = static_cast<uint32_t>(cols.size());
  SparseMatrix h(m, k + m);
  for (uint32_t j = 0; j < k; j++)
    for (uint32_t r : cols[j]) h.insert(r % m, j);
  for (uint32_t r = 0; r < m; r++) {
    if (r) h.insert(r, k + r - 1);
    h.insert(r, k + r);
  }
  return h;
}

struct Counts {
  uint64_t fetches = 0, carried = 0, issued = 0;
};

static int check(const SparseMatrix::Csr &g, const char *what, uint32_t W, uint32_t L, Counts *out) {
  const LfreeTables lf = build_lfree_tables(g);
  REQUIRE(lf.ready);
  const KeepRsTable kr = build_keep_rs(g, lf);
  REQUIRE(kr.ready);
  const uint32_t n_keep = lf.n_keep;
  const VnChainTables t = build_vn_chains(n_keep, lf.keep_ptr, lf.keep_var, kr.rs, W, L);
  const VnChainTables again = build_vn_chains(n_keep, lf.keep_ptr, lf.keep_var, kr.rs, W, L);
  REQUIRE(t.list_var == again.list_var && t.list_ptr == again.list_ptr && t.keep_rs == again.keep_rs);  // deterministic
  REQUIRE(t.list_var.size() == n_keep && t.list_ptr.size() == size_t(n_keep) + 1 && t.list_ptr[0] == 0);
  REQUIRE(t.keep_rs.size() == lf.keep_edge.size() + kTablePad);
  REQUIRE(t.list_ptr[n_keep] == lf.keep_edge.size());
  REQUIRE(t.n_blocks == (n_keep + W * L - 1) / (W * L));
  // a permutation, every entry with its variable's own words in their order
  std::map<uint32_t, uint32_t> old_pos;
  for (uint32_t i = 0; i < n_keep; i++) old_pos[lf.keep_var[i]] = i;
  std::set<uint32_t> seen;
  for (uint32_t i = 0; i < n_keep; i++) {
    const auto it = old_pos.find(t.list_var[i]);
    REQUIRE(it != old_pos.end());
    REQUIRE(seen.insert(t.list_var[i]).second);
    const uint32_t o = it->second, d = lf.keep_ptr[o + 1] - lf.keep_ptr[o];
    REQUIRE(t.list_ptr[i + 1] - t.list_ptr[i] == d);
    for (uint32_t j = 0; j < d; j++) REQUIRE((t.keep_rs[t.list_ptr[i] + j] & kChainRsMask) == kr.rs[lf.keep_ptr[o] + j]);
  }
  for (size_t at = t.list_ptr[n_keep]; at < t.keep_rs.size(); at++) REQUIRE(t.keep_rs[at] == 0);
  if (L == 1) {
    const VnBundleTables b = build_vn_bundles(n_keep, lf.keep_ptr, lf.keep_var, kr.rs, W);
    REQUIRE(t.list_var == b.list_var && t.list_ptr == b.list_ptr && t.keep_rs == b.keep_rs);
    REQUIRE(t.fetches == b.fetches && t.issued == b.distinct && t.carried == 0);
  }
  // carry consistency, wave by wave: the kernel's own walk
  const uint32_t kNone = 0xFFFFFFFFu;
  uint64_t carried = 0, walked = 0;
  for (uint32_t blk = 0; blk < t.n_blocks; blk++)
    for (uint32_t w = 0; w < W; w++) {
      uint32_t carry = kNone;  // the row in the wave's carry
      for (uint32_t s = 0; s < L; s++) {
        const uint64_t at = (uint64_t(blk) * L + s) * W + w;
        if (at >= n_keep) break;
        walked++;
        uint32_t from = kNone, leave = kNone, n_from = 0, n_leave = 0;
        for (uint32_t j = t.list_ptr[at]; j < t.list_ptr[at + 1]; j++) {
          const uint32_t word = t.keep_rs[j], row = (word & kChainRsMask) >> 6;
          if (word & (kChainFrom | kChainLeave)) REQUIRE(j - t.list_ptr[at] < kChainEdges);
          if (word & kChainFrom) {
            from = row;
            n_from++;
          }
          if (word & kChainLeave) {
            leave = row;
            n_leave++;
          }
        }
        REQUIRE(n_from <= 1 && n_leave <= 1);
        if (s == 0) REQUIRE(n_from == 0);
        if (n_from) REQUIRE(carry != kNone && from == carry);
        if (!n_from) REQUIRE(carry == kNone);  // nothing is left in the carry that nobody takes
        carried += n_from;
        carry = n_leave ? leave : kNone;
      }
      REQUIRE(carry == kNone);  // the carry ends with the wave's walk of the block
    }
  REQUIRE(walked == n_keep);
  // the counts, recounted: per step the distinct rows among the step-mates that are not carried
  uint64_t fetches = 0, issued = 0;
  for (uint32_t i0 = 0; i0 < n_keep; i0 += W) {
    std::set<uint32_t> rows;
    for (uint32_t i = i0; i < std::min(n_keep, i0 + W); i++)
      for (uint32_t j = t.list_ptr[i]; j < t.list_ptr[i + 1]; j++) {
        fetches++;
        if (!(t.keep_rs[j] & kChainFrom)) rows.insert((t.keep_rs[j] & kChainRsMask) >> 6);
      }
    issued += rows.size();
  }
  REQUIRE(t.fetches == fetches && t.carried == carried && t.issued == issued);
  REQUIRE(fetches == lf.keep_edge.size() && issued + carried <= fetches);
  Counts c;
  count_vn_chain_fetches(n_keep, t.list_ptr, t.keep_rs, W, L, &c.fetches, &c.carried, &c.issued);
  REQUIRE(c.fetches == fetches && c.carried == carried && c.issued == issued);
  *out = c;
  return 0;
}

int main() {
  const uint32_t widths[] = {1, 2, 3, 4}, lengths[] = {1, 2, 4, 8, 16};
  {
    // 5 columns of weight 8, 6 of weight 4, 7 of weight 3: 18 kept, no multiple of any block, on 37 rows; column 0 of weight 3
    // sits alone in rows 34..36, which no other information column touches
    const char *what = "mixed degrees 3 / 4 / 8";
    std::vector<std::vector<uint32_t>> cols;
    cols.push_back({34, 35, 36});
    for (uint32_t j = 0; j < 5; j++) {
      std::vector<uint32_t> c;
      for (uint32_t i = 0; i < 8; i++) c.push_back(j + 4 * i);
      cols.push_back(c);
    }
    for (uint32_t j = 0; j < 6; j++) cols.push_back({j, j + 9, j + 17, j + 26});
    for (uint32_t j = 0; j < 6; j++) cols.push_back({2 * j + 1, 2 * j + 12, (2 * j + 25) % 34});
    const SparseMatrix::Csr g = staircase(37, cols).csr();
    for (uint32_t W : widths)
      for (uint32_t L : lengths) {
        Counts c;
        if (check(g, what, W, L, &c)) return 1;
        REQUIRE(build_lfree_tables(g).n_keep == 18);
        if (L > 1) REQUIRE(c.carried > 0);  // these columns do share rows
      }
    std::printf("mixed degrees, 18 kept: ok\n");
  }
  {
    // no two kept variables share a row: nothing to carry
    const char *what = "no shared rows";
    std::vector<std::vector<uint32_t>> cols;
    for (uint32_t j = 0; j < 7; j++) cols.push_back({3 * j, 3 * j + 1, 3 * j + 2});
    const SparseMatrix::Csr g = staircase(21, cols).csr();
    for (uint32_t W : widths)
      for (uint32_t L : lengths) {
        Counts c;
        if (check(g, what, W, L, &c)) return 1;
        REQUIRE(c.carried == 0 && c.issued == c.fetches);
      }
    std::printf("no shared rows, 7 kept: ok\n");
  }
  {
    // isolated stars: columns 3s, 3s + 1, 3s + 2 meet in row 10 s and nowhere else: a chain ends after 3 entries
    const char *what = "isolated stars";
    std::vector<std::vector<uint32_t>> cols;
    for (uint32_t s = 0; s < 5; s++)
      for (uint32_t a = 0; a < 3; a++) cols.push_back({10 * s, 10 * s + 1 + 3 * a, 10 * s + 2 + 3 * a, 10 * s + 3 + 3 * a});
    const SparseMatrix::Csr g = staircase(50, cols).csr();
    for (uint32_t W : widths)
      for (uint32_t L : lengths) {
        Counts c;
        if (check(g, what, W, L, &c)) return 1;
        REQUIRE(c.carried <= 10);  // two links per star at most
        if (L == 4 && W == 1) REQUIRE(c.carried >= 5);
      }
    std::printf("isolated stars, 15 kept: ok\n");
  }
  {
    // a column of 11 edges: only its first kChainEdges take part; the others' rows are shared too
    const char *what = "long column";
    std::vector<std::vector<uint32_t>> cols;
    cols.push_back({0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10});
    for (uint32_t j = 0; j < 11; j++) cols.push_back({j, 12 + j, 24 + j});
    const SparseMatrix::Csr g = staircase(40, cols).csr();
    for (uint32_t W : widths)
      for (uint32_t L : lengths) {
        Counts c;
        if (check(g, what, W, L, &c)) return 1;
      }
    std::printf("long column, 12 kept: ok\n");
  }
  {
    const char *what = "dvbs2:R1_2";
    SparseMatrix h;
    uint32_t W = 4, L = 8;
    REQUIRE(codes::dvbs2("R1_2", &h));
    const SparseMatrix::Csr g = h.csr();
    const uint32_t ls[] = {1, 4, 8, 16};
    for (uint32_t l : ls) {
      L = l;
      Counts c;
      if (check(g, what, W, L, &c)) return 1;
      REQUIRE(c.fetches == 162000);
      std::printf("dvbs2:R1_2: W = 4, L = %u: %llu fetches, %llu carried, %llu issued\n", L, (unsigned long long)c.fetches,
                  (unsigned long long)c.carried, (unsigned long long)c.issued);
      if (L == 8) REQUIRE(c.issued * 100 <= c.fetches * 83);
    }
  }
  std::printf("vn_chains driver: ok\n");
  return 0;
}
