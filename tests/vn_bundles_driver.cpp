// CPU check of the bundled kept list (csrc/graph_tables.h: build_vn_bundles), built under ASan/UBSan.
// The function permutes the kept list of the variable-node kernel's record form into aligned bundles of W entries whose
// variables share rows.  Checked on every graph, for W = 1, 2, 3, 4 and 8:
//   * the output is a permutation of the kept list;
//   * every entry has its variable's own list_ptr span and keep_rs words, edge for edge in the original order;
//   * bundles are aligned: the entries [k W, k W + W) never hold more distinct degrees than a fresh walk of the list could
//     avoid -- spelled out below as: a bundle mixes degrees only when the seed's degree has run out;
//   * W = 1 is the identity;
//   * the padding behind the last word;
//   * the two counts equal a brute-force recount with std::set.
// Graphs: kept counts that are no multiple of W; degree classes of 3, 4 and 8 none of which is a multiple of 4; a variable
// that shares no row with any other kept variable; and the built-in DVB-S2 1/2 normal-frame tables, on which W = 4 must save
// at least 12 % of the record fetches (the greedy reaches 13.3 %; a bundle of 4 is a tree on a graph of girth 6, so 15 % is
// the ceiling).
#include <algorithm>
#include <cstdio>
#include <map>
#include <set>
#include <string>

#include "../ldpc_toolbox_amd/csrc/codes.h"
#include "../ldpc_toolbox_amd/csrc/graph_tables.h"

using namespace ldpc;

#define REQUIRE(c)                                                                     \
  do {                                                                                 \
    if (!(c)) {                                                                        \
      std::fprintf(stderr, "%s:%d: %s failed (%s, W = %u)\n", __FILE__, __LINE__, #c, what, W); \
      return 1;                                                                        \
    }                                                                                  \
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

struct Saved {
  uint64_t fetches = 0, distinct = 0, plain = 0;  // plain: distinct of the list in its first order
};

static int check(const SparseMatrix::Csr &g, const char *what, uint32_t W, Saved *saved) {
  const LfreeTables lf = build_lfree_tables(g);
  REQUIRE(lf.ready);
  const KeepRsTable kr = build_keep_rs(g, lf);
  REQUIRE(kr.ready);
  const uint32_t n_keep = lf.n_keep;
  const VnBundleTables t = build_vn_bundles(n_keep, lf.keep_ptr, lf.keep_var, kr.rs, W);
  const VnBundleTables again = build_vn_bundles(n_keep, lf.keep_ptr, lf.keep_var, kr.rs, W);
  REQUIRE(t.list_var == again.list_var && t.list_ptr == again.list_ptr && t.keep_rs == again.keep_rs);  // deterministic
  REQUIRE(t.list_var.size() == n_keep && t.list_ptr.size() == size_t(n_keep) + 1 && t.list_ptr[0] == 0);
  REQUIRE(t.keep_rs.size() == lf.keep_edge.size() + kTablePad);
  REQUIRE(t.list_ptr[n_keep] == lf.keep_edge.size());
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
    for (uint32_t j = 0; j < d; j++) REQUIRE(t.keep_rs[t.list_ptr[i] + j] == kr.rs[lf.keep_ptr[o] + j]);
  }
  for (size_t at = t.list_ptr[n_keep]; at < t.keep_rs.size(); at++) REQUIRE(t.keep_rs[at] == 0);
  if (W == 1) {
    REQUIRE(t.list_var == lf.keep_var && t.list_ptr == lf.keep_ptr && t.keep_rs == kr.rs);
    REQUIRE(t.fetches == lf.keep_edge.size() && t.distinct == t.fetches);
  }
  // aligned bundles: bundle k is the entries [k W, k W + W); it mixes degrees only when no unplaced entry of its first
  // entry's degree was left -- every entry of that degree lies in this bundle or in an earlier one
  std::map<uint32_t, uint32_t> last_of_degree;  // degree -> last bundle that holds it
  auto deg = [&](uint32_t i) { return t.list_ptr[i + 1] - t.list_ptr[i]; };
  for (uint32_t i = 0; i < n_keep; i++) last_of_degree[deg(i)] = i / W;
  uint64_t fetches = 0, distinct = 0;
  for (uint32_t i0 = 0; i0 < n_keep; i0 += W) {
    std::set<uint32_t> rows;
    for (uint32_t i = i0; i < std::min(n_keep, i0 + W); i++) {
      if (deg(i) != deg(i0)) REQUIRE(last_of_degree[deg(i0)] <= i0 / W);
      for (uint32_t j = t.list_ptr[i]; j < t.list_ptr[i + 1]; j++) {
        rows.insert(t.keep_rs[j] >> 6);
        fetches++;
      }
    }
    distinct += rows.size();
  }
  REQUIRE(t.fetches == fetches && t.distinct == distinct);
  REQUIRE(fetches == lf.keep_edge.size() && distinct <= fetches);
  // the same count of the list in its first order, through the function the decoder reports any W with
  uint64_t f0 = 0, d0 = 0;
  count_vn_bundle_fetches(n_keep, lf.keep_ptr, kr.rs, W, &f0, &d0);
  REQUIRE(f0 == fetches && d0 <= f0);
  saved->plain = d0;
  saved->fetches = fetches;
  saved->distinct = distinct;
  return 0;
}

int main() {
  const uint32_t widths[] = {1, 2, 3, 4, 8};
  {
    // 5 columns of weight 8, 6 of weight 4, 7 of weight 3: 18 kept, no class a multiple of 4, on 37 rows; column 0 of weight 3
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
    for (uint32_t W : widths) {
      Saved s;
      if (check(g, what, W, &s)) return 1;
      const LfreeTables lf = build_lfree_tables(g);
      REQUIRE(lf.n_keep == 18);
      std::map<uint32_t, uint32_t> classes;
      for (uint32_t i = 0; i < lf.n_keep; i++) classes[lf.keep_ptr[i + 1] - lf.keep_ptr[i]]++;
      REQUIRE(classes.size() == 3 && classes[3] == 7 && classes[4] == 6 && classes[8] == 5);
      if (W > 1) REQUIRE(s.distinct < s.fetches);  // these columns do share rows
    }
    std::printf("mixed degrees, 18 kept: ok\n");
  }
  {
    // no two kept variables share a row: every bundle is filled in list order, the list comes back unchanged
    const char *what = "no shared rows";
    std::vector<std::vector<uint32_t>> cols;
    for (uint32_t j = 0; j < 7; j++) cols.push_back({3 * j, 3 * j + 1, 3 * j + 2});
    const SparseMatrix::Csr g = staircase(21, cols).csr();
    for (uint32_t W : widths) {
      Saved s;
      if (check(g, what, W, &s)) return 1;
      REQUIRE(s.distinct == s.fetches);
      const LfreeTables lf = build_lfree_tables(g);
      const VnBundleTables t = build_vn_bundles(lf.n_keep, lf.keep_ptr, lf.keep_var, build_keep_rs(g, lf).rs, W);
      REQUIRE(t.list_var == lf.keep_var);
    }
    std::printf("no shared rows, 7 kept: ok\n");
  }
  {
    // a chain: column j shares one row with column j + 2 only, so the greedy must reach past its neighbour
    const char *what = "chain";
    const uint32_t W = 2;
    std::vector<std::vector<uint32_t>> cols;
    for (uint32_t j = 0; j < 9; j++) cols.push_back({4 * j, 4 * j + 1, 4 * (j + 2) + 1});
    const SparseMatrix::Csr g = staircase(48, cols).csr();
    Saved s;
    if (check(g, what, W, &s)) return 1;
    const LfreeTables lf = build_lfree_tables(g);
    const VnBundleTables t = build_vn_bundles(lf.n_keep, lf.keep_ptr, lf.keep_var, build_keep_rs(g, lf).rs, W);
    const std::vector<uint32_t> want = {0, 2, 1, 3, 4, 6, 5, 7, 8};
    REQUIRE(t.list_var == want);
    REQUIRE(s.fetches == 27 && s.distinct == 23);
    std::printf("chain: ok\n");
  }
  {
    const char *what = "dvbs2:R1_2";
    SparseMatrix h;
    uint32_t W = 4;
    REQUIRE(codes::dvbs2("R1_2", &h));
    const SparseMatrix::Csr g = h.csr();
    Saved s4, s8, s1;
    if (check(g, what, 4, &s4)) return 1;
    REQUIRE(s4.fetches == 162000);
    REQUIRE(s4.plain == s4.fetches);  // in variable order the entries 4k .. 4k+3 touch rows q apart: nothing shared
    REQUIRE(s4.distinct * 100 <= s4.fetches * 88);  // at least 12 % saved
    REQUIRE(s4.distinct * 100 >= s4.fetches * 85);  // a bundle of 4 is a tree: at most 3 shared rows of 32 or 12
    W = 8;
    if (check(g, what, 8, &s8)) return 1;
    REQUIRE(s8.distinct < s4.distinct);
    W = 1;
    if (check(g, what, 1, &s1)) return 1;
    std::printf("dvbs2:R1_2: W = 4 %llu -> %llu, W = 8 %llu -> %llu: ok\n", (unsigned long long)s4.fetches,
                (unsigned long long)s4.distinct, (unsigned long long)s8.fetches, (unsigned long long)s8.distinct);
  }
  std::printf("vn_bundles driver: ok\n");
  return 0;
}
