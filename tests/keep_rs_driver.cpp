// CPU check of the variable-node kernel's record source table (csrc/graph_tables.h: build_keep_rs), built under ASan/UBSan.
// The table holds, for every edge of the kept list (the variables of degree >= 3, in keep_var / keep_ptr order, a variable's
// edges in cols[v] order), the word  row << 6 | slot of the edge inside its row.  The expectation is a direct walk of the
// alist the matrix writes (and a decoder parses): its row lists give (row, slot) of every entry, its column lists the
// cols[v] order.
// Cases: kept variables of weight 3, 8, 9 and 13; a variable whose edges sit in the first and in the last row; a 12-edge
// row; the padding behind the last word; and the refusals -- a slot that does not fit 6 bits, a row index that does not fit
// the word (free_rs's limits), a graph without L-free or without kept variables.
#include <algorithm>
#include <cstdio>
#include <map>
#include <sstream>
#include <string>
#include <utility>

#include "../ldpc_toolbox_amd/csrc/graph_tables.h"

using namespace ldpc;

#define REQUIRE(c)                                                                     \
  do {                                                                                 \
    if (!(c)) {                                                                        \
      std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, what);   \
      return 1;                                                                        \
    }                                                                                  \
  } while (0)

// [H0 | bidiagonal]: m rows, information column j has weight w[j] and sits in rows (start[j] + i * step[j]) % m
struct Col {
  uint32_t weight, start, step;
};
static SparseMatrix staircase(uint32_t m, const std::vector<Col> &cols) {
  const uint32_t k = static_cast<uint32_t>(cols.size());
  SparseMatrix h(m, k + m);
  for (uint32_t j = 0; j < k; j++)
    for (uint32_t i = 0; i < cols[j].weight; i++) h.insert((cols[j].start + i * cols[j].step) % m, j);
  for (uint32_t r = 0; r < m; r++) {
    if (r) h.insert(r, k + r - 1);
    h.insert(r, k + r);
  }
  return h;
}

// (row, slot) of every entry and the cols[v] order, read from the alist text alone (1-based indices, 0 = padding):
// n m / max col weight, max row weight / column weights / row weights / n column lists / m row lists
struct AlistWalk {
  uint32_t n = 0, m = 0;
  std::vector<std::vector<uint32_t>> col_rows;            // per variable: its rows in the order the alist lists them
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> slot;  // (row, column) -> position in the row's list
};
static AlistWalk walk(const std::string &alist) {
  std::istringstream in(alist);
  AlistWalk a;
  uint32_t maxc = 0, maxr = 0;
  in >> a.n >> a.m >> maxc >> maxr;
  std::vector<uint32_t> cw(a.n), rw(a.m);
  for (auto &x : cw) in >> x;
  for (auto &x : rw) in >> x;
  a.col_rows.resize(a.n);
  auto list = [&](uint32_t count, std::vector<uint32_t> *out) {
    // a list is `count` entries, possibly followed by zero padding up to the line's end
    std::string line;
    while (line.find_first_not_of(" \t\r") == std::string::npos && std::getline(in, line)) {
    }
    std::istringstream ls(line);
    uint32_t x;
    while (ls >> x)
      if (x != 0) out->push_back(x - 1);
    return out->size() == count;
  };
  for (uint32_t v = 0; v < a.n; v++)
    if (!list(cw[v], &a.col_rows[v])) return AlistWalk();
  for (uint32_t r = 0; r < a.m; r++) {
    std::vector<uint32_t> cs;
    if (!list(rw[r], &cs)) return AlistWalk();
    for (uint32_t s = 0; s < cs.size(); s++) a.slot[{r, cs[s]}] = s;
  }
  return a;
}

// the table of `h` against the walk of its alist; *weights: the kept variables' weights seen
static int check(const SparseMatrix &built, const char *what, std::vector<uint32_t> *weights, uint32_t *longest_row) {
  const std::string text = built.alist();
  const AlistWalk a = walk(text);
  REQUIRE(a.n == built.num_cols() && a.m == built.num_rows());
  SparseMatrix h;  // as a decoder gets it: parsed from the alist
  std::string err;
  REQUIRE(SparseMatrix::from_alist(text, &h, &err));
  const SparseMatrix::Csr g = h.csr();
  const LfreeTables lf = build_lfree_tables(g);
  REQUIRE(lf.ready);
  const KeepRsTable t = build_keep_rs(g, lf);
  REQUIRE(t.ready);
  REQUIRE(t.rs.size() == lf.keep_edge.size() + kTablePad);
  size_t at = 0;
  for (size_t i = 0; i < lf.keep_var.size(); i++) {
    const uint32_t v = lf.keep_var[i];
    REQUIRE(lf.keep_ptr[i] == at);
    const std::vector<uint32_t> &rows = a.col_rows[v];
    REQUIRE(rows.size() >= 3 && lf.keep_ptr[i + 1] - lf.keep_ptr[i] == rows.size());
    weights->push_back(static_cast<uint32_t>(rows.size()));
    for (uint32_t r : rows) {
      const auto it = a.slot.find({r, v});
      REQUIRE(it != a.slot.end());
      REQUIRE((t.rs[at] >> 6) == r);
      REQUIRE((t.rs[at] & 63u) == it->second);
      at++;
    }
  }
  REQUIRE(at == lf.keep_edge.size());
  for (; at < t.rs.size(); at++) REQUIRE(t.rs[at] == 0);  // the padding reads as row 0, slot 0: in bounds
  *longest_row = g.max_row_weight;
  return 0;
}

int main() {
  const char *what = "";
  auto has = [](const std::vector<uint32_t> &ws, uint32_t w) { return std::find(ws.begin(), ws.end(), w) != ws.end(); };
  {
    // weights 3, 8, 9 and 13 on 40 rows; column 4 sits in rows 0, 13, 26 and 39: the first and the last row; the 12-edge row:
    // row 20 takes the columns 5..13 beside 0..3's strides -- counted below, not assumed
    what = "weights 3 / 8 / 9 / 13";
    std::vector<Col> cols = {{3, 1, 7}, {8, 2, 5}, {9, 0, 4}, {13, 0, 3}, {4, 0, 13}};
    for (uint32_t j = 0; j < 9; j++) cols.push_back({3, 20, 9 + j});  // nine columns that all start in row 20
    std::vector<uint32_t> ws;
    uint32_t longest = 0;
    const SparseMatrix built = staircase(40, cols);
    if (check(built, what, &ws, &longest)) return 1;
    SparseMatrix h;
    std::string err;
    REQUIRE(SparseMatrix::from_alist(built.alist(), &h, &err));
    REQUIRE(has(ws, 3) && has(ws, 8) && has(ws, 9) && has(ws, 13) && has(ws, 4));
    REQUIRE(longest == 12);
    // the variable of the first and the last row, spelled out: its words are rows 0, 13, 26, 39
    const SparseMatrix::Csr g = h.csr();
    const LfreeTables lf = build_lfree_tables(g);
    const KeepRsTable t = build_keep_rs(g, lf);
    bool seen = false;
    for (size_t i = 0; i < lf.keep_var.size(); i++)
      if (lf.keep_var[i] == 4) {
        const uint32_t p = lf.keep_ptr[i];
        REQUIRE(lf.keep_ptr[i + 1] - p == 4);
        REQUIRE((t.rs[p] >> 6) == 0 && (t.rs[p + 1] >> 6) == 13 && (t.rs[p + 2] >> 6) == 26 && (t.rs[p + 3] >> 6) == 39);
        REQUIRE((t.rs[p + 3] & 63u) < g.row_ptr[40] - g.row_ptr[39]);
        seen = true;
      }
    REQUIRE(seen);
    std::printf("weights 3, 8, 9, 13 with a 12-edge row: ok\n");
  }
  {
    what = "64-edge row";  // the last slot that fits the word's 6 bits
    std::vector<Col> cols;
    for (uint32_t j = 0; j < 62; j++) cols.push_back({3, 5, 1 + j % 9});
    std::vector<uint32_t> ws;
    uint32_t longest = 0;
    if (check(staircase(30, cols), what, &ws, &longest)) return 1;
    REQUIRE(longest == 64);
    std::printf("64-edge row: ok\n");
  }
  {
    what = "refusals";
    std::vector<Col> cols;
    for (uint32_t j = 0; j < 63; j++) cols.push_back({3, 5, 1 + j % 9});
    const SparseMatrix::Csr g = staircase(30, cols).csr();  // a 65-edge row: slot 64 does not fit
    REQUIRE(g.max_row_weight == 65);
    const LfreeTables lf = build_lfree_tables(g);
    REQUIRE(lf.ready);
    REQUIRE(!build_keep_rs(g, lf).ready && build_keep_rs(g, lf).rs.empty());
    // a row index beyond the word: the function looks at the counts before it looks at the arrays
    SparseMatrix::Csr big = staircase(30, {{3, 0, 7}}).csr();
    const LfreeTables lfb = build_lfree_tables(big);
    REQUIRE(build_keep_rs(big, lfb).ready);
    big.n_rows = dev::kPeerSingle;
    REQUIRE(!build_keep_rs(big, lfb).ready);
    // no kept variable at all (a bare staircase), no L-free variable at all (every column of weight 3)
    const SparseMatrix::Csr bare = staircase(12, {}).csr();
    REQUIRE(!build_keep_rs(bare, build_lfree_tables(bare)).ready);
    SparseMatrix dense(6, 6);
    for (uint32_t c = 0; c < 6; c++)
      for (uint32_t i = 0; i < 3; i++) dense.insert((c + i) % 6, c);
    const SparseMatrix::Csr dg = dense.csr();
    REQUIRE(!build_keep_rs(dg, build_lfree_tables(dg)).ready);
    std::printf("refusals: ok\n");
  }
  std::printf("keep_rs driver: ok\n");
  return 0;
}
