// CPU check of the layered schedule's host tables (csrc/slice_tasks.h): dependency levels and the row records of the
// register-resident level kernels, built for the alist files given on the command line under ASan/UBSan.  Invariants:
//  * rows of one level share no variable, and a row's level is one more than the highest level among the earlier rows
//    it shares a variable with (horizontal_layered.rs:105-110: level order == row order, as far as any result can tell);
//  * a level's row records list its rows in level order: first edge, degree, variables, padded with the last variable.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

#include "../ldpc_toolbox_amd/csrc/slice_tasks.h"
#include "../ldpc_toolbox_amd/csrc/sparse.h"

using namespace ldpc;

#define REQUIRE(c)                                                        \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, path); \
      return 1;                                                           \
    }                                                                     \
  } while (0)

static int check(const char *path) {
  std::string err, text;
  if (FILE *f = std::fopen(path, "rb")) {
    char buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got);
    std::fclose(f);
  }
  SparseMatrix h;
  if (!SparseMatrix::from_alist(text, &h, &err)) {
    std::fprintf(stderr, "%s: %s\n", path, err.c_str());
    return 1;
  }
  const SparseMatrix::Csr g = h.csr();
  const LevelTables lv = build_levels(g.row_ptr, g.edge_col, g.n_rows, g.n_cols);
  const size_t n_levels = lv.maxdeg.size();
  REQUIRE(lv.level_ptr.size() == n_levels + 1 && lv.level_ptr.back() == g.n_rows);
  std::vector<uint32_t> level_of(g.n_rows, 0);
  for (size_t l = 0; l < n_levels; l++) {
    std::set<uint32_t> vars;
    for (uint32_t k = lv.level_ptr[l]; k < lv.level_ptr[l + 1]; k++) {
      const uint32_t r = lv.rows[k];
      level_of[r] = uint32_t(l);
      REQUIRE(k == lv.level_ptr[l] || lv.rows[k - 1] < r);  // row order inside a level
      for (uint32_t e = g.row_ptr[r]; e < g.row_ptr[r + 1]; e++) REQUIRE(vars.insert(g.edge_col[e]).second);
    }
  }
  std::vector<int64_t> last(g.n_cols, -1);
  for (uint32_t r = 0; r < g.n_rows; r++) {
    int64_t want = 0;
    for (uint32_t e = g.row_ptr[r]; e < g.row_ptr[r + 1]; e++) want = std::max(want, last[g.edge_col[e]] + 1);
    REQUIRE(int64_t(level_of[r]) == want);
    for (uint32_t e = g.row_ptr[r]; e < g.row_ptr[r + 1]; e++) last[g.edge_col[e]] = level_of[r];
  }
  // row records of the register-resident level kernels: every row of a level with records, in level order, with its
  // first edge, degree and variables, padded with the last variable to the level's record size
  {
    const LevelRecs lr = build_level_recs(lv, g.row_ptr, g.edge_col);
    REQUIRE(lr.rec_ptr.size() == n_levels);
    size_t expect = 0;
    for (size_t l = 0; l < n_levels; l++) {
      if (lv.maxdeg[l] > kLevelRecLong) {
        REQUIRE(lr.rec_ptr[l] == kNoLevelRecs);
        continue;
      }
      const uint32_t stride = lv.maxdeg[l] <= kLevelRecShort ? 16u : 32u;
      REQUIRE(lr.rec_ptr[l] == expect && lr.rec_ptr[l] % 16 == 0);
      for (uint32_t k = lv.level_ptr[l]; k < lv.level_ptr[l + 1]; k++) {
        const uint32_t r = lv.rows[k], e0 = g.row_ptr[r], d = g.row_ptr[r + 1] - e0;
        REQUIRE(expect + stride <= lr.words.size());
        const uint32_t *rec = &lr.words[expect];
        REQUIRE(rec[0] == e0 && rec[1] == d && d + 2 <= stride);
        for (uint32_t i = 0; i + 2 < stride; i++) REQUIRE(rec[2 + i] == (d ? g.edge_col[e0 + std::min(i, d - 1)] : 0u));
        expect += stride;
      }
    }
    REQUIRE(lr.words.size() == std::max<size_t>(expect, 16));
  }
  std::printf("%s: %u rows, %zu levels: ok\n", path, g.n_rows, n_levels);
  return 0;
}

int main(int argc, char **argv) {
  for (int i = 1; i < argc; i++)
    if (check(argv[i])) return 1;
  std::printf("slice tasks driver: ok\n");
  return 0;
}
