// Host-side tables of the layered schedule: dependency levels of the check rows and their row records.  Used by
// DeviceDecoder::create.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace ldpc {

struct LevelTables {
  std::vector<uint32_t> level_ptr;   // [n_levels + 1] into rows
  std::vector<uint32_t> rows;        // rows grouped by level, in row order inside a level
  std::vector<uint32_t> maxdeg;      // [n_levels] longest row of the level
};

// level(r) = 1 + max level of the earlier rows that share a variable with r: the rows of one level are
// variable-disjoint, so processing level after level equals the serial row order of horizontal_layered.rs:105-110
inline LevelTables build_levels(const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &edge_col, uint32_t n_rows,
                                uint32_t n_cols) {
  LevelTables t;
  std::vector<uint32_t> last(n_cols, 0), level(n_rows, 0);
  uint32_t n_levels = 0;
  for (uint32_t r = 0; r < n_rows; r++) {
    uint32_t lv = 0;
    for (uint32_t e = row_ptr[r]; e < row_ptr[r + 1]; e++) lv = std::max(lv, last[edge_col[e]]);
    lv += 1;
    level[r] = lv;
    n_levels = std::max(n_levels, lv);
    for (uint32_t e = row_ptr[r]; e < row_ptr[r + 1]; e++) last[edge_col[e]] = lv;
  }
  t.level_ptr.assign(n_levels + 1, 0);
  for (uint32_t r = 0; r < n_rows; r++) t.level_ptr[level[r]]++;
  for (uint32_t l = 1; l <= n_levels; l++) t.level_ptr[l] += t.level_ptr[l - 1];
  std::vector<uint32_t> cursor(t.level_ptr.begin(), t.level_ptr.end() - 1);
  t.rows.assign(n_rows, 0);
  for (uint32_t r = 0; r < n_rows; r++) t.rows[cursor[level[r] - 1]++] = r;
  t.maxdeg.assign(n_levels, 0);
  for (uint32_t r = 0; r < n_rows; r++)
    t.maxdeg[level[r] - 1] = std::max(t.maxdeg[level[r] - 1], row_ptr[r + 1] - row_ptr[r]);
  return t;
}

// Row records of the register-resident level kernels (kernels.hip.h, hl_level_reg_kernel): per row of a level whose
// longest row has at most 24 edges, in level order, [first edge, degree, variable of edge 0, 1, ...] padded with the
// last variable to 16 words (levels of at most 12 edges) or 32 words -- one scalar load per row instead of the chain
// level_rows -> row_ptr -> edge_col.  rec_ptr[l] = first word of level l's records (kNoLevelRecs: the level has none).
constexpr uint32_t kNoLevelRecs = 0xFFFFFFFFu;
constexpr uint32_t kLevelRecShort = 12, kLevelRecLong = 24;  // edges of a 16-word / 32-word record
struct LevelRecs {
  std::vector<uint32_t> words;
  std::vector<uint32_t> rec_ptr;  // [n_levels]
};
inline LevelRecs build_level_recs(const LevelTables &lv, const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &edge_col) {
  LevelRecs t;
  const size_t n_levels = lv.maxdeg.size();
  t.rec_ptr.assign(n_levels, kNoLevelRecs);
  for (size_t l = 0; l < n_levels; l++) {
    if (lv.maxdeg[l] > kLevelRecLong) continue;
    const uint32_t stride = lv.maxdeg[l] <= kLevelRecShort ? 16u : 32u;
    t.rec_ptr[l] = static_cast<uint32_t>(t.words.size());
    for (uint32_t idx = lv.level_ptr[l]; idx < lv.level_ptr[l + 1]; idx++) {
      const uint32_t r = lv.rows[idx], e0 = row_ptr[r], d = row_ptr[r + 1] - e0;
      const size_t base = t.words.size();
      t.words.resize(base + stride, 0);
      t.words[base] = e0;
      t.words[base + 1] = d;
      for (uint32_t i = 0; i + 2 < stride; i++) t.words[base + 2 + i] = d ? edge_col[e0 + std::min(i, d - 1)] : 0u;
    }
  }
  if (t.words.empty()) t.words.assign(16, 0);  // (an empty upload is an error)
  return t;
}

}  // namespace ldpc
