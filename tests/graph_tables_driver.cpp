// CPU check of the decoder's graph tables (csrc/graph_tables.h), built under ASan/UBSan for the alist files given on the
// command line and for a hand-made matrix with an empty row, a degree-1 variable and a variable in no row.  An argument
// "near:<file>" / "far:<file>" also states whether the code's degree-2 variables join neighbouring rows (rec_prefers).
// Every invariant is derived from the CSR form alone:
//  * keep / free split: keep_var and free_var partition the variables, each in increasing order, with their edges in
//    cols[v] order; the aux words of a degree-2 variable's edges point at each other and exactly one is the writer;
//  * peer words: a keep edge's word holds its position in keep_edge; a free edge's word and every free_rs entry hold
//    (row << 6) | slot of the edge they name;
//  * sliced tables: perm and inv are inverse bijections, col at every edge id is perm[edge_col], vedge lists the edge ids of
//    a variable's edges in col_ptr order, a slice is as wide as its largest degree;
//  * lane packing: no row is split over two 64-lane chunks, lane_info is slot | degree << 8 | chunk max degree << 16, every
//    level closes its chunk, and in flooding form var_lane lists each variable's edges' lanes in col_ptr order.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "../ldpc_toolbox_amd/csrc/graph_tables.h"

using namespace ldpc;
using Csr = SparseMatrix::Csr;

#define REQUIRE(c)                                                                   \
  do {                                                                               \
    if (!(c)) {                                                                      \
      std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, name); \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

// edge -> row << 6 | slot
static std::vector<uint32_t> row_slots(const Csr &g) {
  std::vector<uint32_t> rs(g.n_edges);
  for (uint32_t r = 0; r < g.n_rows; r++)
    for (uint32_t e = g.row_ptr[r]; e < g.row_ptr[r + 1]; e++) rs[e] = (r << 6) | (e - g.row_ptr[r]);
  return rs;
}

static int check_lfree(const char *name, const Csr &g, const LfreeTables &t) {
  REQUIRE(t.aux.size() == std::max<uint32_t>(g.n_edges, 1));
  REQUIRE(t.keep_ptr.size() == t.keep_var.size() + 1 && t.free_ptr.size() == t.free_var.size() + 1);
  REQUIRE(t.keep_var.size() + t.free_var.size() == g.n_cols);
  size_t ik = 0, ifr = 0;
  std::vector<bool> edge_seen(g.n_edges, false);
  for (uint32_t v = 0; v < g.n_cols; v++) {  // the merge of the two increasing lists is 0, 1, 2, ...
    const uint32_t s0 = g.col_ptr[v], dv = g.col_ptr[v + 1] - s0;
    const bool is_free = dv == 1 || dv == 2;
    const auto &var = is_free ? t.free_var : t.keep_var;
    const auto &ptr = is_free ? t.free_ptr : t.keep_ptr;
    const auto &edge = is_free ? t.free_edge : t.keep_edge;
    size_t &i = is_free ? ifr : ik;
    REQUIRE(i < var.size() && var[i] == v);
    REQUIRE(ptr[i + 1] - ptr[i] == dv && ptr[i + 1] <= edge.size());
    for (uint32_t j = 0; j < dv; j++) {
      const uint32_t e = g.col_edge[s0 + j];
      REQUIRE(edge[ptr[i] + j] == e && !edge_seen[e]);
      edge_seen[e] = true;
      if (!is_free) REQUIRE(t.aux[e] == dev::kAuxNone);
    }
    if (dv == 1) REQUIRE(t.aux[g.col_edge[s0]] == (dev::kAuxSingle | dev::kAuxWriter));
    if (dv == 2) {
      const uint32_t a = g.col_edge[s0], b = g.col_edge[s0 + 1];
      REQUIRE((t.aux[a] & dev::kAuxMask) == b && (t.aux[b] & dev::kAuxMask) == a);
      REQUIRE(((t.aux[a] & dev::kAuxWriter) != 0) != ((t.aux[b] & dev::kAuxWriter) != 0));
    }
    i++;
  }
  REQUIRE(t.keep_ptr[0] == 0 && t.free_ptr[0] == 0 && t.keep_ptr.back() == t.keep_edge.size() && t.free_ptr.back() == t.free_edge.size());
  REQUIRE(t.keep_edge.size() + t.free_edge.size() == g.n_edges);
  REQUIRE(t.ready == (!t.keep_var.empty() && !t.free_var.empty() && g.n_edges < dev::kAuxSingle));
  if (t.ready) REQUIRE(t.n_keep == t.keep_var.size() && t.n_free == t.free_var.size() && t.post_rows_keep == t.keep_var.back() + 1);
  return 0;
}

static int check_row_records(const char *name, const Csr &g, const LfreeTables &lf, bool f64, int expect_prefers) {
  const RowRecordTables t = build_row_record_tables(g, lf, f64);
  REQUIRE(t.ready == (lf.ready && g.max_row_weight <= (f64 ? 64u : 32u) && g.n_rows < dev::kPeerSingle));
  if (!t.ready) return 0;
  const std::vector<uint32_t> rs = row_slots(g);
  REQUIRE(t.peer.size() == std::max<uint32_t>(g.n_edges, 1) + kTablePad && t.keep_pos.size() == lf.keep_edge.size());
  for (size_t k = g.n_edges; k < t.peer.size(); k++) REQUIRE(t.peer[k] == dev::kPeerKeep);
  for (size_t j = 0; j < lf.keep_edge.size(); j++)
    REQUIRE(t.peer[lf.keep_edge[j]] == (dev::kPeerKeep | j) && t.keep_pos[j] == j);
  REQUIRE(t.free_rs.size() == 2 * lf.free_var.size());
  size_t near_peers = 0, far_peers = 0;
  for (size_t i = 0; i < lf.free_var.size(); i++) {
    const uint32_t v = lf.free_var[i], s0 = g.col_ptr[v], dv = g.col_ptr[v + 1] - s0, a = g.col_edge[s0];
    REQUIRE(t.free_rs[2 * i] == rs[a]);
    if (dv == 1) {
      REQUIRE(t.free_rs[2 * i + 1] == dev::kAuxNone && t.peer[a] == (dev::kPeerWriter | (dev::kPeerSingle << 6)));
      continue;
    }
    const uint32_t b = g.col_edge[s0 + 1];
    REQUIRE(t.free_rs[2 * i + 1] == rs[b]);
    REQUIRE(t.peer[a] == (dev::kPeerWriter | rs[b]) && t.peer[b] == rs[a]);  // each names the OTHER edge's row and slot
    const uint32_t ra = rs[a] >> 6, rb = rs[b] >> 6;
    ((ra + 1 == rb || rb + 1 == ra) ? near_peers : far_peers)++;
  }
  REQUIRE(t.rec_prefers == (far_peers * 4 <= near_peers + far_peers));
  if (expect_prefers >= 0) REQUIRE(t.rec_prefers == (expect_prefers != 0));
  REQUIRE(t.rec_w == (g.max_row_weight <= (f64 ? 58u : 26u) ? 3u : 4u));
  return 0;
}

static int check_sliced(const char *name, const Csr &g) {
  const SlicedTables t = build_sliced_tables(g);
  REQUIRE(t.ready == (g.max_row_weight <= 64 && g.n_rows > 0 && uint64_t(g.max_row_weight) * (g.n_rows + 64) < (1ull << 30) &&
                      uint64_t(g.max_col_weight) * (g.n_cols + 64) < (1ull << 30)));
  if (!t.ready) return 0;
  const uint32_t n = g.n_cols, m = g.n_rows, n_rs = (m + 63) / 64, n_vs = (n + 63) / 64;
  REQUIRE(t.perm.size() == n && t.inv.size() == n);
  for (uint32_t v = 0; v < n; v++) REQUIRE(t.perm[v] < n && t.inv[t.perm[v]] == v);
  for (uint32_t k = 0; k < n; k++) REQUIRE(t.inv[k] < n && t.perm[t.inv[k]] == k);
  // rows in the order of their first variable (an empty row last), ties in row order
  std::vector<uint32_t> order(m), pos(m);
  for (uint32_t r = 0; r < m; r++) order[r] = r;
  auto first_var = [&](uint32_t r) { return g.row_ptr[r] < g.row_ptr[r + 1] ? g.edge_col[g.row_ptr[r]] : 0xFFFFFFFFu; };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return first_var(a) < first_var(b); });
  for (uint32_t p = 0; p < m; p++) pos[order[p]] = p;
  REQUIRE(t.rslice_ptr.size() == n_rs + 1 && t.rdeg.size() == size_t(n_rs) * 64 && t.rslice_ptr[0] == 0);
  REQUIRE(t.vslice_ptr.size() == n_vs + 1 && t.vdeg.size() == size_t(n_vs) * 64 && t.vslice_ptr[0] == 0);
  for (uint32_t sl = 0; sl < n_rs; sl++) {
    uint32_t width = 0;
    for (uint32_t p = sl * 64; p < sl * 64 + 64; p++) {
      REQUIRE(t.rdeg[p] == (p < m ? g.row_ptr[order[p] + 1] - g.row_ptr[order[p]] : 0u));
      width = std::max(width, t.rdeg[p]);
    }
    REQUIRE(t.rslice_ptr[sl + 1] - t.rslice_ptr[sl] == width * 64);
  }
  for (uint32_t sl = 0; sl < n_vs; sl++) {
    uint32_t width = 0;
    for (uint32_t k = sl * 64; k < sl * 64 + 64; k++) {
      REQUIRE(t.vdeg[k] == (k < n ? g.col_ptr[t.inv[k] + 1] - g.col_ptr[t.inv[k]] : 0u));
      width = std::max(width, t.vdeg[k]);
    }
    REQUIRE(t.vslice_ptr[sl + 1] - t.vslice_ptr[sl] == width * 64);
  }
  REQUIRE(t.col.size() == size_t(t.rslice_ptr.back()) + 8 * 64 && t.vedge.size() == size_t(t.vslice_ptr.back()) + 8 * 64);
  std::vector<uint32_t> id_of(g.n_edges);
  for (uint32_t r = 0; r < m; r++)
    for (uint32_t e = g.row_ptr[r]; e < g.row_ptr[r + 1]; e++) {
      id_of[e] = t.rslice_ptr[pos[r] / 64] + (e - g.row_ptr[r]) * 64 + pos[r] % 64;
      REQUIRE(id_of[e] < t.rslice_ptr[pos[r] / 64 + 1]);
      REQUIRE(t.col[id_of[e]] == t.perm[g.edge_col[e]]);
    }
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t v = t.inv[k];
    for (uint32_t c = g.col_ptr[v]; c < g.col_ptr[v + 1]; c++) {
      const size_t at = t.vslice_ptr[k / 64] + size_t(c - g.col_ptr[v]) * 64 + k % 64;
      REQUIRE(at < t.vslice_ptr[k / 64 + 1] && t.vedge[at] == id_of[g.col_edge[c]]);
    }
  }
  return 0;
}

static int check_edge_lanes(const char *name, const Csr &g, const LevelTables *levels) {
  const EdgeLaneTables t = build_edge_lane_tables(g, levels);
  REQUIRE(t.ready == (g.max_row_weight <= 64 && g.n_rows > 0));
  if (!t.ready) return 0;
  REQUIRE(t.layered == (levels != nullptr));
  REQUIRE(t.lane_var.size() % 64 == 0 && t.lane_info.size() == t.lane_var.size() && t.n_chunks == t.lane_var.size() / 64);
  // the rows in the order they must appear, and the level each one closes
  LevelTables one;
  if (!levels) {
    one.level_ptr = {0u, g.n_rows};
    one.rows.resize(g.n_rows);
    for (uint32_t r = 0; r < g.n_rows; r++) one.rows[r] = r;
    levels = &one;
  }
  const size_t n_levels = levels->level_ptr.size() - 1;
  REQUIRE(t.level_chunk.size() == n_levels + 1 && t.level_chunk[0] == 0 && t.level_chunk.back() == t.n_chunks);
  std::vector<uint32_t> lane_of(g.n_edges);
  size_t lane = 0;
  for (size_t l = 0; l < n_levels; l++) {
    REQUIRE(lane == size_t(t.level_chunk[l]) * 64);  // the level before closed its chunk
    for (uint32_t idx = levels->level_ptr[l]; idx < levels->level_ptr[l + 1]; idx++) {
      const uint32_t r = levels->rows[idx], e0 = g.row_ptr[r], d = g.row_ptr[r + 1] - e0;
      if (d == 0) continue;
      if (lane < t.lane_var.size() && t.lane_var[lane] == dev::kNoLane) {  // padding: only up to the chunk's end
        while (lane < t.lane_var.size() && t.lane_var[lane] == dev::kNoLane) lane++;
        REQUIRE(lane % 64 == 0);
      }
      REQUIRE(lane + d <= t.lane_var.size() && lane / 64 == (lane + d - 1) / 64);    // the row is whole inside one chunk
      REQUIRE(lane / 64 < t.level_chunk[l + 1]);
      for (uint32_t i = 0; i < d; i++, lane++) {
        REQUIRE(t.lane_var[lane] == g.edge_col[e0 + i] && (t.lane_info[lane] & 0xFFFFu) == (i | (d << 8)));
        lane_of[e0 + i] = static_cast<uint32_t>(lane);
      }
    }
    while (lane % 64 != 0) {
      REQUIRE(t.lane_var[lane] == dev::kNoLane);
      lane++;
    }
    REQUIRE(lane == size_t(t.level_chunk[l + 1]) * 64);
  }
  REQUIRE(lane == t.lane_var.size());
  for (size_t c = 0; c < t.n_chunks; c++) {
    uint32_t dmax = 0;
    for (size_t k = c * 64; k < c * 64 + 64; k++)
      if (t.lane_var[k] != dev::kNoLane) dmax = std::max(dmax, (t.lane_info[k] >> 8) & 0xFFu);
    REQUIRE(dmax > 0);  // no chunk is empty
    for (size_t k = c * 64; k < c * 64 + 64; k++) {
      REQUIRE(t.lane_info[k] >> 16 == dmax);
      if (t.lane_var[k] == dev::kNoLane) REQUIRE((t.lane_info[k] & 0xFFFFu) == 0);
    }
  }
  if (t.layered) {
    REQUIRE(t.var_ptr.empty() && t.var_lane.empty());
  } else {
    REQUIRE(t.var_ptr == g.col_ptr && t.var_lane.size() == std::max<uint32_t>(g.n_edges, 1));
    for (uint32_t j = 0; j < g.n_edges; j++) REQUIRE(t.var_lane[j] == lane_of[g.col_edge[j]]);
  }
  return 0;
}

static int check_depuncture(const char *name, size_t n) {
  REQUIRE(!build_depuncture_map({0, 0}, 2 * n).ready);        // keeps nothing
  REQUIRE(!build_depuncture_map({1, 1, 0}, 3 * n + 1).ready);  // does not divide the length
  const DepunctureMap t = build_depuncture_map({1, 0, 1, 1, 0}, 5 * n);
  REQUIRE(t.ready && t.input_len == 3 * n && t.src_block == (std::vector<int32_t>{0, -1, 1, 2, -1}));
  return 0;
}

static int check(const char *name, const SparseMatrix &h, int expect_prefers) {
  const Csr g = h.csr();
  const LfreeTables lf = build_lfree_tables(g);
  if (check_lfree(name, g, lf)) return 1;
  for (bool f64 : {false, true})
    if (check_row_records(name, g, lf, f64, expect_prefers)) return 1;
  if (check_sliced(name, g)) return 1;
  const LevelTables lv = build_levels(g.row_ptr, g.edge_col, g.n_rows, g.n_cols);
  if (check_edge_lanes(name, g, nullptr) || check_edge_lanes(name, g, &lv)) return 1;
  if (check_depuncture(name, g.n_cols)) return 1;
  std::printf("%s: %u rows, %u columns, %u edges, %zu keep / %zu free variables: ok\n", name, g.n_rows, g.n_cols, g.n_edges,
              lf.keep_var.size(), lf.free_var.size());
  return 0;
}

int main(int argc, char **argv) {
  for (int i = 1; i < argc; i++) {
    const char *path = argv[i];
    int expect_prefers = -1;
    if (std::strncmp(path, "near:", 5) == 0) expect_prefers = 1, path += 5;
    if (std::strncmp(path, "far:", 4) == 0) expect_prefers = 0, path += 4;
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
    if (check(path, h, expect_prefers)) return 1;
  }
  // rows {0,1,2}, {1,2,3,4}, {} and {0,2,4,5}: variable 2 has degree 3, variables 3 and 5 degree 1, variable 6 is in no row
  SparseMatrix hand(4, 7);
  const int ones[][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {1, 3}, {1, 4}, {3, 0}, {3, 2}, {3, 4}, {3, 5}};
  for (const auto &rc : ones) hand.insert(rc[0], rc[1]);
  if (check("hand-made", hand, -1)) return 1;
  std::printf("graph tables driver: ok\n");
  return 0;
}
