// CPU check of the row shapes of the flooding record kernel (csrc/graph_tables.h, build_row_shapes: "cn_row_shape"), built
// under ASan/UBSan.  Arguments: "<name>=<alist file>"... (a name that starts with dvbs2:R1_2 is held to that code's bounds); the
// built-in dvbs2:R1_2 tables, whose rows are not sorted by column, are always checked last.  Every expectation
// is derived here from the CSR form alone, without the peer words the builder reads:
//  * the signature of every row -- kept slots at the front, then P / N / S / F / T / K per slot -- and the histogram;
//  * which rows fit the kernel's straight-line step, for both kinds: 5 kept slots, then (PN) a degree-2 variable whose other
//    edge is slot 6 of the row before, then one whose other edge is slot 5 of the row after and whose first edge this one
//    is -- or (NP) the same two the other way round, slot for slot; the tables are about the kind more rows fit;
//  * the span words against a recount, and for run lengths 1 .. 12, 16, 40 and 65536 the kernel's test of every run
//    (row_shape_run_conforms) against "every row of the run fits", with both neighbours of every row of a conforming run
//    inside the graph: no far fetch but the one of the run's first row;
//  * dvbs2:R1_2: the histogram is printed, the dominant signature must be one the kernel is built for, and at the
//    kernel's default run of 8 the rows in conforming runs, as recounted here, are at least M - 2 x (number of runs).
// Prints per code "<name>: rows M fitting F kind PN|NP|none" and "<name>: run R: runs X rows Y of Z runs first A,B,..." for the
// test to compare with its own count.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "../ldpc_toolbox_amd/csrc/codes.h"
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

struct Edge {
  uint32_t row, slot;
};

static int check(const char *name, const Csr &g, bool is_dvbs2_half) {
  is_dvbs2_half = is_dvbs2_half || std::strncmp(name, "dvbs2:R1_2", 10) == 0;  // (the same code from an alist: "dvbs2:R1_2=<file>")
  const LfreeTables lf = build_lfree_tables(g);
  const RowRecordTables rr = build_row_record_tables(g, lf, false);
  const RowShapeTables t = build_row_shapes(g, rr);
  if (!rr.ready) {
    REQUIRE(t.signature.empty() && t.span.empty() && t.fitting_rows == 0);
    std::printf("%s: no row records\n", name);
    return 0;
  }
  const uint32_t M = g.n_rows;
  REQUIRE(t.signature.size() == M && t.fits.size() == M && t.span.size() == M);
  // a variable's edges as (row, slot), in col_ptr order
  std::vector<Edge> where(g.n_edges);
  for (uint32_t r = 0; r < M; r++)
    for (uint32_t e = g.row_ptr[r]; e < g.row_ptr[r + 1]; e++) where[e] = Edge{r, e - g.row_ptr[r]};
  auto degree = [&](uint32_t v) { return g.col_ptr[v + 1] - g.col_ptr[v]; };
  std::vector<uint8_t> fits_kind[2] = {std::vector<uint8_t>(M, 0), std::vector<uint8_t>(M, 0)};  // PN, NP
  uint32_t n_kind[2] = {0, 0};
  std::map<std::string, uint32_t> hist;
  for (uint32_t c = 0; c < M; c++) {
    const uint32_t e0 = g.row_ptr[c], d = g.row_ptr[c + 1] - e0;
    uint32_t k = 0;
    while (k < d && degree(g.edge_col[e0 + k]) > 2) k++;
    std::string s = std::to_string(k) + ":";
    std::vector<uint32_t> seen;
    bool fit[2] = {k == 5 && d == 7, k == 5 && d == 7};
    for (uint32_t u = k; u < d; u++) {
      const uint32_t v = g.edge_col[e0 + u], dv = degree(v);
      char ch = 'K';
      if (dv == 1) ch = 'S';
      if (dv == 2) {
        const uint32_t ea = g.col_edge[g.col_ptr[v]], eb = g.col_edge[g.col_ptr[v] + 1];
        const bool first = ea == e0 + u;
        const Edge other = where[first ? eb : ea];
        REQUIRE(other.row != c);  // (a variable meets a row once)
        if (std::find(seen.begin(), seen.end(), other.row) != seen.end())
          ch = 'T';
        else if (other.row + 1 == c)
          ch = 'P';
        else if (other.row == c + 1)
          ch = 'N';
        else
          ch = 'F';
        seen.push_back(other.row);
        for (int kind = 0; kind < 2; kind++) {
          const uint32_t p_slot = kind == 0 ? 5 : 6, n_slot = kind == 0 ? 6 : 5;
          if (u == p_slot) fit[kind] = fit[kind] && ch == 'P' && other.slot == n_slot && !first;
          if (u == n_slot) fit[kind] = fit[kind] && ch == 'N' && other.slot == p_slot && first;
        }
      } else {
        fit[0] = fit[1] = false;
      }
      s.push_back(ch);
    }
    REQUIRE(t.signature[c] == s);
    REQUIRE(!(fit[0] && fit[1]));
    for (int kind = 0; kind < 2; kind++) {
      fits_kind[kind][c] = fit[kind];
      n_kind[kind] += fit[kind];
      if (fit[kind]) REQUIRE(c > 0 && c + 1 < M);  // both neighbours exist
    }
    hist[s]++;
  }
  const uint32_t kind = (n_kind[0] == 0 && n_kind[1] == 0) ? kRowShapeNone : (n_kind[0] >= n_kind[1] ? kRowShapePN : kRowShapeNP);
  REQUIRE(t.kind == kind);
  const std::vector<uint8_t> &fits = fits_kind[kind == kRowShapeNP ? 1 : 0];
  const uint32_t fitting = n_kind[kind == kRowShapeNP ? 1 : 0];
  for (uint32_t c = 0; c < M; c++) REQUIRE(t.fits[c] == fits[c]);
  REQUIRE(t.fitting_rows == fitting);
  uint32_t total = 0;
  for (size_t i = 0; i < t.histogram.size(); i++) {
    REQUIRE(hist.count(t.histogram[i].first) && hist[t.histogram[i].first] == t.histogram[i].second);
    if (i) REQUIRE(t.histogram[i - 1].second >= t.histogram[i].second);
    total += t.histogram[i].second;
  }
  REQUIRE(total == M && t.histogram.size() == hist.size());
  for (uint32_t c = 0; c < M; c++) {
    uint32_t up = 0, down = 0;
    while (c + up < M && fits[c + up] && up < 0xFFFFu) up++;
    while (down <= c && fits[c - down] && down < 0xFFFFu) down++;
    REQUIRE(t.span[c] == (up | (down << 16)));
  }
  std::printf("%s: rows %u fitting %u kind %s\n", name, M, fitting, kind == kRowShapePN ? "PN" : (kind == kRowShapeNP ? "NP" : "none"));
  if (is_dvbs2_half) {
    for (const auto &h : t.histogram) std::printf("%s: signature %s rows %u\n", name, h.first.c_str(), h.second);
    REQUIRE(!t.histogram.empty() && kRowShapeKept == 5);
    REQUIRE(t.histogram[0].first == (kind == kRowShapePN ? "5:PN" : "5:NP") && kind != kRowShapeNone);
  }
  const uint32_t runs_tried[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16, 40, 65536};
  for (uint32_t run : runs_tried) {
    uint32_t n_runs = 0, n_rows = 0, all_runs = 0;
    std::string first;
    for (uint32_t r = 0; uint64_t(r) * run < M; r++, all_runs++) {
      const uint32_t lo = r * run, hi = static_cast<uint32_t>(std::min<uint64_t>(uint64_t(lo) + run, M));
      bool all = hi - lo <= 0xFFFFu;  // (the counts are half-words: a longer run never conforms)
      for (uint32_t c = lo; c < hi && all; c++) all = fits[c];
      REQUIRE(row_shape_run_conforms(t.span, M, run, r) == all);
      if (all) {
        n_runs++;
        n_rows += hi - lo;
        if (n_runs <= 12) first += (first.empty() ? "" : ",") + std::to_string(r);
      }
    }
    REQUIRE(!row_shape_run_conforms(t.span, M, run, all_runs));  // (beyond the last run)
    uint32_t got_runs = 0, got_rows = 0;
    count_row_shape_runs(t.span, M, run, &got_runs, &got_rows);
    REQUIRE(got_runs == n_runs && got_rows == n_rows);
    std::printf("%s: run %u: runs %u rows %u of %u runs first %s\n", name, run, n_runs, n_rows, all_runs, first.empty() ? "-" : first.c_str());
    if (is_dvbs2_half && run == 8) REQUIRE(uint64_t(n_rows) + 2ull * all_runs >= M);
  }
  uint32_t none_runs = 1, none_rows = 1;
  count_row_shape_runs(t.span, M, 0, &none_runs, &none_rows);
  REQUIRE(none_runs == 0 && none_rows == 0);
  return 0;
}

int main(int argc, char **argv) {
  for (int i = 1; i < argc; i++) {
    const char *eq = std::strchr(argv[i], '=');
    const char *name = argv[i];
    REQUIRE(eq != nullptr);
    const std::string label(argv[i], eq - argv[i]);
    std::string err, text;
    if (FILE *f = std::fopen(eq + 1, "rb")) {
      char buf[65536];
      size_t got;
      while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got);
      std::fclose(f);
    }
    SparseMatrix h;
    if (!SparseMatrix::from_alist(text, &h, &err)) {
      std::fprintf(stderr, "%s: %s\n", argv[i], err.c_str());
      return 1;
    }
    if (check(label.c_str(), h.csr(), false)) return 1;
  }
  {
    const char *name = "builtin:dvbs2:R1_2";
    SparseMatrix h;
    REQUIRE(codes::dvbs2("R1_2", &h));
    if (check(name, h.csr(), true)) return 1;
  }
  std::printf("cn_row_shape driver: ok\n");
  return 0;
}
