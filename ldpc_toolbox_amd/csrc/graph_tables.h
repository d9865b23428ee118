// Host-side graph tables of the decoder, as pure functions of the parity check matrix's CSR form: what
// DeviceDecoder::create uploads (and the small-batch paths at their first call).  No HIP here: tests/graph_tables_driver.cpp
// checks these tables on the CPU.  The layered schedule's levels and row records are in slice_tasks.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "record_flags8.h"
#include "slice_tasks.h"
#include "sparse.h"

namespace ldpc {

namespace dev {
// edge_aux[e]: kAuxNone, or for an edge whose variable is L-free: the edge id of the variable's other edge (kAuxSingle for
// degree 1), with kAuxWriter set on the variable's first slot (kernels_common.hip.h, Graph)
enum : uint32_t { kAuxNone = 0xFFFFFFFFu, kAuxWriter = 0x80000000u, kAuxSingle = 0x7FFFFFFEu, kAuxMask = 0x7FFFFFFFu };
// edge_peer[e]: see kernels_flooding.hip.h, cn_minsum_rec_kernel
enum : uint32_t { kPeerKeep = 0x80000000u, kPeerPosMask = 0x7FFFFFFFu, kPeerWriter = 0x40000000u, kPeerRowMask = 0xFFFFFFu,
                  kPeerSingle = 0xFFFFFFu };
// lane_var of a padding lane (latency_edge.hip.h)
enum : uint32_t { kNoLane = 0xFFFFFFFFu };
}  // namespace dev

// the row-record kernel fetches a row's first indices as one block of U entries -- 8, or 7 in the byte form of the flags
// (launch.hip.h, cn_rec) -- whatever the row's length: this much slack behind edge_col and peer keeps any U up to 16 in bounds
constexpr uint32_t kTablePad = 16;

// L-free variables (degree 1 or 2) of the flooding min-sum path (kernels_flooding.hip.h, cn_minsum_lfree_kernel): the
// per-edge aux word, and the variables the variable-node kernel still handles ("keep") and the L-free ones ("free") as
// compacted CSC.  ready: the graph has both kinds and its edge ids fit the aux word.
struct LfreeTables {
  bool ready = false;
  std::vector<uint32_t> aux, keep_var, keep_ptr{0}, keep_edge, free_var, free_ptr{0}, free_edge;
  uint32_t n_keep = 0, n_free = 0;
  uint32_t post_rows_keep = 0;  // posterior rows up to the last variable the variable-node kernel writes
};
inline LfreeTables build_lfree_tables(const SparseMatrix::Csr &g) {
  LfreeTables t;
  t.aux.assign(std::max<uint32_t>(g.n_edges, 1), dev::kAuxNone);
  for (uint32_t v = 0; v < g.n_cols; v++) {
    const uint32_t s0 = g.col_ptr[v], dv = g.col_ptr[v + 1] - s0;
    const bool is_free = dv == 1 || dv == 2;
    auto &lv = is_free ? t.free_var : t.keep_var;
    auto &lp = is_free ? t.free_ptr : t.keep_ptr;
    auto &le = is_free ? t.free_edge : t.keep_edge;
    lv.push_back(v);
    for (uint32_t j = 0; j < dv; j++) le.push_back(g.col_edge[s0 + j]);
    lp.push_back(static_cast<uint32_t>(le.size()));
    if (dv == 1) t.aux[g.col_edge[s0]] = dev::kAuxSingle | dev::kAuxWriter;
    if (dv == 2) {
      t.aux[g.col_edge[s0]] = g.col_edge[s0 + 1] | dev::kAuxWriter;
      t.aux[g.col_edge[s0 + 1]] = g.col_edge[s0];
    }
  }
  if (!t.free_var.empty() && !t.keep_var.empty() && g.n_edges < dev::kAuxSingle) {
    t.ready = true;
    t.n_keep = static_cast<uint32_t>(t.keep_var.size());
    t.n_free = static_cast<uint32_t>(t.free_var.size());
    t.post_rows_keep = t.keep_var.back() + 1;
  }
  return t;
}

// Row records (cn_minsum_rec_kernel): where the OTHER message of an L-free variable lives, as (row, slot).
// ready: every row fits a record's sign mask (32 / 64 bits) and the row index fits the peer word.
struct RowRecordTables {
  bool ready = false;
  std::vector<uint32_t> peer, free_rs, keep_pos;
  uint32_t rec_w = 0;        // words per record: 3, or 4 for rows too long for the packed form
  uint32_t flag_bits = 0;    // width of a record's flags word in memory: 16, 32 or 64 (record_flag_bits)
  bool rec_prefers = false;  // at most a quarter of the degree-2 variables join distant rows
};
// Width of the word that holds a row record's flip bits and argmin, from the longest row: 16 where the flip bits and the
// argmin (ceil(log2(weight)) bits, one for a single edge) fit a half-word -- rows of at most 12 edges --, else the decoder's
// own word: packed with the argmin up to 26 (f32) / 58 (f64) edges, the argmin in a fourth word beyond.  0: no record form.
inline uint32_t record_arg_bits(uint32_t max_row_weight) {
  uint32_t bits = 1;
  while ((1u << bits) < max_row_weight) bits++;
  return bits;
}
inline uint32_t record_flag_bits(uint32_t max_row_weight, bool f64) {
  const uint32_t word = f64 ? 64u : 32u;
  if (max_row_weight == 0 || max_row_weight > word) return 0;
  return max_row_weight + record_arg_bits(max_row_weight) <= 16 ? 16u : word;
}
// Bytes of that word in memory when the byte form is chosen ("flags8", device_decoder.h): 1 where the flags are a half-word
// and the flip bits and the argmin take at most 10 bits -- rows of at most 7 edges: 8 bits in a byte of their own, 2 in the
// sign bits of the stored magnitudes (record_flags8.h) --, else the width record_flag_bits names.  record_flag_bits keeps
// naming the FAMILY (16 for such rows): the byte form is a way of storing the half-word family's records.
inline uint32_t record_flag_bytes(uint32_t max_row_weight, bool f64) {
  const uint32_t bits = record_flag_bits(max_row_weight, f64);
  if (bits == 16 && max_row_weight + record_arg_bits(max_row_weight) <= 10) return 1;
  return bits / 8;
}
inline RowRecordTables build_row_record_tables(const SparseMatrix::Csr &g, const LfreeTables &lf, bool f64) {
  RowRecordTables t;
  const uint32_t rec_bits = f64 ? 64u : 32u, rec_packed = f64 ? 58u : 26u;
  if (!lf.ready || g.max_row_weight > rec_bits || g.n_rows >= dev::kPeerSingle) return t;
  std::vector<uint32_t> rs(std::max<uint32_t>(g.n_edges, 1));  // edge -> row << 6 | slot
  for (uint32_t r = 0; r < g.n_rows; r++)
    for (uint32_t e = g.row_ptr[r]; e < g.row_ptr[r + 1]; e++) rs[e] = (r << 6) | (e - g.row_ptr[r]);
  // keep edges: where the variable-node kernel reads the message (its compacted list, variable-major)
  t.peer.assign(std::max<uint32_t>(g.n_edges, 1), dev::kPeerKeep);
  t.free_rs.assign(2 * lf.free_var.size(), dev::kAuxNone);
  t.keep_pos.resize(lf.keep_edge.size());
  for (size_t j = 0; j < lf.keep_edge.size(); j++) {
    t.peer[lf.keep_edge[j]] = dev::kPeerKeep | static_cast<uint32_t>(j);
    t.keep_pos[j] = static_cast<uint32_t>(j);
  }
  // The record kernel rebuilds an L-free variable's other message from the peer row's record, which it has at hand only
  // when the peer is the row before or after (staircase codes; a degree-1 variable has no peer).  Codes whose degree-2
  // variables join distant rows (AR4JA: measured 10 % slower with records) keep per-edge messages.
  size_t far_peers = 0, near_peers = 0;
  for (size_t i = 0; i < lf.free_var.size(); i++) {
    const uint32_t v = lf.free_var[i], s0 = g.col_ptr[v], dv = g.col_ptr[v + 1] - s0;
    const uint32_t ea = g.col_edge[s0];
    t.free_rs[2 * i] = rs[ea];
    if (dv == 1) {
      t.peer[ea] = dev::kPeerWriter | (dev::kPeerSingle << 6);
      continue;
    }
    const uint32_t eb = g.col_edge[s0 + 1];
    t.peer[ea] = dev::kPeerWriter | rs[eb];
    t.peer[eb] = rs[ea];
    t.free_rs[2 * i + 1] = rs[eb];
    const uint32_t ra = rs[ea] >> 6, rb = rs[eb] >> 6;
    ((ra + 1 == rb || rb + 1 == ra) ? near_peers : far_peers) += 1;
  }
  t.rec_prefers = far_peers * 4 <= near_peers + far_peers;
  t.rec_w = g.max_row_weight <= rec_packed ? 3u : 4u;
  t.flag_bits = record_flag_bits(g.max_row_weight, f64);
  t.peer.resize(t.peer.size() + kTablePad, dev::kPeerKeep);
  t.ready = true;
  return t;
}

// ROW SHAPES ("cn_row_shape", cn_minsum_rec_kernel's SHAPE form): what the record kernel otherwise learns per row and slot
// from the peer words, as a signature per row, and which runs of the kernel's walk have a shape the kernel has
// straight-line code for.
//   * signature of a row: "<k>:" and a letter per remaining slot, k the number of kept slots at the front (peer word with
//     kPeerKeep).  P: L-free, the other edge in the row before (row order, c - 1); N: in the row after; S: single, degree 1;
//     F: far, any other row; T: twin, a second degree-2 variable on a pair of rows an earlier slot of this row already joins;
//     K: a kept slot behind an L-free one.
//   * a row FITS the straight-line step of kind "PN" (kRowShapePN) when its signature is kRowShapeKept kept slots, then P,
//     then N, AND the two peers sit where the step takes them from without a look: P's other edge in the N slot of row
//     c - 1, N's in the P slot of row c + 1, the variable's first edge (kPeerWriter) the N one.  Kind "NP" (kRowShapeNP): the
//     same with the two L-free slots the other way round.  The tables are made for ONE kind per graph, the one more rows
//     fit (ties: PN).  dvbs2:R1_2 read from its alist, as every decoder's graph is (rows sorted by column), is PN: 32 398 of
//     its 32 400 rows have the signature "5:PN" and 32 397 of them fit (row 1 sits behind the first row, "5:N", one edge
//     short), the last row is "5:PS"; the built-in tables as codes.cpp lists them, the parity bit shared with the next row
//     first, are NP: 32 398 rows "5:NP", all fitting.  At a run of 8 both leave the first and the last run to the generic step
//     (tests/cn_row_shape_driver.cpp prints both histograms).  A row with the signature may still not fit: behind a
//     shorter row, or one with a second degree-2 variable, the peer's slot is another.
constexpr uint32_t kRowShapeKept = 5;
enum : uint32_t { kRowShapeNone = 0, kRowShapePN = 1, kRowShapeNP = 2 };
struct RowShapeTables {
  // these two only `with_signatures` (the test driver, a printout): a decoder uses `kind` and `span`
  std::vector<std::string> signature;                           // per row
  std::vector<std::pair<std::string, uint32_t>> histogram;      // signature -> rows, most frequent first (ties: by name)
  uint32_t kind = kRowShapeNone;                                // the kind `fits` and `span` are about (none: no row fits either)
  std::vector<uint8_t> fits;                                    // per row
  std::vector<uint32_t> span;                                   // per row, see above
  uint32_t fitting_rows = 0;
};
inline RowShapeTables build_row_shapes(const SparseMatrix::Csr &g, const RowRecordTables &rr, bool with_signatures = true) {
  RowShapeTables t;
  if (!rr.ready) return t;
  const uint32_t M = g.n_rows;
  if (with_signatures) t.signature.resize(M);
  t.span.assign(M, 0);
  std::vector<uint8_t> fits_pn(M, 0), fits_np(M, 0);
  uint32_t n_pn = 0, n_np = 0;
  std::vector<uint32_t> seen;  // peer rows of the L-free slots so far
  std::string s;               // the row's signature (one buffer for all rows)
  for (uint32_t c = 0; c < M; c++) {
    const uint32_t e0 = g.row_ptr[c], d = g.row_ptr[c + 1] - e0;
    uint32_t k = 0;
    while (k < d && (rr.peer[e0 + k] & dev::kPeerKeep)) k++;
    s = std::to_string(k);
    s.push_back(':');
    seen.clear();
    for (uint32_t u = k; u < d; u++) {
      const uint32_t p = rr.peer[e0 + u], prow = (p >> 6) & dev::kPeerRowMask;
      char ch;
      if (p & dev::kPeerKeep)
        ch = 'K';
      else if (prow == dev::kPeerSingle)
        ch = 'S';
      else if (std::find(seen.begin(), seen.end(), prow) != seen.end())
        ch = 'T';
      else if (prow + 1 == c)
        ch = 'P';
      else if (prow == c + 1)
        ch = 'N';
      else
        ch = 'F';
      if (!(p & dev::kPeerKeep) && prow != dev::kPeerSingle) seen.push_back(prow);
      s.push_back(ch);
    }
    if (k == kRowShapeKept && d == kRowShapeKept + 2) {
      const bool pn = s.compare(s.size() - 2, 2, "PN") == 0, np = s.compare(s.size() - 2, 2, "NP") == 0;
      if (pn || np) {
        const uint32_t p_slot = pn ? kRowShapeKept : kRowShapeKept + 1, n_slot = pn ? kRowShapeKept + 1 : kRowShapeKept;
        const uint32_t pp = rr.peer[e0 + p_slot], pn_word = rr.peer[e0 + n_slot];
        const bool fit = (pp & 63u) == n_slot && (pn_word & 63u) == p_slot && !(pp & dev::kPeerWriter) && (pn_word & dev::kPeerWriter);
        (pn ? fits_pn : fits_np)[c] = fit;
        (pn ? n_pn : n_np) += fit;
      }
    }
    if (with_signatures) t.signature[c] = s;
  }
  t.kind = (n_pn == 0 && n_np == 0) ? kRowShapeNone : (n_pn >= n_np ? kRowShapePN : kRowShapeNP);
  t.fits = t.kind == kRowShapeNP ? std::move(fits_np) : std::move(fits_pn);
  t.fitting_rows = t.kind == kRowShapeNP ? n_np : n_pn;
  for (uint32_t c = M; c-- > 0;)
    if (t.fits[c]) t.span[c] = std::min<uint32_t>(0xFFFFu, 1 + (c + 1 < M ? (t.span[c + 1] & 0xFFFFu) : 0u));
  for (uint32_t c = 0; c < M; c++)
    if (t.fits[c]) t.span[c] |= std::min<uint32_t>(0xFFFFu, 1 + (c > 0 ? (t.span[c - 1] >> 16) : 0u)) << 16;
  if (!with_signatures) return t;
  std::vector<std::string> sorted = t.signature;
  std::sort(sorted.begin(), sorted.end());
  for (size_t i = 0; i < sorted.size();) {
    size_t j = i;
    while (j < sorted.size() && sorted[j] == sorted[i]) j++;
    t.histogram.emplace_back(sorted[i], static_cast<uint32_t>(j - i));
    i = j;
  }
  std::stable_sort(t.histogram.begin(), t.histogram.end(), [](const auto &a, const auto &b) { return a.second > b.second; });
  return t;
}
// the kernel's test: run r of `run` rows (rows r * run .. , the last run shorter; even runs walk upwards from their first row,
// odd ones downwards from their last) is all fitting rows
inline bool row_shape_run_conforms(const std::vector<uint32_t> &span, uint32_t n_rows, uint32_t run, uint32_t r) {
  const uint64_t lo = uint64_t(r) * run;
  if (run == 0 || lo >= n_rows) return false;
  const uint32_t hi = static_cast<uint32_t>(std::min<uint64_t>(lo + run, n_rows)), len = hi - static_cast<uint32_t>(lo);
  const uint32_t w = span[(r & 1u) ? hi - 1 : static_cast<uint32_t>(lo)];
  return ((r & 1u) ? w >> 16 : w & 0xFFFFu) >= len;
}
// runs of the walk that conform at this run length, and the rows in them
inline void count_row_shape_runs(const std::vector<uint32_t> &span, uint32_t n_rows, uint32_t run, uint32_t *runs, uint32_t *rows) {
  *runs = *rows = 0;
  if (run == 0 || span.size() < n_rows) return;
  for (uint32_t r = 0; uint64_t(r) * run < n_rows; r++)
    if (row_shape_run_conforms(span, n_rows, run, r)) {
      *runs += 1;
      *rows += static_cast<uint32_t>(std::min<uint64_t>(uint64_t(r) * run + run, n_rows) - uint64_t(r) * run);
    }
}

// The variable-node kernel's record source (kernels_flooding.hip.h, vn_kernel's record form): for every edge of the kept list, in
// the list's own order (keep_var / keep_ptr, cols[v] order inside a variable), row << 6 | slot of the edge inside its row --
// free_rs's word, with free_rs's limits: a slot below 64 and a row index below kPeerSingle, else not ready.  Padded by
// kTablePad words (the kernel fetches a variable's first indices as one block).
struct KeepRsTable {
  bool ready = false;
  std::vector<uint32_t> rs;
};
inline KeepRsTable build_keep_rs(const SparseMatrix::Csr &g, const LfreeTables &lf) {
  KeepRsTable t;
  if (!lf.ready || g.max_row_weight > 64 || g.n_rows >= dev::kPeerSingle) return t;
  std::vector<uint32_t> rs(std::max<uint32_t>(g.n_edges, 1));  // edge -> row << 6 | slot
  for (uint32_t r = 0; r < g.n_rows; r++)
    for (uint32_t e = g.row_ptr[r]; e < g.row_ptr[r + 1]; e++) rs[e] = (r << 6) | (e - g.row_ptr[r]);
  t.rs.reserve(lf.keep_edge.size() + kTablePad);
  for (uint32_t e : lf.keep_edge) t.rs.push_back(rs[e]);
  t.rs.resize(t.rs.size() + kTablePad, 0);
  t.ready = true;
  return t;
}

// The kept list in BUNDLES ("vn_bundles", run_group.hip.h): the same entries in another order.  In vn_kernel the waves of a
// workgroup that work on the same codewords sum, at every step of their loops, W consecutive list entries that start at a
// multiple of W (W = waves per workgroup / slices per tile, make_tiling); a row's record that two of them want at that step
// is fetched from beyond the L2 once.  Every entry is a sum of its own, so the order of the list is free: variables that
// share rows are put into the same aligned bundle of W entries.
//   * Greedy: the seed of a bundle is the first entry not yet placed; the bundle grows by the unplaced entry of the seed's
//     degree that shares the most rows with the entries already in it (ties: the earliest in the list); where none shares a
//     row, by the next unplaced entry of that degree, and where that degree has run out, by the next unplaced entry of any.
//     Equal degrees inside a bundle: the waves of a workgroup issue the same number of loads per step.
//   * An entry keeps its variable, its edges and their cols[v] order: the sums do not change.
//   * Deterministic; W <= 1 returns the list as it is.
// fetches / distinct: record fetches of one pass over the list (its edges), and the distinct rows per bundle, summed -- what
// is left of them when every coincident request inside a bundle is served once (count_vn_bundle_fetches: the same count of
// any list, for any W).
struct VnBundleTables {
  std::vector<uint32_t> list_var, list_ptr{0}, keep_rs;  // keep_rs padded by kTablePad words, as build_keep_rs pads it
  uint64_t fetches = 0, distinct = 0;
};
inline void count_vn_bundle_fetches(uint32_t n_keep, const std::vector<uint32_t> &list_ptr, const std::vector<uint32_t> &keep_rs,
                                    uint32_t W, uint64_t *fetches, uint64_t *distinct) {
  *fetches = 0;
  *distinct = 0;
  std::vector<uint32_t> rows;
  for (uint32_t i0 = 0; i0 < n_keep; i0 += std::max<uint32_t>(W, 1)) {
    const uint32_t i1 = std::min<uint64_t>(n_keep, uint64_t(i0) + std::max<uint32_t>(W, 1));
    rows.clear();
    for (uint32_t j = list_ptr[i0]; j < list_ptr[i1]; j++) rows.push_back(keep_rs[j] >> 6);
    *fetches += rows.size();
    std::sort(rows.begin(), rows.end());
    *distinct += static_cast<uint64_t>(std::unique(rows.begin(), rows.end()) - rows.begin());
  }
}
inline VnBundleTables build_vn_bundles(uint32_t n_keep, const std::vector<uint32_t> &keep_ptr, const std::vector<uint32_t> &keep_var,
                                       const std::vector<uint32_t> &keep_rs, uint32_t W) {
  VnBundleTables t;
  std::vector<uint32_t> order;  // new position -> old position
  order.reserve(n_keep);
  if (W <= 1) {
    for (uint32_t i = 0; i < n_keep; i++) order.push_back(i);
  } else {
    auto degree = [&](uint32_t i) { return keep_ptr[i + 1] - keep_ptr[i]; };
    // row -> the entries on it (CSR over the rows the list touches), entries in list order
    uint32_t n_rows = 0;
    for (uint32_t j = 0; j < keep_ptr[n_keep]; j++) n_rows = std::max(n_rows, (keep_rs[j] >> 6) + 1);
    std::vector<uint32_t> row_ptr(size_t(n_rows) + 1, 0), row_entry(keep_ptr[n_keep]);
    for (uint32_t j = 0; j < keep_ptr[n_keep]; j++) row_ptr[(keep_rs[j] >> 6) + 1]++;
    for (uint32_t r = 0; r < n_rows; r++) row_ptr[r + 1] += row_ptr[r];
    {
      std::vector<uint32_t> fill(row_ptr.begin(), row_ptr.end() - 1);
      for (uint32_t i = 0; i < n_keep; i++)
        for (uint32_t j = keep_ptr[i]; j < keep_ptr[i + 1]; j++) row_entry[fill[keep_rs[j] >> 6]++] = i;
    }
    std::vector<uint8_t> placed(n_keep, 0), row_in(n_rows, 0);
    std::vector<uint32_t> shared(n_keep, 0), touched, bundle_rows;
    uint32_t max_deg = 0;
    for (uint32_t i = 0; i < n_keep; i++) max_deg = std::max(max_deg, degree(i));
    std::vector<uint32_t> next_of(size_t(max_deg) + 1, 0);  // per degree: no unplaced entry of it lies before this position
    uint32_t next_any = 0;
    auto place = [&](uint32_t i) {
      placed[i] = 1;
      order.push_back(i);
      // the rows the bundle gains: every unplaced entry on them shares one more row with the bundle
      for (uint32_t j = keep_ptr[i]; j < keep_ptr[i + 1]; j++) {
        const uint32_t r = keep_rs[j] >> 6;
        if (row_in[r]) continue;
        row_in[r] = 1;
        bundle_rows.push_back(r);
        for (uint32_t k = row_ptr[r]; k < row_ptr[r + 1]; k++) {
          const uint32_t c = row_entry[k];
          if (placed[c]) continue;
          if (shared[c]++ == 0) touched.push_back(c);
        }
      }
    };
    while (order.size() < n_keep) {
      while (placed[next_any]) next_any++;
      const uint32_t seed = next_any, d = degree(seed);
      place(seed);
      for (uint32_t k = 1; k < W && order.size() < n_keep; k++) {
        uint32_t best = 0xFFFFFFFFu, best_shared = 0;
        for (uint32_t c : touched)
          if (!placed[c] && degree(c) == d && (shared[c] > best_shared || (shared[c] == best_shared && c < best))) {
            best = c;
            best_shared = shared[c];
          }
        if (best == 0xFFFFFFFFu) {
          uint32_t &nd = next_of[d];
          while (nd < n_keep && (placed[nd] || degree(nd) != d)) nd++;
          best = nd;
        }
        if (best >= n_keep) {
          while (placed[next_any]) next_any++;
          best = next_any;
        }
        place(best);
      }
      for (uint32_t c : touched) shared[c] = 0;
      for (uint32_t r : bundle_rows) row_in[r] = 0;
      touched.clear();
      bundle_rows.clear();
    }
  }
  t.list_var.reserve(n_keep);
  t.keep_rs.reserve(size_t(keep_ptr[n_keep]) + kTablePad);
  for (uint32_t i : order) {
    t.list_var.push_back(keep_var[i]);
    t.keep_rs.insert(t.keep_rs.end(), keep_rs.begin() + keep_ptr[i], keep_rs.begin() + keep_ptr[i + 1]);
    t.list_ptr.push_back(static_cast<uint32_t>(t.keep_rs.size()));
  }
  count_vn_bundle_fetches(n_keep, t.list_ptr, t.keep_rs, W, &t.fetches, &t.distinct);
  t.keep_rs.resize(t.keep_rs.size() + kTablePad, 0);
  return t;
}

// The kept list in CHAINS ("vn_chains", run_group.hip.h): the same entries in blocks of W * L.  Block position (t, w), step
// t < L and wave w < W, is list index block * W * L + t * W + w; a wave walks t = 0 .. L - 1 of its w, and where two
// consecutive entries of that walk share a row, the second takes the row's record from the wave's registers (the CARRY)
// and not from memory: a variable of a chain costs one fetch less, whatever the other waves do and whenever they do it.
// A tree of n variables shares at most n - 1 rows (girth >= 6), so a chain is as good as any cluster of its size.
//   * The order is a walk over the graph "two entries share a row": a path starts at the unplaced entry with the fewest
//     unplaced neighbours and steps to the unplaced neighbour with the fewest unplaced neighbours (ties: the earliest in
//     the list), until there is none.  The paths, one behind the other, are cut into runs of L: run number block * W + w
//     is wave w's walk of that block.  (The last block holds the R < W * L entries left: wave w walks its t * W + w < R.)
//   * keep_rs carries the two decisions in the bits its limits leave free (a row index is below kPeerSingle = 2^24):
//     kChainFrom on an edge whose record is the carry, kChainLeave on the edge whose record the entry leaves in the carry
//     for the wave's next entry.  Both on one edge: three entries in a row on the same check row, the carry stays.  Only an
//     entry's first kChainEdges edges take part: the kernel has them in flight together, so the carry is read before it is
//     replaced.  Never kChainFrom at t = 0, at most one kChainFrom and one kChainLeave per entry.
//   * An entry keeps its variable, its edges and their cols[v] order: the sums do not change.
//   * Deterministic; L <= 1 is build_vn_bundles(..., W): the same list, no flags.
// fetches: the list's edges; carried: the edges marked kChainFrom; issued: the loads a pass really issues -- per step the
// distinct rows among the W step-mates, each having dropped its carried row (count_vn_chain_fetches: of any such list).
enum : uint32_t { kChainFrom = 0x80000000u, kChainLeave = 0x40000000u, kChainRsMask = 0x3FFFFFFFu, kChainEdges = 8 };
struct VnChainTables {
  std::vector<uint32_t> list_var, list_ptr{0}, keep_rs;  // keep_rs padded by kTablePad words
  uint32_t n_blocks = 0;
  uint64_t fetches = 0, carried = 0, issued = 0;
};
inline void count_vn_chain_fetches(uint32_t n_keep, const std::vector<uint32_t> &list_ptr, const std::vector<uint32_t> &keep_rs,
                                   uint32_t W, uint32_t L, uint64_t *fetches, uint64_t *carried, uint64_t *issued) {
  *fetches = *carried = *issued = 0;
  W = std::max<uint32_t>(W, 1);
  (void)L;  // (a step's mates are W consecutive entries from a multiple of W, in a whole block and in the last one)
  std::vector<uint32_t> rows;
  for (uint32_t i0 = 0; i0 < n_keep; i0 += W) {
    const uint32_t i1 = std::min<uint64_t>(n_keep, uint64_t(i0) + W);
    rows.clear();
    for (uint32_t j = list_ptr[i0]; j < list_ptr[i1]; j++) {
      if (keep_rs[j] & kChainFrom)
        *carried += 1;
      else
        rows.push_back((keep_rs[j] & kChainRsMask) >> 6);
    }
    *fetches += list_ptr[i1] - list_ptr[i0];
    std::sort(rows.begin(), rows.end());
    *issued += static_cast<uint64_t>(std::unique(rows.begin(), rows.end()) - rows.begin());
  }
}
inline VnChainTables build_vn_chains(uint32_t n_keep, const std::vector<uint32_t> &keep_ptr, const std::vector<uint32_t> &keep_var,
                                     const std::vector<uint32_t> &keep_rs, uint32_t W, uint32_t L) {
  VnChainTables t;
  W = std::max<uint32_t>(W, 1);
  if (L <= 1) {
    VnBundleTables b = build_vn_bundles(n_keep, keep_ptr, keep_var, keep_rs, W);
    t.list_var = std::move(b.list_var);
    t.list_ptr = std::move(b.list_ptr);
    t.keep_rs = std::move(b.keep_rs);
    t.n_blocks = (n_keep + W - 1) / W;
    t.fetches = b.fetches;
    t.issued = b.distinct;
    return t;
  }
  const uint32_t kNone = 0xFFFFFFFFu;
  auto chain_deg = [&](uint32_t i) { return std::min<uint32_t>(keep_ptr[i + 1] - keep_ptr[i], kChainEdges); };
  // row -> the entries that have it among their first kChainEdges edges, in list order
  uint32_t n_rows = 0;
  for (uint32_t j = 0; j < keep_ptr[n_keep]; j++) n_rows = std::max(n_rows, (keep_rs[j] >> 6) + 1);
  std::vector<uint32_t> row_ptr(size_t(n_rows) + 1, 0);
  for (uint32_t i = 0; i < n_keep; i++)
    for (uint32_t p = 0; p < chain_deg(i); p++) row_ptr[(keep_rs[keep_ptr[i] + p] >> 6) + 1]++;
  for (uint32_t r = 0; r < n_rows; r++) row_ptr[r + 1] += row_ptr[r];
  std::vector<uint32_t> row_entry(row_ptr[n_rows]);
  {
    std::vector<uint32_t> fill(row_ptr.begin(), row_ptr.end() - 1);
    for (uint32_t i = 0; i < n_keep; i++)
      for (uint32_t p = 0; p < chain_deg(i); p++) row_entry[fill[keep_rs[keep_ptr[i] + p] >> 6]++] = i;
  }
  // unplaced neighbours of every entry (with multiplicity where two entries share more than one row), and the unplaced
  // entries ordered by that count, then by list position
  std::vector<uint32_t> free_nb(n_keep, 0);
  for (uint32_t i = 0; i < n_keep; i++)
    for (uint32_t p = 0; p < chain_deg(i); p++) {
      const uint32_t r = keep_rs[keep_ptr[i] + p] >> 6;
      free_nb[i] += row_ptr[r + 1] - row_ptr[r] - 1;
    }
  auto key = [&](uint32_t i) { return (uint64_t(free_nb[i]) << 32) | i; };
  std::vector<uint64_t> heap;  // min-heap with lazy deletion: an element counts while it matches key() of an unplaced entry
  heap.reserve(size_t(n_keep) * 2);
  for (uint32_t i = 0; i < n_keep; i++) heap.push_back(key(i));
  auto later = [](uint64_t a, uint64_t b) { return a > b; };
  std::make_heap(heap.begin(), heap.end(), later);
  std::vector<uint8_t> placed(n_keep, 0);
  std::vector<uint32_t> seq, link;  // the walk; link[k]: the row seq[k] shares with seq[k - 1] as its chain link, or kNone
  seq.reserve(n_keep);
  link.reserve(n_keep);
  auto place = [&](uint32_t i, uint32_t via) {
    placed[i] = 1;
    seq.push_back(i);
    link.push_back(via);
    for (uint32_t p = 0; p < chain_deg(i); p++) {
      const uint32_t r = keep_rs[keep_ptr[i] + p] >> 6;
      for (uint32_t k = row_ptr[r]; k < row_ptr[r + 1]; k++) {
        const uint32_t c = row_entry[k];
        if (placed[c]) continue;
        free_nb[c]--;
        heap.push_back(key(c));
        std::push_heap(heap.begin(), heap.end(), later);
      }
    }
  };
  while (seq.size() < n_keep) {
    uint32_t cur = kNone;
    while (cur == kNone) {
      const uint64_t top = heap.front();
      std::pop_heap(heap.begin(), heap.end(), later);
      heap.pop_back();
      const uint32_t i = static_cast<uint32_t>(top);
      if (!placed[i] && key(i) == top) cur = i;
    }
    place(cur, kNone);
    for (;;) {
      uint32_t best = kNone, best_row = kNone;
      for (uint32_t p = 0; p < chain_deg(cur); p++) {
        const uint32_t r = keep_rs[keep_ptr[cur] + p] >> 6;
        for (uint32_t k = row_ptr[r]; k < row_ptr[r + 1]; k++) {
          const uint32_t c = row_entry[k];
          if (placed[c]) continue;
          if (best == kNone || key(c) < key(best)) {
            best = c;
            best_row = r;
          }
        }
      }
      if (best == kNone) break;
      place(best, best_row);
      cur = best;
    }
  }
  // the runs: run s = block * W + w takes the next len(s) entries of the walk
  const uint32_t per_block = W * L;
  t.n_blocks = (n_keep + per_block - 1) / per_block;
  std::vector<uint32_t> order(n_keep, 0), from_row(n_keep, kNone), leave_row(n_keep, kNone);  // by new position
  uint32_t k = 0;
  for (uint32_t blk = 0; blk < t.n_blocks; blk++) {
    const uint32_t base = blk * per_block, room = std::min(per_block, n_keep - base);
    for (uint32_t w = 0; w < W && w < room; w++) {
      const uint32_t len = (room - w + W - 1) / W;  // t with t * W + w < room
      for (uint32_t s = 0; s < len; s++, k++) {
        const uint32_t at = base + s * W + w;
        order[at] = seq[k];
        if (s > 0 && link[k] != kNone) {
          from_row[at] = link[k];
          leave_row[at - W] = link[k];
        }
      }
    }
  }
  t.list_var.reserve(n_keep);
  t.keep_rs.reserve(size_t(keep_ptr[n_keep]) + kTablePad);
  for (uint32_t at = 0; at < n_keep; at++) {
    const uint32_t i = order[at];
    t.list_var.push_back(keep_var[i]);
    bool from_set = false, leave_set = false;
    for (uint32_t j = keep_ptr[i]; j < keep_ptr[i + 1]; j++) {
      uint32_t word = keep_rs[j];
      const uint32_t row = word >> 6;
      if (j - keep_ptr[i] < kChainEdges) {
        if (!from_set && row == from_row[at]) {
          word |= kChainFrom;
          from_set = true;
        }
        if (!leave_set && row == leave_row[at]) {
          word |= kChainLeave;
          leave_set = true;
        }
      }
      t.keep_rs.push_back(word);
    }
    t.list_ptr.push_back(static_cast<uint32_t>(t.keep_rs.size()));
  }
  count_vn_chain_fetches(n_keep, t.list_ptr, t.keep_rs, W, L, &t.fetches, &t.carried, &t.issued);
  t.keep_rs.resize(t.keep_rs.size() + kTablePad, 0);
  return t;
}

// Sliced-ELLPACK tables of the small-batch path (latency.hip.h): rows in the order of their first variable, 64 to a slice,
// slot-major inside a slice: edge (position p, slot j) -> id rslice_ptr[p / 64] + j * 64 + p % 64 (messages and `col`
// share it).  ready: rows of at most 64 edges, at least one row, and edge ids within 2^30.
struct SlicedTables {
  bool ready = false;
  std::vector<uint32_t> rslice_ptr, rdeg, col, vslice_ptr, vdeg, vedge, perm, inv;
};
inline SlicedTables build_sliced_tables(const SparseMatrix::Csr &g) {
  SlicedTables t;
  if (g.max_row_weight > 64 || g.n_rows == 0 || uint64_t(g.max_row_weight) * (g.n_rows + 64) >= (1ull << 30) ||
      uint64_t(g.max_col_weight) * (g.n_cols + 64) >= (1ull << 30))
    return t;
  std::vector<uint32_t> order(g.n_rows), pos_of_row(g.n_rows), edge_row(std::max<uint32_t>(g.n_edges, 1));
  for (uint32_t r = 0; r < g.n_rows; r++) order[r] = r;
  auto first_var = [&](uint32_t r) { return g.row_ptr[r] < g.row_ptr[r + 1] ? g.edge_col[g.row_ptr[r]] : 0xFFFFFFFFu; };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return first_var(a) < first_var(b); });
  const uint32_t n_rs = (g.n_rows + 63) / 64, n_vs = (g.n_cols + 63) / 64;
  t.rslice_ptr.assign(1, 0);
  t.rdeg.assign(size_t(n_rs) * 64, 0);
  for (uint32_t sl = 0; sl < n_rs; sl++) {
    uint32_t width = 0;
    for (uint32_t p = sl * 64; p < std::min(g.n_rows, sl * 64 + 64); p++) {
      const uint32_t r = order[p], dr = g.row_ptr[r + 1] - g.row_ptr[r];
      pos_of_row[r] = p;
      t.rdeg[p] = dr;
      width = std::max(width, dr);
    }
    t.rslice_ptr.push_back(t.rslice_ptr.back() + width * 64);
  }
  // The variables are renumbered too, in the order of their first appearance when the slots are scanned
  // slot-major over the row positions: neighbouring lanes (rows) then gather neighbouring words of the
  // soft values in EVERY slot where the code has structure -- also in DVB-S2's staircase part, whose
  // natural numbering puts the parity bits of neighbouring positions q words apart (a gather per lane) --
  // and neighbouring variables read neighbouring messages.  The per-codeword arrays (chan, post, rawhard)
  // live in this numbering; only ingest and emit translate (perm / inv).
  t.perm.assign(g.n_cols, 0xFFFFFFFFu);
  uint32_t next = 0;
  for (uint32_t j = 0; j < g.max_row_weight; j++)
    for (uint32_t p = 0; p < g.n_rows; p++) {
      const uint32_t r = order[p];
      if (j < g.row_ptr[r + 1] - g.row_ptr[r]) {
        const uint32_t v = g.edge_col[g.row_ptr[r] + j];
        if (t.perm[v] == 0xFFFFFFFFu) t.perm[v] = next++;
      }
    }
  for (uint32_t v = 0; v < g.n_cols; v++)
    if (t.perm[v] == 0xFFFFFFFFu) t.perm[v] = next++;
  t.inv.assign(g.n_cols, 0);
  for (uint32_t v = 0; v < g.n_cols; v++) t.inv[t.perm[v]] = v;
  t.col.assign(t.rslice_ptr.back() + 8 * 64, 0);  // + padding: a chunk may read past the last slice
  auto edge_id = [&](uint32_t r, uint32_t j) { return t.rslice_ptr[pos_of_row[r] / 64] + j * 64 + pos_of_row[r] % 64; };
  for (uint32_t r = 0; r < g.n_rows; r++)
    for (uint32_t e = g.row_ptr[r]; e < g.row_ptr[r + 1]; e++) {
      t.col[edge_id(r, e - g.row_ptr[r])] = t.perm[g.edge_col[e]];
      edge_row[e] = r;
    }
  t.vslice_ptr.assign(1, 0);
  t.vdeg.assign(size_t(n_vs) * 64, 0);
  for (uint32_t sl = 0; sl < n_vs; sl++) {
    uint32_t width = 0;
    for (uint32_t k = sl * 64; k < std::min(g.n_cols, sl * 64 + 64); k++) {
      const uint32_t v = t.inv[k];
      t.vdeg[k] = g.col_ptr[v + 1] - g.col_ptr[v];
      width = std::max(width, t.vdeg[k]);
    }
    t.vslice_ptr.push_back(t.vslice_ptr.back() + width * 64);
  }
  t.vedge.assign(t.vslice_ptr.back() + 8 * 64, 0);
  for (uint32_t k = 0; k < g.n_cols; k++) {
    const uint32_t v = t.inv[k];
    for (uint32_t c = g.col_ptr[v]; c < g.col_ptr[v + 1]; c++) {  // cols[v] order: the reference's sum order
      const uint32_t e = g.col_edge[c], r = edge_row[e];
      t.vedge[t.vslice_ptr[k / 64] + (c - g.col_ptr[v]) * 64 + k % 64] = edge_id(r, e - g.row_ptr[r]);
    }
  }
  t.ready = true;
  return t;
}

// Lane packing of the lane-per-edge small-batch path (latency_edge.hip.h): the rows are packed, whole, into chunks of at
// most 64 lanes (one wavefront) -- level after level for the layered schedule (levels != nullptr), all rows in order for
// flooding, which also gets the variables' edge lists (cols[v] order) as lane indices.
// lane_info: slot | degree << 8 | the chunk's largest degree << 16.  ready: rows of at most 64 edges, at least one row.
struct EdgeLaneTables {
  bool ready = false, layered = true;
  std::vector<uint32_t> level_chunk, lane_var, lane_info, var_ptr, var_lane;
  uint32_t n_chunks = 0;
};
inline EdgeLaneTables build_edge_lane_tables(const SparseMatrix::Csr &g, const LevelTables *levels) {
  EdgeLaneTables t;
  if (g.max_row_weight > 64 || g.n_rows == 0) return t;
  t.layered = levels != nullptr;
  t.level_chunk.assign(1, 0);
  std::vector<uint32_t> edge_lane(std::max<uint32_t>(g.n_edges, 1), 0);
  uint32_t fill = 0;  // lanes used in the open chunk
  auto close = [&]() {
    if (fill == 0) return;
    const size_t c0 = t.lane_var.size() - fill;
    uint32_t dmax = 0;
    for (size_t k = c0; k < c0 + fill; k++) dmax = std::max(dmax, (t.lane_info[k] >> 8) & 0xFFu);
    t.lane_var.resize(c0 + 64, dev::kNoLane);
    t.lane_info.resize(c0 + 64, 0);
    for (size_t k = c0; k < c0 + 64; k++) t.lane_info[k] |= dmax << 16;
    fill = 0;
  };
  auto add_row = [&](uint32_t r) {
    const uint32_t e0 = g.row_ptr[r], dr = g.row_ptr[r + 1] - e0;
    if (dr == 0) return;  // an empty row has no message and an even parity
    if (fill + dr > 64) close();
    for (uint32_t i = 0; i < dr; i++) {
      edge_lane[e0 + i] = static_cast<uint32_t>(t.lane_var.size());
      t.lane_var.push_back(g.edge_col[e0 + i]);
      t.lane_info.push_back(i | (dr << 8));
    }
    fill += dr;
  };
  auto close_level = [&]() {
    close();
    t.level_chunk.push_back(static_cast<uint32_t>(t.lane_var.size() / 64));
  };
  if (t.layered) {
    for (size_t l = 0; l + 1 < levels->level_ptr.size(); l++) {
      for (uint32_t idx = levels->level_ptr[l]; idx < levels->level_ptr[l + 1]; idx++) add_row(levels->rows[idx]);
      close_level();
    }
  } else {
    for (uint32_t r = 0; r < g.n_rows; r++) add_row(r);
    close_level();
    t.var_ptr.assign(g.col_ptr.begin(), g.col_ptr.end());
    t.var_lane.resize(std::max<uint32_t>(g.n_edges, 1), 0);
    for (uint32_t j = 0; j < g.n_edges; j++) t.var_lane[j] = edge_lane[g.col_edge[j]];
  }
  t.n_chunks = static_cast<uint32_t>(t.lane_var.size() / 64);
  t.ready = true;
  return t;
}

// Depuncture map of the reference's block pattern (puncturing.rs:27-40): source block of every pattern block, -1 =
// punctured.  ready: the pattern keeps something and its length divides the codeword length.
struct DepunctureMap {
  bool ready = false;
  std::vector<int32_t> src_block;
  size_t input_len = 0;  // LLRs per codeword a caller supplies
};
inline DepunctureMap build_depuncture_map(const std::vector<uint8_t> &puncturing, size_t n_cols) {
  DepunctureMap t;
  size_t trues = 0;
  for (uint8_t p : puncturing) trues += p ? 1 : 0;
  if (trues == 0 || n_cols % puncturing.size() != 0) return t;
  t.src_block.resize(puncturing.size());
  int32_t j = 0;
  for (size_t k = 0; k < puncturing.size(); k++) t.src_block[k] = puncturing[k] ? j++ : -1;
  t.input_len = n_cols / puncturing.size() * trues;
  t.ready = true;
  return t;
}

}  // namespace ldpc
