// 5G NR rate matching and rate recovery for one LDPC code block (TS 38.212 5.4.2): the host logic, and the index
// arithmetic the kernels of kernels_nr_rm.hip.h run per element.  Plain C++ (no HIP needed):
// tests/nr_rate_match_driver.cpp compiles this header alone under ASan/UBSan and checks it against the standard's loop.
//
// The definition every layer follows.  A code block configuration is (BG, Zc, F, Ncb); a transmission is (E, rv, Qm).
//   n = 68 Zc (BG1) or 52 Zc (BG2): the columns of "nr5g:BG:ZC";  K = 22 Zc or 10 Zc;  N = n - 2 Zc.
//   Column c of the codeword is buffer bit d = c - 2 Zc; the columns c < 2 Zc are never transmitted.
//   Fillers: the F columns K-F .. K-1 (buffer bits fs .. fs+F-1, fs = K - 2 Zc - F) are NULL; 0 <= F <= K - 2 Zc.
//   Ncb: 1 <= Ncb <= N (N = no limited-buffer rate matching).  L = the non-NULL bits among buffer bits 0 .. Ncb-1, L >= 1.
//   k0 = floor(a Ncb / N) Zc with a = 0, 17, 33, 56 (BG1) or 0, 13, 25, 43 (BG2) for rv 0..3.
//   Bit selection:  k = j = 0; while k < E: d = (k0 + j) mod Ncb; if d is not NULL: e[k++] = d; j++.
//   Interleaver:    f[i + q Qm] = e[i (E / Qm) + q], i < Qm, q < E / Qm; Qm in 1..8 divides E.
//   f is the transmitted order: the output of match and the rx of recover.
// Closed forms instead of the loop.  cnt(x) = x - clamp(x - fs, 0, F) is the number of non-NULL bits below x, so
// L = cnt(Ncb); the selection rank of a non-NULL buffer bit d < Ncb is r = (cnt(d) - cnt(k0)) mod L -- also when k0 lies
// inside the filler run, where cnt(k0) = fs -- and d is carried by the selection indices r, r + L, r + 2L, ... < E.
// Selection index j sits at transmitted position (j mod (E/Qm)) Qm + j div (E/Qm).
#pragma once
#include <cstdint>

#include "fast_div.h"

namespace ldpc {
namespace nrrm {

using dev::FastDiv;

constexpr uint32_t kMaxE = 0x7fffffffu;  // fdiv_q is exact below 2^31

struct Config {
  uint32_t bg = 0, zc = 0, fillers = 0, ncb = 0;
  // derived: codeword columns, information columns, circular buffer N, first filler bit fs, non-NULL bits L
  uint32_t n = 0, k = 0, nbuf = 0, fs = 0, l = 0;
};

// non-NULL buffer bits below x (x <= N)
__host__ __device__ LDPC_FD_INLINE uint32_t count_below(uint32_t x, uint32_t fs, uint32_t fillers) {
  const uint32_t over = x > fs ? x - fs : 0;
  return x - (over < fillers ? over : fillers);
}

// nullptr and *c filled, or why (bg, zc, fillers, ncb) is no configuration.  ncb < 0: N.  That zc is one of the 51
// lifting sizes is the caller's check (codes::nr5g_set_index); here 1 <= zc <= 384.
inline const char *make_config(int64_t bg, int64_t zc, int64_t fillers, int64_t ncb, Config *c) {
  if (bg != 1 && bg != 2) return "base graph must be 1 or 2";
  if (zc < 1 || zc > 384) return "lifting size out of range";
  Config r;
  r.bg = static_cast<uint32_t>(bg);
  r.zc = static_cast<uint32_t>(zc);
  r.n = (bg == 1 ? 68u : 52u) * r.zc;
  r.k = (bg == 1 ? 22u : 10u) * r.zc;
  r.nbuf = r.n - 2 * r.zc;
  if (fillers < 0 || fillers > int64_t(r.k - 2 * r.zc)) return "filler bits must be 0 .. K - 2 Zc";
  r.fillers = static_cast<uint32_t>(fillers);
  r.fs = r.k - 2 * r.zc - r.fillers;
  if (ncb < 0) ncb = r.nbuf;
  if (ncb < 1 || ncb > int64_t(r.nbuf)) return "Ncb must be 1 .. N";
  r.ncb = static_cast<uint32_t>(ncb);
  r.l = count_below(r.ncb, r.fs, r.fillers);
  if (r.l < 1) return "the circular buffer holds filler bits only";
  *c = r;
  return nullptr;
}

// k0 of redundancy version rv (TS 38.212 Table 5.4.2.1-2)
inline uint32_t k0_of(const Config &c, uint32_t rv) {
  static const uint32_t a[2][4] = {{0, 17, 33, 56}, {0, 13, 25, 43}};
  return static_cast<uint32_t>(uint64_t(a[c.bg - 1][rv & 3]) * c.ncb / c.nbuf) * c.zc;
}

// nullptr, or why (e, rv, qm) is no transmission
inline const char *transmission_error(uint64_t e, uint32_t rv, uint32_t qm) {
  if (rv > 3) return "rv must be 0 .. 3";
  if (qm < 1 || qm > 8) return "Qm must be 1 .. 8";
  if (e < 1) return "E must be positive";
  if (e > kMaxE) return "E above 0x7fffffff";
  if (e % qm != 0) return "Qm must divide E";
  return nullptr;
}

// what the kernels get: one transmission of one configuration
struct Plan {
  uint32_t n, two_zc, fs, fillers, ncb, l;
  uint32_t e, qm, cols;  // cols = E / Qm
  uint32_t c0;           // cnt(k0)
  uint32_t k0;
  FastDiv div_l, div_cols, div_qm;
};

// (e, rv, qm) accepted by transmission_error
inline Plan make_plan(const Config &c, uint32_t e, uint32_t rv, uint32_t qm) {
  Plan p;
  p.n = c.n;
  p.two_zc = 2 * c.zc;
  p.fs = c.fs;
  p.fillers = c.fillers;
  p.ncb = c.ncb;
  p.l = c.l;
  p.e = e;
  p.qm = qm;
  p.cols = e / qm;
  p.k0 = k0_of(c, rv);
  p.c0 = count_below(p.k0, c.fs, c.fillers);
  p.div_l = dev::fast_div(p.l);
  p.div_cols = dev::fast_div(p.cols);
  p.div_qm = dev::fast_div(qm);
  return p;
}

// transmitted position of selection index j < E
__host__ __device__ LDPC_FD_INLINE uint32_t position_of_selection(const Plan &p, uint32_t j) {
  const uint32_t i = dev::fdiv_q(j, p.div_cols);
  return (j - i * p.cols) * p.qm + i;
}

// selection index of transmitted position pos < E
__host__ __device__ LDPC_FD_INLINE uint32_t selection_of_position(const Plan &p, uint32_t pos) {
  const uint32_t q = dev::fdiv_q(pos, p.div_qm);
  return (pos - q * p.qm) * p.cols + q;
}

// codeword column that selection index j < E carries
__host__ __device__ LDPC_FD_INLINE uint32_t column_of_selection(const Plan &p, uint32_t j) {
  uint32_t o = j - dev::fdiv_q(j, p.div_l) * p.l + p.c0;  // ordinal among the non-NULL bits of the buffer
  if (o >= p.l) o -= p.l;
  return (o < p.fs ? o : o + p.fillers) + p.two_zc;
}

// the transmit side's mapping: codeword column of transmitted position pos < E
__host__ __device__ LDPC_FD_INLINE uint32_t column_of_position(const Plan &p, uint32_t pos) {
  return column_of_selection(p, selection_of_position(p, pos));
}

enum ColumnKind : uint32_t { kFiller = 0xffffffffu, kNotSent = 0xfffffffeu };

// the receive side's mapping: the first selection index r that carries column c < n (the others are r + L, r + 2L, ...
// below E; r >= E: none this transmission), or kFiller, or kNotSent for a column outside the circular buffer
__host__ __device__ LDPC_FD_INLINE uint32_t first_selection_of_column(const Plan &p, uint32_t c) {
  if (c < p.two_zc) return kNotSent;
  const uint32_t d = c - p.two_zc;
  if (d >= p.fs && d - p.fs < p.fillers) return kFiller;
  if (d >= p.ncb) return kNotSent;
  const uint32_t cd = count_below(d, p.fs, p.fillers);
  return cd >= p.c0 ? cd - p.c0 : cd + p.l - p.c0;
}

// nullptr, or why a match / recover call is refused: the row lengths, the transmission, and (recover) the filler LLR
inline const char *match_argument_error(const Config &c, uint64_t n, uint64_t e, uint32_t rv, uint32_t qm) {
  if (n != c.n) return "codeword length is not the code's n";
  return transmission_error(e, rv, qm);
}
inline const char *recover_argument_error(const Config &c, uint64_t n, uint64_t e, uint32_t rv, uint32_t qm, double filler_llr) {
  if (const char *why = match_argument_error(c, n, e, rv, qm)) return why;
  if (!(filler_llr > 0.0)) return "filler LLR must be positive (+inf allowed)";  // (a NaN fails the comparison)
  return nullptr;
}

}  // namespace nrrm
}  // namespace ldpc
