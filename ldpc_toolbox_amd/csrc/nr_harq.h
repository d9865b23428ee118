// 5G NR HARQ with incremental-redundancy soft combining for one LDPC code block: the host logic of a sequence of
// transmissions of one rate matcher configuration (nr_rate_match.h).  Plain C++ (no HIP needed):
// tests/nr_harq_driver.cpp compiles this header alone under ASan/UBSan and checks it against a literal loop.
//
// The definition every layer follows.  A sequence is T transmissions (E_t, rv_t), t < T, 1 <= T <= 8, of one Qm.
//   Each (E_t, rv_t, Qm) is a transmission of nr_rate_match.h; each E_t is a multiple of the modulation's bits per symbol;
//   sum E_t <= 0x7fffffff.
//   A frame's HARQ process is ONE long transmitted row: its T rate-matched rows, concatenated.  P_t = E_0 + ... + E_{t-1}
//   is where transmission t starts in it, and the channel puts on position P_t + j of that row the noise it puts there on
//   any row of the frame: a BPSK position g takes the normal pair g >> 1 (its first normal for even g, its second for odd
//   g), the symbol s of a modulation of M bits the pair P_t / M + s.
//   The soft buffer of a frame after transmission 0 is recover(combine = 0) of its LLRs, after each later one
//   recover(combine = 1) into the same row.
#pragma once
#include <cstdint>

#include "nr_rate_match.h"

namespace ldpc {
namespace nrharq {

constexpr uint32_t kMaxTransmissions = 8;

struct Sequence {
  uint32_t t = 0;  // 0: none
  uint32_t qm = 1;
  uint32_t e[kMaxTransmissions] = {}, rv[kMaxTransmissions] = {};
  uint32_t offset[kMaxTransmissions + 1] = {};  // P_t; offset[t] = the length of the concatenated row
};

// nullptr, or why (e, rv)[transmissions] with qm is no sequence for a modulation of bits_per_symbol bits
inline const char *sequence_error(const uint64_t *e, const uint32_t *rv, uint64_t transmissions, uint32_t qm, uint32_t bits_per_symbol) {
  if (transmissions < 1 || transmissions > kMaxTransmissions) return "a HARQ sequence has 1 .. 8 transmissions";
  if (e == nullptr || rv == nullptr) return "null E or rv array";
  if (bits_per_symbol < 1) return "the modulation has no bits";
  uint64_t sum = 0;
  for (uint64_t t = 0; t < transmissions; t++) {
    if (const char *why = nrrm::transmission_error(e[t], rv[t], qm)) return why;
    if (e[t] % bits_per_symbol != 0) return "every E must be a multiple of the modulation's bits per symbol";
    sum += e[t];  // (each term is at most 0x7fffffff, and there are at most 8)
  }
  if (sum > nrrm::kMaxE) return "the transmissions' E sum above 0x7fffffff";
  return nullptr;
}

// (e, rv, transmissions, qm) accepted by sequence_error
inline Sequence make_sequence(const uint64_t *e, const uint32_t *rv, uint32_t transmissions, uint32_t qm) {
  Sequence s;
  s.t = transmissions;
  s.qm = qm;
  for (uint32_t t = 0; t < transmissions; t++) {
    s.e[t] = static_cast<uint32_t>(e[t]);
    s.rv[t] = rv[t];
    s.offset[t + 1] = s.offset[t] + s.e[t];
  }
  return s;
}

// the rate matcher's plan of transmission t < s.t
inline nrrm::Plan plan_of(const nrrm::Config &c, const Sequence &s, uint32_t t) { return nrrm::make_plan(c, s.e[t], s.rv[t], s.qm); }

// BPSK: the normal pairs that positions [P_t, P_t + E_t) of the concatenated row touch are first_pair .. first_pair + pairs - 1;
// the first one is shared with transmission t-1 when P_t is odd, the last one with t+1 when P_t + E_t is
inline uint32_t first_pair(const Sequence &s, uint32_t t) { return s.offset[t] >> 1; }
inline uint32_t pairs(const Sequence &s, uint32_t t) { return ((s.offset[t + 1] - 1) >> 1) - (s.offset[t] >> 1) + 1; }

// a modulation of m bits per symbol (m divides every E_t, so every P_t): the pair of symbol 0 of transmission t
inline uint32_t first_symbol(const Sequence &s, uint32_t t, uint32_t m) { return s.offset[t] / m; }

}  // namespace nrharq
}  // namespace ldpc
