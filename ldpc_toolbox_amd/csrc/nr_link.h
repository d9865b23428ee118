// The 5G NR shared-channel link of one configuration: what the ldpc_toolbox_nr_link_* entries (include/ldpc_toolbox.h,
// PART 11) derive from their spec, what they refuse, and the index arithmetic the fused rate-recovery kernel of
// kernels_nr_link.hip.h runs per element.  Plain C++ (no HIP needed): tests/nr_link_driver.cpp compiles this header
// alone under ASan/UBSan and checks it against literal loops.
//
// The definition every layer follows.  A configuration is (BG, A, G, QM, NL); q = QM NL.
//   (C, K', Zc, K, F, n) are those of the transport block (BG, A) (nr_transport_block.h); the C code blocks are codewords
//   of "nr5g:BG:ZC", rate-matched by "nr5g:BG:ZC:F" (nr_rate_match.h) with the call's rv and QM.
//   (e_lo, e_hi, c_lo) = block_lengths(G, q): blocks 0 .. c_lo-1 carry e_lo bits, the others e_hi; a transmission is
//   G / QM symbols.  Block r of a transport block begins at position start(r) = r e_lo + max(r - c_lo, 0) (e_hi - e_lo)
//   of the transport block's row of G demapper LLRs (TS 38.212 5.5: the blocks one after the other).
//   The HARQ state is `slots` transport blocks.  Slot rows are block-major over the slots: row r * slots + slot is block
//   r of the slot -- the rows of one block index are contiguous.
// The fused recover kernel runs over the elements (transport block, block, column) of a call, column fastest, in passes
// of at most pass_elements elements that may begin and end anywhere inside a transport block.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <initializer_list>
#include <string>

#include "fast_div.h"
#include "nr_rate_match.h"
#include "nr_transport_block.h"
#include "soft_i8.h"

namespace ldpc {
namespace nrlink {

// elements of a pass of the fused recover kernel: with a transport block's C n <= 152 * 26112 on top, the kernel's
// indices stay below 2^31
constexpr uint64_t kPassElements = uint64_t(1) << 30;
// what a host entry stages on the device at a time: about this many bytes of a transport block's longest side
constexpr uint64_t kStageBytes = uint64_t(1) << 28;

struct Config {
  nrtb::Config tb;
  nrrm::Config rm;
  nrtb::Lengths len;  // (G, e_lo, e_hi, c_lo)
  uint32_t qm = 0, layers = 1, q = 0, symbols = 0;
};

// "nr5g-link:BG:A:G:QM[:NL]", decimal fields and nothing else: nullptr and v[0..4] filled (NL = 1 when absent), or why not
inline const char *parse_fields(const std::string &spec, int64_t v[5]) {
  static const char *kForm = "invalid link spec (expected nr5g-link:BG:A:G:QM[:NL])";
  const std::string prefix = "nr5g-link:";
  if (spec.compare(0, prefix.size(), prefix) != 0) return kForm;
  v[4] = 1;
  size_t at = prefix.size(), field = 0;
  for (;; field++) {
    if (field == 5) return kForm;
    const size_t end = spec.find(':', at);
    const std::string t = spec.substr(at, end == std::string::npos ? std::string::npos : end - at);
    if (t.empty() || t.size() > 10 || t.find_first_not_of("0123456789") != std::string::npos) return kForm;
    v[field] = std::strtoll(t.c_str(), nullptr, 10);
    if (end == std::string::npos) break;
    at = end + 1;
  }
  return field >= 3 ? nullptr : kForm;
}

// nullptr and *out filled, or why (bg, a, g, qm, nl) is no configuration: what the transport block, the block lengths,
// the rate matcher with each of the two lengths, or the modulation would refuse.  That Zc is a lifting size follows from
// the transport block's choice of it.
inline const char *make_config(int64_t bg, int64_t a, int64_t g, int64_t qm, int64_t nl, Config *out) {
  Config c;
  if (const char *why = nrtb::make_config(bg, a, &c.tb)) return why;
  if (qm != 2 && qm != 4 && qm != 6 && qm != 8) return "QM must be 2, 4, 6 or 8";
  if (nl < 1 || nl > 4) return "NL must be 1 .. 4";
  c.qm = static_cast<uint32_t>(qm);
  c.layers = static_cast<uint32_t>(nl);
  c.q = c.qm * c.layers;
  if (g < 0) return "G must be 1 .. 0x7fffffff";
  if (const char *why = nrtb::make_lengths(c.tb, static_cast<uint64_t>(g), c.q, &c.len)) return why;
  if (const char *why = nrrm::make_config(c.tb.bg, c.tb.zc, c.tb.fillers, -1, &c.rm)) return why;
  for (uint32_t e : {c.len.e_lo, c.len.e_hi})
    if (const char *why = nrrm::transmission_error(e, 0, c.qm)) return why;
  c.symbols = c.len.g / c.qm;
  *out = c;
  return nullptr;
}

inline const char *parse_spec(const std::string &spec, Config *out) {
  int64_t v[5];
  if (const char *why = parse_fields(spec, v)) return why;
  return make_config(v[0], v[1], v[2], v[3], v[4], out);
}

// E_r, and where block r < C begins in a transport block's row of G
inline uint32_t block_length(const Config &c, uint32_t r) { return r < c.len.c_lo ? c.len.e_lo : c.len.e_hi; }
inline uint32_t block_start(const Config &c, uint32_t r) {
  return r * c.len.e_lo + (r > c.len.c_lo ? (r - c.len.c_lo) * (c.len.e_hi - c.len.e_lo) : 0);
}

// nullptr, or why a call is refused (before the GPU is touched)
inline const char *filler_llr_error(double v) { return v > 0.0 ? nullptr : "filler LLR must be positive (+inf allowed)"; }
inline const char *c_init_error(int64_t c_init) {
  return c_init >= -1 && c_init <= 0x7fffffffll ? nullptr : "c_init must be -1 (no scrambling) or 0 .. 2^31 - 1";
}
inline const char *slots_error(uint64_t first_slot, uint64_t batch, uint64_t slots) {
  return first_slot <= slots && batch <= slots - first_slot ? nullptr : "first_slot + batch is above the handle's slots";
}
inline const char *transmit_argument_error(const Config &c, uint64_t symbols_len, uint64_t a, uint32_t rv, int64_t c_init) {
  if (a != c.tb.a) return "payload length is not the handle's A";
  if (symbols_len != c.symbols) return "symbols_len is not the handle's G / QM";
  if (rv > 3) return "rv must be 0 .. 3";
  return c_init_error(c_init);
}
// csi: a scale per symbol is given, and noise_sigma is not read
inline const char *receive_argument_error(const Config &c, uint64_t symbols_len, uint64_t a, uint32_t rv, int64_t c_init, bool csi,
                                          double noise_sigma, uint64_t first_slot, uint64_t batch, uint64_t slots) {
  if (const char *why = transmit_argument_error(c, symbols_len, a, rv, c_init)) return why;
  if (!csi && !(std::isfinite(noise_sigma) && noise_sigma > 0.0)) return "noise_sigma must be finite and greater than 0";
  return slots_error(first_slot, batch, slots);
}
inline const char *pass_elements_error(int64_t v) {
  return v >= 1 && uint64_t(v) <= kPassElements ? nullptr : "pass_elements must be 1 .. 2^30";
}


// ---- the 8-bit mode (include/ldpc_toolbox.h, PART 12): "soft_bits" 8, one byte per soft bit from the demapper to the decoder ----

// the filler soft bit of an 8-bit handle, Q(filler_llr): 127 for +inf and for 20.0
inline int filler_soft_bit(double filler_llr) { return soft::soft_quantize(filler_llr); }
inline const char *filler_soft_bit_error(double filler_llr) {
  return filler_soft_bit(filler_llr) != 0 ? nullptr : "the filler LLR quantises to the soft bit 0 (an 8-bit handle needs 8 * filler_llr >= 0.5)";
}
// nullptr, or why "soft_bits" cannot become `value`; implementation_i8: the handle's implementation is one of the 8-bit
// names; device_state: the slots exist
inline const char *soft_bits_error(int64_t value, int64_t current, bool implementation_i8, double filler_llr, bool device_state) {
  if (value != 8 && value != 32) return "soft_bits must be 8 or 32";
  if (value == current) return nullptr;
  if (value == 8 && !implementation_i8) return "soft_bits 8 needs one of the 8-bit implementations";
  if (value == 8)
    if (const char *why = filler_soft_bit_error(filler_llr)) return why;
  if (device_state) return "soft_bits is chosen before the first batched call: the HARQ slots exist";
  return nullptr;
}
// bytes of the slots' soft rows
inline uint64_t soft_bytes(const Config &c, uint64_t slots, uint32_t soft_bits) {
  return uint64_t(c.tb.c) * slots * c.tb.n * (soft_bits / 8);
}
// A pass of the 8-bit recover kernel is a whole number of dwords: pass_elements rounded down to a multiple of 4, and 4
// below that.  C n is a multiple of 4, so every such pass begins and ends on a dword of a soft row.
inline uint64_t dword_pass_elements(uint64_t pass_elements) { return pass_elements < 4 ? 4 : pass_elements / 4 * 4; }

// One pass of the fused recover kernel: elements first .. first + total - 1 of the call's [batch][C][n], as
// (tb0, within): element i of the pass is x = within + i < 2^31 elements behind the beginning of transport block tb0.
struct Pass {
  uint64_t tb0;
  uint32_t within, total;
};
inline Pass make_pass(const Config &c, uint64_t first, uint64_t count) {
  const uint64_t per_tb = uint64_t(c.tb.c) * c.tb.n;
  return Pass{first / per_tb, static_cast<uint32_t>(first % per_tb), static_cast<uint32_t>(count)};
}

// what the kernel gets beside the two rate matcher plans
struct Geometry {
  uint32_t c, n, per_tb, c_lo, e_lo, e_hi, g;  // per_tb = C n
  dev::FastDiv div_per_tb, div_n;
};
inline Geometry make_geometry(const Config &c) {
  Geometry k;
  k.c = c.tb.c;
  k.n = c.tb.n;
  k.per_tb = c.tb.c * c.tb.n;
  k.c_lo = c.len.c_lo;
  k.e_lo = c.len.e_lo;
  k.e_hi = c.len.e_hi;
  k.g = c.len.g;
  k.div_per_tb = dev::fast_div(k.per_tb);
  k.div_n = dev::fast_div(k.n);
  return k;
}

// element x < 2^31 behind the beginning of a transport block -> (transport blocks further on, block r, column)
struct Element {
  uint32_t tb, r, column;
};
__host__ __device__ LDPC_FD_INLINE Element element_of(const Geometry &k, uint32_t x) {
  Element e;
  e.tb = dev::fdiv_q(x, k.div_per_tb);
  const uint32_t y = x - e.tb * k.per_tb;
  e.r = dev::fdiv_q(y, k.div_n);
  e.column = y - e.r * k.n;
  return e;
}
// where block r begins in a transport block's row of G (block_start)
__host__ __device__ LDPC_FD_INLINE uint32_t start_of_block(const Geometry &k, uint32_t r) {
  return r * k.e_lo + (r > k.c_lo ? (r - k.c_lo) * (k.e_hi - k.e_lo) : 0);
}

}  // namespace nrlink
}  // namespace ldpc
