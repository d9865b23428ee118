// 5G NR transport block processing around the LDPC code (TS 38.212 5.1, 5.2.2, 5.5 and the E_r of 5.4.2.1): the host
// logic, and the CRC arithmetic the kernels of kernels_nr_tb.hip.h run in registers.  Plain C++ (no HIP needed):
// tests/nr_transport_block_driver.cpp compiles this header alone under ASan/UBSan and checks it against literal loops.
//
// The definition every layer follows.  A configuration is (BG, A): base graph and payload bits.
//   L_tb = 24 (gCRC24A) if A > 3824, else 16 (gCRC16);  B = A + L_tb;  Kcb = 8448 (BG 1) or 3840 (BG 2).
//   B <= Kcb: C = 1, L_cb = 0, B' = B.  Else L_cb = 24 (gCRC24B), C = ceil(B / (Kcb - 24)), B' = B + 24 C.
//   K' = B' / C (a pair for which C does not divide B' is refused);  S = K' - L_cb is what a block takes of the B bits.
//   Kb = 22 (BG 1); BG 2: 10 if B > 640, 9 if B > 560, 8 if B > 192, else 6.  Zc = the smallest lifting size with
//   Kb Zc >= K'.  K = 22 Zc or 10 Zc, F = K - K', n = 68 Zc or 52 Zc.
//   Block r of a transport block: bits r S .. r S + S - 1 of (payload, transport block CRC), its CRC24B when C > 1, F zeros.
// CRC arithmetic.  A polynomial over GF(2) is a word, bit i = the coefficient of x^i; the first bit of a sequence is the
// highest power.  The remainder of a sequence is Horner's rule bit by bit (rem_step); the CRC of a message m is
// m(x) x^L mod g, and a sequence that ends in its own CRC has remainder zero.  A long sequence is cut into runs of 32
// bits counted from its end (run_from_end): the remainder of the whole is the XOR over the runs of
// run(x) (x^(32 w) mod g) mod g (mul_mod_word), with x^(32 w) mod g from a table (power_table).  Sequences are joined the
// same way: by x^(bits behind) mod g, from the table and j mod 32 further zero steps (shift_by_table).
#pragma once
#include <cstdint>
#include <vector>

#include "fast_div.h"

#ifdef __HIPCC__
#define LDPC_TB_INLINE __forceinline__
#else
#define LDPC_TB_INLINE inline
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace ldpc {
namespace nrtb {

constexpr uint32_t kMaxA = 1277992;  // the largest transport block of TS 38.214 5.1.3.2
constexpr uint64_t kMaxG = 0x7fffffffu;

// g(x) without its leading term, and its degree
struct Poly {
  uint32_t low, len;
};
constexpr Poly kCrc24A{0x864CFBu, 24};  // x^24 + x^23 + x^18 + x^17 + x^14 + x^11 + x^10 + x^7 + x^6 + x^5 + x^4 + x^3 + x + 1
constexpr Poly kCrc24B{0x800063u, 24};  // x^24 + x^23 + x^6 + x^5 + x + 1
constexpr Poly kCrc16{0x1021u, 16};     // x^16 + x^12 + x^5 + 1

// s(x) x + bit mod g
__host__ __device__ LDPC_TB_INLINE uint32_t rem_step(uint32_t s, uint32_t bit, Poly g) {
  const uint32_t top = (s >> (g.len - 1)) & 1u;
  return (((s << 1) | bit) & ((1u << g.len) - 1u)) ^ ((0u - top) & g.low);
}

// s(x) x^count mod g
__host__ __device__ LDPC_TB_INLINE uint32_t rem_shift(uint32_t s, uint32_t count, Poly g) {
  for (uint32_t i = 0; i < count; i++) s = rem_step(s, 0, g);
  return s;
}

// a(x) t(x) mod g; a, t of degree < g.len
__host__ __device__ LDPC_TB_INLINE uint32_t mul_mod(uint32_t a, uint32_t t, Poly g) {
  uint32_t acc = 0;
  for (uint32_t i = g.len; i-- > 0;) {
    acc = rem_step(acc, 0, g);
    acc ^= (0u - ((a >> i) & 1u)) & t;
  }
  return acc;
}

// a(x) t(x) mod g for a word a of degree < 32; t of degree < g.len
__host__ __device__ LDPC_TB_INLINE uint32_t mul_mod_word(uint32_t a, uint32_t t, Poly g) {
  uint32_t acc = 0;
  for (uint32_t i = 32; i-- > 0;) {
    acc = rem_step(acc, 0, g);
    acc ^= (0u - ((a >> i) & 1u)) & t;
  }
  return acc;
}

// Run w of a sequence of `cover` bits, counted from its end: the 32 bits that end 32 w bits before the end (32 w < cover),
// so that x^(32 w) is what lies behind them.  The run at the head is shorter and has zeros on top.  words[i] holds bits
// 32 i .. 32 i + 31 of the sequence, the first on top; words[cover / 32] may be read when no bit of it is taken.
__host__ __device__ LDPC_TB_INLINE uint32_t run_from_end(const uint32_t *words, uint32_t cover, uint32_t w) {
  const uint32_t end = cover - 32 * w;
  if (end < 32) return words[0] >> (32 - end);
  const uint32_t start = end - 32, at = start >> 5, shift = start & 31;
  return static_cast<uint32_t>((((uint64_t(words[at]) << 32) | words[at + 1]) << shift) >> 32);
}

// entry h = x^(32 h) mod g, h < entries
inline std::vector<uint32_t> power_table(Poly g, size_t entries) {
  std::vector<uint32_t> t(entries);
  uint32_t s = 1;
  for (size_t h = 0; h < entries; h++) {
    t[h] = s;
    s = rem_shift(s, 32, g);
  }
  return t;
}

// s(x) x^j mod g through a table with more than j / 32 entries
__host__ __device__ LDPC_TB_INLINE uint32_t shift_by_table(uint32_t s, uint64_t j, const uint32_t *table, Poly g) {
  return mul_mod(rem_shift(s, static_cast<uint32_t>(j & 31), g), table[j >> 5], g);
}

struct Config {
  uint32_t a = 0, bg = 0;
  // derived (the header of this file)
  uint32_t l_tb = 0, b = 0, c = 0, l_cb = 0, k_prime = 0, kb = 0, zc = 0, k = 0, fillers = 0, n = 0;
  uint32_t s = 0;  // K' - L_cb
};

inline Poly tb_poly(const Config &c) { return c.l_tb == 24 ? kCrc24A : kCrc16; }

// the smallest of the 51 lifting sizes (a 2^j <= 384, a in 2, 3, 5, 7, 9, 11, 13, 15) that is >= need; 0 = none
inline uint32_t lifting_size_at_least(uint32_t need) {
  static const uint32_t a[8] = {2, 3, 5, 7, 9, 11, 13, 15};
  uint32_t best = 0;
  for (uint32_t v : a)
    for (uint32_t z = v; z <= 384; z *= 2)
      if (z >= need && (best == 0 || z < best)) best = z;
  return best;
}

// nullptr and *out filled, or why (bg, a) is no configuration
inline const char *make_config(int64_t bg, int64_t a, Config *out) {
  if (bg != 1 && bg != 2) return "base graph must be 1 or 2";
  if (a < 1 || a > int64_t(kMaxA)) return "payload size A must be 1 .. 1277992";
  Config r;
  r.bg = static_cast<uint32_t>(bg);
  r.a = static_cast<uint32_t>(a);
  r.l_tb = r.a > 3824 ? 24 : 16;
  r.b = r.a + r.l_tb;
  const uint32_t kcb = bg == 1 ? 8448 : 3840;
  uint32_t b_prime = r.b;
  r.c = 1;
  if (r.b > kcb) {
    r.l_cb = 24;
    r.c = (r.b + kcb - 25) / (kcb - 24);
    b_prime = r.b + 24 * r.c;
  }
  if (b_prime % r.c != 0) return "the code blocks would differ in length: C does not divide B' (no transport block size of TS 38.214)";
  r.k_prime = b_prime / r.c;
  r.s = r.k_prime - r.l_cb;
  r.kb = bg == 1 ? 22 : r.b > 640 ? 10 : r.b > 560 ? 9 : r.b > 192 ? 8 : 6;
  r.zc = lifting_size_at_least((r.k_prime + r.kb - 1) / r.kb);
  if (r.zc == 0) return "no lifting size holds K'";  // (unreachable: K' <= Kcb)
  r.k = (bg == 1 ? 22u : 10u) * r.zc;
  r.fillers = r.k - r.k_prime;
  r.n = (bg == 1 ? 68u : 52u) * r.zc;
  *out = r;
  return nullptr;
}

// entries of each power table of a configuration: the exponents inside a block stay below K' + 32
inline uint32_t power_entries(const Config &c) { return c.k_prime / 32 + 2; }

// What the kernels read, in one array: x^(32 h) mod the transport block's polynomial (power_entries words), the same
// mod gCRC24B, and C words x^((C - 1 - r) S) mod the transport block's polynomial: the bits of B behind block r.
inline std::vector<uint32_t> device_tables(const Config &c) {
  const uint32_t entries = power_entries(c);
  std::vector<uint32_t> t = power_table(tb_poly(c), entries);
  const std::vector<uint32_t> cb = power_table(kCrc24B, entries);
  t.insert(t.end(), cb.begin(), cb.end());
  std::vector<uint32_t> behind(c.c);
  const uint32_t step = shift_by_table(1, c.s, t.data(), tb_poly(c));
  uint32_t v = 1;
  for (uint32_t r = c.c; r-- > 0;) {
    behind[r] = v;
    v = mul_mod(v, step, tb_poly(c));
  }
  t.insert(t.end(), behind.begin(), behind.end());
  return t;
}

// TS 38.212 7.2.2 (and 6.2.2): the base graph of payload size a at target code rate `rate`
inline int base_graph(uint64_t a, double rate) { return (a <= 292 || (a <= 3824 && rate <= 0.67) || rate <= 0.25) ? 2 : 1; }

// TS 38.212 5.4.2.1: the E_r of G coded bits over C blocks, q = N_L Qm.  nullptr, or why (g, q) is refused.
inline const char *block_lengths(const Config &c, uint64_t g, uint64_t q, uint64_t *e_lo, uint64_t *e_hi, uint64_t *c_lo) {
  if (q < 1) return "q = N_L Qm must be positive";
  if (g < 1 || g > kMaxG) return "G must be 1 .. 0x7fffffff";
  if (g % q != 0) return "q must divide G";
  const uint64_t symbols = g / q;
  if (symbols < c.c) return "G / q is below the number of code blocks";
  *c_lo = c.c - symbols % c.c;
  *e_lo = q * (symbols / c.c);
  *e_hi = q * ((symbols + c.c - 1) / c.c);
  return nullptr;
}

// what concatenate and split get: the packed block-major rows of 5.5
struct Lengths {
  uint32_t g, e_lo, e_hi, c_lo;
};

// nullptr and *l filled, or why a concatenate / split call over (g, q) is refused
inline const char *make_lengths(const Config &c, uint64_t g, uint64_t q, Lengths *l) {
  uint64_t e_lo, e_hi, c_lo;
  if (const char *why = block_lengths(c, g, q, &e_lo, &e_hi, &c_lo)) return why;
  *l = Lengths{static_cast<uint32_t>(g), static_cast<uint32_t>(e_lo), static_cast<uint32_t>(e_hi), static_cast<uint32_t>(c_lo)};
  return nullptr;
}

// One pass of concatenate / split: transport blocks b0 .. of `batch`, element index = frame * G + position < 2^31.
struct Packing {
  uint32_t g, e_lo, e_hi, lo_span;  // lo_span = c_lo e_lo: the positions of a row of G that the e_lo blocks fill
  dev::FastDiv div_g, div_lo, div_hi;
  uint64_t batch, b0, hi_base;  // hi_base = c_lo batch e_lo: where the rows of e_hi begin in the packed array
};

inline Packing make_packing(const Lengths &l, uint64_t batch, uint64_t b0) {
  Packing p;
  p.g = l.g;
  p.e_lo = l.e_lo;
  p.e_hi = l.e_hi;
  p.lo_span = l.c_lo * l.e_lo;
  p.div_g = dev::fast_div(l.g);
  p.div_lo = dev::fast_div(l.e_lo);
  p.div_hi = dev::fast_div(l.e_hi);
  p.batch = batch;
  p.b0 = b0;
  p.hi_base = uint64_t(l.c_lo) * batch * l.e_lo;
  return p;
}

// where element `idx` of the pass's [frames][G] lies in the packed block-major array
__host__ __device__ LDPC_TB_INLINE uint64_t packed_index(const Packing &p, uint32_t idx) {
  const uint32_t frame = dev::fdiv_q(idx, p.div_g);
  uint32_t pos = idx - frame * p.g;
  const uint64_t b = p.b0 + frame;
  if (pos < p.lo_span) {
    const uint32_t r = dev::fdiv_q(pos, p.div_lo);
    return (uint64_t(r) * p.batch + b) * p.e_lo + (pos - r * p.e_lo);
  }
  pos -= p.lo_span;
  const uint32_t r = dev::fdiv_q(pos, p.div_hi);
  return p.hi_base + (uint64_t(r) * p.batch + b) * p.e_hi + (pos - r * p.e_hi);
}

// nullptr, or why the row lengths of a segment / desegment call are refused
inline const char *row_lengths_error(const Config &c, uint64_t a, uint64_t k) {
  if (a != c.a) return "payload length is not the handle's A";
  if (k != c.k) return "code block length is not the handle's K";
  return nullptr;
}

// payload bits that block r carries (the last block also carries the transport block CRC)
__host__ __device__ LDPC_TB_INLINE uint32_t payload_bits_of_block(uint32_t a, uint32_t s, uint32_t r) {
  const uint64_t first = uint64_t(r) * s;
  return a - first < s ? static_cast<uint32_t>(a - first) : s;
}

}  // namespace nrtb
}  // namespace ldpc
