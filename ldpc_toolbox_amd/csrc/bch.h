// Binary BCH outer code (the DVB-S2 outer code, EN 302 307-1 5.3.1), for the ldpc_toolbox_bch_* entries of the C ABI.
//
// GF(2^m) is built from a primitive polynomial P with alpha = x.  g(x) is the least common multiple of the minimal
// polynomials of alpha^1, alpha^3, ..., alpha^(2t-1) (equal ones taken once), parity = deg g, k = n - parity: the
// narrow-sense code of length 2^m - 1, shortened to n by dropping high-order message positions.
// Bytes hold one bit each (on input a byte equal to 1 is a one, anything else a zero); byte i of a row of n is the
// coefficient of x^(n-1-i), so the first message bit is the highest power.
//   encoder   c(x) = x^parity m(x) + (x^parity m(x) mod g(x)): the message, then the remainder.
//   decoder   bounded distance: the codeword within Hamming distance t of the input if there is one (errors = that
//             distance), else the normalised input unchanged and errors = -1.
//
// This header is pure host code plus the functions the kernels and a CPU driver both compile (BCH_FN): the shift
// register of the remainder, the syndromes of a remainder, the locator (binary Berlekamp-Massey) and the root search.
// How the kernels (kernels_bch.hip.h) use them:
//   * a frame's bits are cut into runs of 32 * W bits, one per lane, the frame's LAST bit at the end of the last run
//     (zeros in front).  A lane leaves run(x) * x^parity mod g in a left-aligned register of NW words (rem_step), and
//     the runs are combined through a table of x^(offset + i) mod g (Geometry, remainder_table).
//   * the decoder's remainder is R' = r(x) x^parity mod g; R' = 0 exactly for a codeword, and r(alpha^j) =
//     R'(alpha^j) alpha^(-j parity) (syndrome_of_remainder).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define BCH_FN __host__ __device__ __forceinline__
#define BCH_UNROLL _Pragma("unroll")
#else
#define BCH_FN inline
#define BCH_UNROLL
#endif

namespace ldpc {
namespace bch {

constexpr uint32_t kMaxT = 12;        // the locator holds 13 coefficients
constexpr uint32_t kMaxM = 16;
constexpr uint32_t kMaxParityWords = 6;  // deg g <= 16 * 12 = 192 bits
constexpr uint32_t kThreads = 256;    // lanes of a frame's workgroup
constexpr uint32_t kNoLog = 0xFFFFu;  // "log of zero" (a log is at most 2^16 - 2)

// ---- what host and device both run --------------------------------------------------------------------------------

// x mod (2^m - 1), any x: the digits of x in base 2^m are summed until one is left (two rounds for the products of
// an index below 24 with a field exponent that the callers form)
BCH_FN uint32_t mod_order(uint32_t x, uint32_t m) {
  const uint32_t order = (1u << m) - 1u;
  while (x > order) x = (x & order) + (x >> m);
  return x == order ? 0u : x;
}

// a * b in GF(2^m), P = poly (bit i = coefficient of x^i, bit m set)
BCH_FN uint32_t gf_mul(uint32_t a, uint32_t b, uint32_t poly, uint32_t m) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < m; i++) {
    r ^= (0u - ((b >> i) & 1u)) & a;
    a <<= 1;
    a ^= (0u - ((a >> m) & 1u)) & poly;
  }
  return r;
}

// One step of the division by g on a register of NW words, left-aligned (the coefficient of x^(parity-1) in the top
// bit of s[NW-1]; g_top = g without its leading term, shifted the same way): s <- (s * x + bit * x^parity) mod g.
template <int NW>
BCH_FN void rem_step(uint32_t (&s)[NW], const uint32_t (&g_top)[NW], uint32_t bit) {
  const uint32_t fb = 0u - ((s[NW - 1] >> 31) ^ bit);
  BCH_UNROLL
  for (int w = NW - 1; w > 0; w--) s[w] = ((s[w] << 1) | (s[w - 1] >> 31)) ^ (fb & g_top[w]);
  s[0] = (s[0] << 1) ^ (fb & g_top[0]);
}

// r(alpha^j) from R' = r(x) x^parity mod g (bit i of rem = coefficient of x^i; words of 32 bits):
// sum over the set bits of alpha^(j (i - parity)).  antilog: alpha^e for e in [0, 2^m - 1).
BCH_FN uint32_t syndrome_of_remainder(const uint32_t *rem, uint32_t parity, uint32_t j, uint32_t m, const uint16_t *antilog) {
  const uint32_t order = (1u << m) - 1u;
  const uint32_t back = order - mod_order(parity, m);  // -parity mod order, in 1..order
  uint32_t s = 0;
  for (uint32_t i = 0; i < parity; i++)
    if ((rem[i >> 5] >> (i & 31)) & 1u) s ^= antilog[mod_order(j * mod_order(i + back, m), m)];
  return s;
}

// The error locator of the odd syndromes odd[j] = S(2j+1), j < t <= 12, by the binary form of Berlekamp-Massey
// (a discrepancy is computed at every second step; the others are zero for a binary code), without inversions:
// lambda is a non-zero multiple of the locator.  Returns its length L; lambda[0..12] is exact while L <= t, and
// L > t means "more than t errors".  Every index is a compile-time constant once the loops are unrolled.
BCH_FN uint32_t locator(const uint32_t (&odd)[kMaxT], uint32_t t, uint32_t poly, uint32_t m, uint32_t (&lambda)[kMaxT + 1]) {
  uint32_t S[2 * kMaxT];  // S[e] = S(e + 1)
  BCH_UNROLL
  for (uint32_t e = 0; e < 2 * kMaxT; e++) {
    if (e % 2 == 0)
      S[e] = e / 2 < t ? odd[e / 2] : 0u;
    else
      S[e] = gf_mul(S[(e + 1) / 2 - 1], S[(e + 1) / 2 - 1], poly, m);  // S(2i) = S(i)^2
  }
  uint32_t C[kMaxT + 1], B[kMaxT + 1];  // B holds x^shift * (the last locator before a length change)
  BCH_UNROLL
  for (uint32_t i = 0; i <= kMaxT; i++) C[i] = B[i] = 0;
  C[0] = 1;
  B[1] = 1;
  uint32_t L = 0, b = 1;
  BCH_UNROLL
  for (uint32_t r = 0; r < kMaxT; r++) {
    if (r < t) {
      const uint32_t n = 2 * r;
      uint32_t d = 0;
      BCH_UNROLL
      for (uint32_t i = 0; i <= kMaxT; i++)
        if (i <= n) d ^= gf_mul(C[i], S[n - i], poly, m);
      const bool grow = d != 0 && 2 * L <= n;
      uint32_t next[kMaxT + 1];
      BCH_UNROLL
      for (uint32_t i = 0; i <= kMaxT; i++) next[i] = d != 0 ? (gf_mul(b, C[i], poly, m) ^ gf_mul(d, B[i], poly, m)) : C[i];
      // B <- x^2 * (the old C when the length changes, else B)
      BCH_UNROLL
      for (uint32_t i = kMaxT; i >= 2; i--) B[i] = grow ? C[i - 2] : B[i - 2];
      B[0] = B[1] = 0;
      if (grow) {
        L = n + 1 - L;
        b = d;
      }
      BCH_UNROLL
      for (uint32_t i = 0; i <= kMaxT; i++) C[i] = next[i];
    }
  }
  BCH_UNROLL
  for (uint32_t i = 0; i <= kMaxT; i++) lambda[i] = C[i];
  return L;
}

// lambda(alpha^(-p)) == 0, the coefficients given as logs (kNoLog for a zero one); antilog2 covers [0, 2 * order)
BCH_FN bool is_root(const uint16_t (&loglambda)[kMaxT + 1], uint32_t p, uint32_t m, const uint16_t *antilog2) {
  const uint32_t order = (1u << m) - 1u;
  uint32_t v = 0;
  BCH_UNROLL
  for (uint32_t i = 0; i <= kMaxT; i++)
    if (loglambda[i] != kNoLog) v ^= antilog2[loglambda[i] + order - mod_order(i * p, m)];
  return v == 0;
}

// ---- host ---------------------------------------------------------------------------------------------------------

struct Code {
  uint32_t m = 0, poly = 0, t = 0, n = 0, k = 0, parity = 0;
  std::vector<uint8_t> g;         // g_0 .. g_parity
  std::vector<uint16_t> antilog;  // alpha^e, e in [0, 2 * order): the second half repeats the first
  std::vector<uint16_t> log;      // log[v], v in [1, 2^m); log[0] = kNoLog
  uint32_t order() const { return (1u << m) - 1u; }
  uint32_t parity_words() const { return (parity + 31) / 32; }
};

// (n, t) of the 21 DVB-S2 names of ldpc_toolbox_code_alist (EN 302 307-1 Tables 5a and 5b).  n is the LDPC code's k --
// except that the library's "dvbs2:R3_4short" follows the reference's m() and has k = 1080 where the standard, and this
// table, have 11880: that pair cannot be chained, and the length checks of the entries refuse it.
struct Dvbs2Entry {
  const char *name;
  uint32_t n, t;
};
inline const Dvbs2Entry *dvbs2_entries(size_t *count) {
  static const Dvbs2Entry e[] = {
      {"R1_4", 16200, 12},      {"R1_3", 21600, 12},      {"R2_5", 25920, 12},      {"R1_2", 32400, 12},
      {"R3_5", 38880, 12},      {"R2_3", 43200, 10},      {"R3_4", 48600, 12},      {"R4_5", 51840, 12},
      {"R5_6", 54000, 10},      {"R8_9", 57600, 8},       {"R9_10", 58320, 8},      {"R1_4short", 3240, 12},
      {"R1_3short", 5400, 12},  {"R2_5short", 6480, 12},  {"R1_2short", 7200, 12},  {"R3_5short", 9720, 12},
      {"R2_3short", 10800, 12}, {"R3_4short", 11880, 12}, {"R4_5short", 12600, 12}, {"R5_6short", 13320, 12},
      {"R8_9short", 14400, 12}};
  *count = sizeof(e) / sizeof(e[0]);
  return e;
}

// the field's tables; false when P has another degree than m or x has not order 2^m - 1
inline bool build_field(uint32_t m, uint32_t poly, Code *c) {
  if (m < 4 || m > kMaxM || (poly >> m) != 1u) return false;
  const uint32_t order = (1u << m) - 1u;
  c->m = m;
  c->poly = poly;
  c->antilog.assign(2 * size_t(order), 0);
  c->log.assign(size_t(order) + 1, static_cast<uint16_t>(kNoLog));
  uint32_t v = 1;
  for (uint32_t e = 0; e < order; e++) {
    if (c->log[v] != kNoLog) return false;  // back at an earlier power before 2^m - 1 steps (v == 0 included: log[0] is set below)
    if (v == 0) return false;
    c->log[v] = static_cast<uint16_t>(e);
    c->antilog[e] = c->antilog[e + order] = static_cast<uint16_t>(v);
    v <<= 1;
    if (v >> m) v ^= poly;
  }
  return v == 1;
}

// g = lcm of the minimal polynomials of alpha^1, alpha^3, ..., alpha^(2t-1); minimal (when given) gets each of them in
// the order of first appearance, as bit masks
inline void build_generator(Code *c, std::vector<uint32_t> *minimal = nullptr) {
  const uint32_t order = c->order(), m = c->m;
  auto mul = [&](uint32_t a, uint32_t b) -> uint32_t {
    return (a && b) ? c->antilog[uint32_t(c->log[a]) + c->log[b]] : 0u;
  };
  std::vector<uint8_t> seen(order, 0);
  std::vector<uint8_t> g{1};
  for (uint32_t j = 0; j < c->t; j++) {
    const uint32_t e0 = (2 * j + 1) % order;
    if (seen[e0]) continue;  // a conjugate of an earlier root: the same minimal polynomial
    std::vector<uint32_t> mp{1};  // product of (x + alpha^e) over the coset, coefficients in the field
    for (uint32_t e = e0; !seen[e]; e = mod_order(2 * e, m)) {
      seen[e] = 1;
      const uint32_t root = c->antilog[e];
      std::vector<uint32_t> next(mp.size() + 1, 0);
      for (size_t i = 0; i < mp.size(); i++) {
        next[i + 1] ^= mp[i];
        next[i] ^= mul(mp[i], root);
      }
      mp.swap(next);
    }
    uint32_t mask = 0;
    for (size_t i = 0; i < mp.size(); i++) mask |= (mp[i] & 1u) << i;  // (the coefficients are 0 or 1)
    if (minimal) minimal->push_back(mask);
    std::vector<uint8_t> next(g.size() + mp.size() - 1, 0);
    for (size_t i = 0; i < g.size(); i++)
      for (size_t q = 0; q < mp.size(); q++) next[i + q] ^= g[i] & static_cast<uint8_t>(mp[q] & 1u);
    g.swap(next);
  }
  c->g = g;
  c->parity = static_cast<uint32_t>(g.size() - 1);
}

inline bool parse_u32(const std::string &s, int base, uint32_t *out) {
  if (s.empty() || s.size() > 9) return false;
  for (char ch : s) {
    const bool digit = ch >= '0' && ch <= '9';
    const bool hex = base == 16 && ((ch >= 'a' && ch <= 'f') || (ch >= 'A' && ch <= 'F'));
    if (!digit && !hex) return false;
  }
  const unsigned long long v = std::strtoull(s.c_str(), nullptr, base);
  if (v > 0xFFFFFFFFull) return false;
  *out = static_cast<uint32_t>(v);
  return true;
}

// "dvbs2:NAME" or "bch:M:P:T:N" (P in hex) -> the code; false and *err when the spec is refused
inline bool parse_spec(const std::string &spec, Code *c, std::string *err) {
  *c = Code();
  uint32_t m = 0, poly = 0, t = 0, n = 0;
  if (spec.rfind("dvbs2:", 0) == 0) {
    const std::string name = spec.substr(6);
    size_t count = 0;
    const Dvbs2Entry *e = dvbs2_entries(&count);
    size_t i = 0;
    while (i < count && name != e[i].name) i++;
    if (i == count) {
      *err = "unknown DVB-S2 code name";
      return false;
    }
    const bool is_short = name.size() > 5 && name.compare(name.size() - 5, 5, "short") == 0;
    m = is_short ? 14 : 16;
    poly = is_short ? 0x402Bu : 0x1002Du;
    t = e[i].t;
    n = e[i].n;
  } else if (spec.rfind("bch:", 0) == 0) {
    std::vector<std::string> f;
    size_t at = 4;
    while (true) {
      const size_t colon = spec.find(':', at);
      f.push_back(spec.substr(at, colon == std::string::npos ? std::string::npos : colon - at));
      if (colon == std::string::npos) break;
      at = colon + 1;
    }
    if (f.size() != 4 || !parse_u32(f[0], 10, &m) || !parse_u32(f[1], 16, &poly) || !parse_u32(f[2], 10, &t) ||
        !parse_u32(f[3], 10, &n)) {
      *err = "malformed BCH spec (expected bch:M:P:T:N with P in hex)";
      return false;
    }
  } else {
    *err = "unknown BCH spec (expected dvbs2:NAME or bch:M:P:T:N)";
    return false;
  }
  if (m < 4 || m > kMaxM) {
    *err = "M must be 4..16";
    return false;
  }
  if ((poly >> m) != 1u) {
    *err = "the degree of P is not M";
    return false;
  }
  if (!build_field(m, poly, c)) {
    *err = "P is not primitive (x has not order 2^M - 1)";
    return false;
  }
  const uint32_t order = c->order();
  if (t < 1) {
    *err = "T must be at least 1";
    return false;
  }
  if (2ull * t >= order) {
    *err = "2T must be less than 2^M - 1";
    return false;
  }
  if (t > kMaxT) {
    *err = "T above 12 is not supported (the locator holds 13 coefficients)";
    return false;
  }
  if (n > order) {
    *err = "N exceeds 2^M - 1";
    return false;
  }
  c->t = t;
  c->n = n;
  build_generator(c);
  if (n < c->parity + 1) {
    *err = "N leaves no message bit (N - deg g < 1)";
    return false;
  }
  c->k = n - c->parity;
  return true;
}

// What a run call must satisfy before the GPU is touched (nullptr), or why it does not.
inline const char *bch_argument_error(const Code &c, bool decode, size_t output_len, size_t input_len) {
  if (!decode) {
    if (input_len != c.k) return "input_len is not the code's k";
    if (output_len != c.n) return "output_len is not the code's n";
    return nullptr;
  }
  if (input_len != c.n) return "input_len is not the code's n";
  if (output_len != c.k && output_len != c.n) return "output_len is neither the code's k nor its n";
  return nullptr;
}

// How the `bits` bits of a frame are spread over a workgroup: runs of `run_words` 32-bit words, `lanes` of them, the
// frame's last bit being the last bit of the last run (pad zero bits in front).  run_words is odd: neighbouring lanes
// then read different LDS banks.
struct Geometry {
  uint32_t bits = 0, run_words = 1, lanes = 1, pad = 0, staged_words = 0;
};
inline Geometry geometry(uint32_t bits) {
  Geometry g;
  g.bits = bits;
  const uint32_t words = (bits + 31) / 32;
  g.run_words = ((words + kThreads - 1) / kThreads) | 1u;
  g.lanes = (words + g.run_words - 1) / g.run_words;
  const uint32_t total = g.lanes * g.run_words * 32;
  g.pad = total - bits;
  g.staged_words = (total + kThreads - 1) / kThreads * kThreads / 32;  // what the staging loop writes
  return g;
}
constexpr uint32_t kMaxStagedWords = 2080;  // geometry(65535).staged_words = 2056

// table[(i * NW + w) * lanes + lane] = word w of x^(offset(lane) + i) mod g, i < parity, offset(lane) = the power of
// the lane's last bit = (lanes - 1 - lane) * 32 * run_words
inline std::vector<uint32_t> remainder_table(const Code &c, const Geometry &geo) {
  const uint32_t nw = c.parity_words(), parity = c.parity;
  std::vector<uint32_t> table(size_t(parity) * nw * geo.lanes, 0);
  std::vector<uint32_t> g_low(nw, 0), v(nw, 0);
  for (uint32_t i = 0; i < parity; i++) g_low[i >> 5] |= uint32_t(c.g[i]) << (i & 31);
  // x^0 mod g (parity >= 1, so 1 is reduced -- unless parity bits cannot hold it, which cannot happen)
  v[0] = 1;
  const uint32_t top = parity - 1;
  const uint32_t run_bits = 32 * geo.run_words;
  const uint64_t last = uint64_t(geo.lanes - 1) * run_bits + parity;  // powers 0 .. last - 1 are needed
  for (uint64_t e = 0; e < last; e++) {
    const uint64_t lane_from_end = e / run_bits;
    // x^e belongs to lane (lanes-1-q) at i = e - q * run_bits for every q with 0 <= i < parity
    for (uint64_t q = lane_from_end + 1; q-- > 0;) {
      const uint64_t i = e - q * run_bits;
      if (i >= parity) break;
      if (q >= geo.lanes) continue;
      const uint32_t lane = geo.lanes - 1 - static_cast<uint32_t>(q);
      for (uint32_t w = 0; w < nw; w++) table[(size_t(i) * nw + w) * geo.lanes + lane] = v[w];
    }
    const uint32_t carry = (v[top >> 5] >> (top & 31)) & 1u;
    v[top >> 5] &= ~(1u << (top & 31));
    for (uint32_t w = nw; w-- > 1;) v[w] = (v[w] << 1) | (v[w - 1] >> 31);
    v[0] <<= 1;
    if (carry)
      for (uint32_t w = 0; w < nw; w++) v[w] ^= g_low[w];
  }
  return table;
}

// g without its leading term, left-aligned in nw words (rem_step)
inline void generator_top(const Code &c, uint32_t *g_top) {
  const uint32_t nw = c.parity_words(), shift = 32 * nw - c.parity;
  for (uint32_t w = 0; w < kMaxParityWords; w++) g_top[w] = 0;
  for (uint32_t i = 0; i < c.parity; i++)
    if (c.g[i]) g_top[(i + shift) >> 5] |= 1u << ((i + shift) & 31);
}

}  // namespace bch
}  // namespace ldpc
