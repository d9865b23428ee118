// Kernels of the 5G NR modulation mapper, soft demapper and scrambling (nr_qam.h; include/ldpc_toolbox.h, PART 8).
// One thread per symbol, indexed by a 64-bit id; no LDS.  Compiled with -ffp-contract=off: every product and sum below is
// rounded once, as the definition says.
//
//   * gold_kernel: c(n) of 38.211 5.2.1, bit n of the sequence at bit n % 32 of word n / 32.  One thread per run of
//     kGoldRunWords words.  It reaches the two LFSR states at the start of its run by jump-ahead -- x^(1600 + start)
//     modulo each feedback polynomial, square-and-multiply over GF(2), applied to the first 61 bits of the register's
//     sequence -- and then steps the run out a word at a time.  Nothing is serial in the sequence length.
//   * map_kernel: the 2^h amplitudes are not selected from a table at all: a lane computes its integer level L_u from
//     its h bits with 38.211's nested form (h - 1 integer subtractions) and multiplies by a in f64 -- the one product
//     that defines A_u -- so there is neither LDS nor a lane-dependent index into the kernel arguments.
//   * demap_kernel<H, IO, A, MAXLOG>: per axis d_u = sx * A_u - K_u and the 2h folds over ascending u; A_u and K_u travel
//     in the kernel arguments and every index is wave-uniform (scalar loads).  The QM LLRs of a symbol leave as 8- or
//     16-byte vector stores, nontemporal on the max-log path.
//   * demap_i8_kernel<H, A, MAXLOG, WIDE>: the same arithmetic from float symbols, each LLR quantised to an 8-bit soft bit:
//     QM bytes out per symbol, the float row never stored.
//   * demap_csi_kernel<H, IO, A, MAXLOG>, demap_csi_i8_kernel<H, A, MAXLOG, WIDE>: the two demappers with a scale per symbol
//     (PART 10): one more coalesced load per lane, and K_u = (0.5 * s) * Q_u made from the symbol's own s.
//   * qam_llr_kernel<H, MAXLOG, FADING>: the simulator's generator, fused: pooled transmitted row -> symbol -> AWGN, or
//     (FADING) the Rayleigh block-fading channel -> the f64 demapper, or its per-symbol-scale form -> float.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "frame_gen.hip.h"
#include "kernels_demod.hip.h"
#include "soft_i8.h"

namespace ldpc {
namespace nrqam {

constexpr int kThreads = demod::kThreads;

// ---- the Gold sequence ------------------------------------------------------------------------------------------------

constexpr uint32_t kGoldRunWords = 32;               // a thread's run: 1024 bits of c
constexpr uint32_t kGoldPoly1 = 0x00000009u;         // x1(n+31) = x1(n+3) ^ x1(n):                      x^31 = x^3 + 1
constexpr uint32_t kGoldPoly2 = 0x0000000Fu;         // x2(n+31) = x2(n+3) ^ x2(n+2) ^ x2(n+1) ^ x2(n):  x^31 = x^3 + x^2 + x + 1
constexpr uint32_t kGoldMask31 = 0x7FFFFFFFu;

// a * b modulo x^31 + poly over GF(2): a, b of degree < 31
GEN_FN uint32_t gf2_mulmod(uint32_t a, uint32_t b, uint32_t poly) {
  uint64_t p = 0;
  for (int i = 0; i < 31; i++)
    if ((b >> i) & 1u) p ^= uint64_t(a) << i;
  for (int d = 60; d >= 31; d--)  // x^d = x^(d-31) * poly
    if ((p >> d) & 1u) p ^= (uint64_t(1) << d) ^ (uint64_t(poly) << (d - 31));
  return static_cast<uint32_t>(p);
}

// x^e modulo x^31 + poly, left-to-right square-and-multiply (the multiplication by x is a shift)
GEN_FN uint32_t gf2_xpow(uint64_t e, uint32_t poly) {
  uint32_t r = 1;
  for (int i = e ? 63 - __builtin_clzll(e) : -1; i >= 0; i--) {
    r = gf2_mulmod(r, r, poly);
    if ((e >> i) & 1u) {
      r <<= 1;
      if (r >> 31) r = (r & kGoldMask31) ^ poly;
    }
  }
  return r;
}

// the feedback of both registers reaches at most 3 positions ahead, so 28 new bits follow from 31 known ones at once
template <bool X2>
GEN_FN uint64_t gold_taps(uint64_t s) {
  return X2 ? (s >> 3) ^ (s >> 2) ^ (s >> 1) ^ s : (s >> 3) ^ s;
}

// s: bits n .. n+30 of a register's sequence at bits 0..30 -> bits n .. n+63 (two steps of 28 and of 5 new bits)
template <bool X2>
GEN_FN uint64_t gold_extend(uint64_t s) {
  s |= (gold_taps<X2>(s) & 0x0FFFFFFFull) << 31;  // bits 31..58 from bits 0..30 (+3)
  s |= (gold_taps<X2>(s) >> 28) << 59;            // bits 59..63 from bits 28..35 (+3)
  return s;
}

// bits n .. n+30 of the register's sequence from its first 61 bits: x(n+k) = sum_i r_i x(k+i), r = x^n mod the polynomial
GEN_FN uint32_t gold_state_at(uint64_t first61, uint32_t r) {
  uint32_t s = 0;
  for (int k = 0; k < 31; k++) s |= (static_cast<uint32_t>(__builtin_popcount(r & static_cast<uint32_t>(first61 >> k) & kGoldMask31)) & 1u) << k;
  return s;
}

// the first 61 bits of a register's sequence from its initial 31
template <bool X2>
GEN_FN uint64_t gold_first61(uint32_t init) {
  return gold_extend<X2>(init & kGoldMask31) & ((uint64_t(1) << 61) - 1);
}

// words [run * kGoldRunWords, ...) of c, as far as `words` reaches
GEN_FN void gold_run(uint32_t c_init, uint32_t run, uint32_t words, uint32_t *out) {
  const uint64_t start = 1600ull + uint64_t(run) * kGoldRunWords * 32u;
  uint64_t s1 = gold_state_at(gold_first61<false>(1u), gf2_xpow(start, kGoldPoly1));
  uint64_t s2 = gold_state_at(gold_first61<true>(c_init), gf2_xpow(start, kGoldPoly2));
  const uint32_t w0 = run * kGoldRunWords;
  for (uint32_t w = w0; w < w0 + kGoldRunWords && w < words; w++) {
    s1 = gold_extend<false>(s1);
    s2 = gold_extend<true>(s2);
    out[w] = static_cast<uint32_t>(s1) ^ static_cast<uint32_t>(s2);
    s1 = (s1 >> 32) & kGoldMask31;
    s2 = (s2 >> 32) & kGoldMask31;
  }
}

__global__ __launch_bounds__(kThreads) void gold_kernel(uint32_t c_init, uint32_t words, uint32_t runs, uint32_t *__restrict__ out) {
  const uint32_t run = blockIdx.x * kThreads + threadIdx.x;
  if (run >= runs) return;
  gold_run(c_init, run, words, out);
}

// the QM bits c(i0) .. c(i0 + QM - 1) at bits 0 .. QM-1; the buffer has one word beyond the last bit's, so a window that
// straddles a word boundary (QM = 6, symbol 5: bits 30..35) reads both words without a bound test
template <int QM>
__device__ __forceinline__ uint32_t gold_window(const uint32_t *__restrict__ c, uint32_t i0) {
  const uint32_t w = i0 >> 5;
  const uint64_t two = (uint64_t(c[w + 1]) << 32) | c[w];
  return static_cast<uint32_t>(two >> (i0 & 31u)) & ((1u << QM) - 1u);
}

// ---- the mapper -------------------------------------------------------------------------------------------------------

// L_u of nr_qam.h from the H bits of one axis: bit t of the axis is bit 2 t + axis of the symbol, at bit 2 t + axis of `sym_bits`
template <int H>
__device__ __forceinline__ int32_t axis_level(uint32_t sym_bits, int axis) {
  int32_t v = ((sym_bits >> (2 * (H - 1) + axis)) & 1u) ? -1 : 1;
#pragma unroll
  for (int t = H - 2; t >= 0; t--) {
    const int32_t rest = (int32_t(1) << (H - 1 - t)) - v;
    v = ((sym_bits >> (2 * t + axis)) & 1u) ? -rest : rest;
  }
  return v;
}

template <typename T>
struct Pair {
  typedef T type __attribute__((ext_vector_type(2)));
};

// bits [frames][bits_len] -> symbols [frames][bits_len / QM] (re, im); c: the scrambling sequence, or nullptr
template <int QM, typename T>
__global__ __launch_bounds__(kThreads) void map_kernel(const uint8_t *__restrict__ bits, T *__restrict__ symbols, uint32_t symbols_len,
                                                       uint64_t total, double a, const uint32_t *__restrict__ c) {
  const uint64_t id = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (id >= total) return;
  const uint8_t *b = bits + id * QM;  // (bits_len = QM * symbols_len: the rows are dense)
  uint32_t sym_bits = 0;
#pragma unroll
  for (int j = 0; j < QM; j++) sym_bits |= (b[j] == 1 ? 1u : 0u) << j;
  if (c != nullptr) {
    const uint32_t sym = static_cast<uint32_t>(id % symbols_len);
    sym_bits ^= gold_window<QM>(c, QM * sym);
  }
  typename Pair<T>::type p;
  p.x = static_cast<T>(static_cast<double>(axis_level<QM / 2>(sym_bits, 0)) * a);
  p.y = static_cast<T>(static_cast<double>(axis_level<QM / 2>(sym_bits, 1)) * a);
  *reinterpret_cast<typename Pair<T>::type *>(symbols + 2 * id) = p;
}

// ---- the demapper -----------------------------------------------------------------------------------------------------

// one call's per-axis table in the arithmetic type A: amp[u] = A_u, k[u] = (0.5 * scale) * (A_u * A_u), made in double
template <typename A>
struct Axis {
  A amp[16], k[16];
};

// the per-axis table of the demappers with a scale per symbol: q[u] = Q_u = A_u * A_u, made in double; a symbol's
// K_u = (0.5 * s) * Q_u follows from its own s
template <typename A>
struct AxisCsi {
  A amp[16], q[16];
};

// The H LLRs of one axis from its scaled coordinate.  acc1[t] starts at its first element, u = 1 << (H-1-t); acc0[t] at
// u = 0.  Every test on u is wave-uniform.  The max-log fold is one instruction per step, and the exact fold for H <= 2 has
// at most 4 maxstar bodies per axis: those unroll over u completely.  The exact fold for H = 3, 4 (18 and 56 maxstar
// bodies per axis, each an f64 exp and log1p of about 4.7 KB of code) runs the loop over u at run time with H bodies in it:
// 23 and 30 KB per loop, one axis after the other, so that a loop stays within the 64 KB instruction cache while it runs.
// k(u) gives K_u: the call's table entry, or the product with the symbol's own half scale.
template <int H, typename A, bool MAXLOG, typename K>
__device__ __forceinline__ void axis_fold(A s, const A (&amp)[16], K k, A (&out)[H]) {
  A acc0[H], acc1[H];
  const A d0 = s * amp[0] - k(0u);
#pragma unroll
  for (int j = 0; j < H; j++) acc0[j] = acc1[j] = d0;
#pragma unroll MAXLOG || H <= 2 ? (1 << H) - 1 : 1
  for (uint32_t u = 1; u < (1u << H); u++) {
    const A d = s * amp[u] - k(u);
#pragma unroll
    for (int j = 0; j < H; j++) {
      const uint32_t first = 1u << (H - 1 - j);
      if (u & first)
        acc1[j] = u == first ? d : demod::fold_step<MAXLOG>(acc1[j], d);
      else
        acc0[j] = demod::fold_step<MAXLOG>(acc0[j], d);
    }
  }
#pragma unroll
  for (int j = 0; j < H; j++) out[j] = acc0[j] - acc1[j];
}

// The 2 H LLRs of a symbol from its scaled coordinates: llr[2 t] from the I axis, llr[2 t + 1] from the Q axis.
template <int H, typename A, bool MAXLOG, typename K>
__device__ __forceinline__ void axis_llrs_k(A sx, A sy, const A (&amp)[16], K k, A (&llr)[2 * H]) {
  A x[H], y[H];
  axis_fold<H, A, MAXLOG>(sx, amp, k, x);
  axis_fold<H, A, MAXLOG>(sy, amp, k, y);
#pragma unroll
  for (int j = 0; j < H; j++) {
    llr[2 * j] = x[j];
    llr[2 * j + 1] = y[j];
  }
}

// one scale per call: K_u from the table
template <int H, typename A, bool MAXLOG>
__device__ __forceinline__ void axis_llrs(A sx, A sy, const Axis<A> &t, A (&llr)[2 * H]) {
  axis_llrs_k<H, A, MAXLOG>(sx, sy, t.amp, [&](uint32_t u) { return t.k[u]; }, llr);
}

// the symbol's own scale s: sx = x * s, sy = y * s, K_u = half * Q_u with half = 0.5 * s.  K_u is the same for both axes:
// where the loop over u unrolls the compiler makes each product once per symbol, and the run-time loops of the exact
// H = 3, 4 folds make it once per axis, beside H exp / log1p bodies.
template <int H, typename A, bool MAXLOG>
__device__ __forceinline__ void axis_llrs_csi(A sx, A sy, A half, const AxisCsi<A> &t, A (&llr)[2 * H]) {
  axis_llrs_k<H, A, MAXLOG>(sx, sy, t.amp, [&](uint32_t u) { return half * t.q[u]; }, llr);
}

// N values of type T at p (aligned to the piece size) in pieces of 16 bytes, or of 8 where 16 does not divide the row of
// a symbol (float, QM = 2 and 6)
template <bool NT, typename T, int N>
__device__ __forceinline__ void store_row(T *p, const T (&x)[N]) {
  constexpr int kPiece = (N * sizeof(T)) % 16 == 0 ? 16 / sizeof(T) : 8 / sizeof(T);
  typedef T piece __attribute__((ext_vector_type(kPiece)));
#pragma unroll
  for (int i = 0; i < N; i += kPiece) {
    piece v;
#pragma unroll
    for (int e = 0; e < kPiece; e++) v[e] = x[i + e];
    demod::store_llr<NT>(reinterpret_cast<piece *>(p + i), v);
  }
}

// symbols [frames][symbols_len] (re, im) -> llrs [frames][2 H symbols_len]; c: the scrambling sequence, or nullptr
template <int H, typename IO, typename A, bool MAXLOG>
__global__ __launch_bounds__(kThreads) void demap_kernel(const IO *__restrict__ symbols, IO *__restrict__ llrs, uint32_t symbols_len,
                                                         uint64_t total, A scale, const uint32_t *__restrict__ c, const Axis<A> t) {
  const uint64_t id = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (id >= total) return;
  const typename Pair<IO>::type s = *reinterpret_cast<const typename Pair<IO>::type *>(symbols + 2 * id);
  A llr[2 * H];
  axis_llrs<H, A, MAXLOG>(static_cast<A>(s.x) * scale, static_cast<A>(s.y) * scale, t, llr);
  uint32_t flip = 0;
  if (c != nullptr) flip = gold_window<2 * H>(c, 2 * H * static_cast<uint32_t>(id % symbols_len));
  IO out[2 * H];
#pragma unroll
  for (int j = 0; j < 2 * H; j++) {
    const IO x = static_cast<IO>(llr[j]);
    out[j] = ((flip >> j) & 1u) ? -x : x;
  }
  store_row<MAXLOG>(llrs + id * (2 * H), out);
}

// The 8-bit demapper (include/ldpc_toolbox.h, PART 9): demap_kernel<H, float, A, MAXLOG> up to the float it would store --
// exact: double arithmetic rounded once to float -- then the descrambling sign and Q (soft_i8.h; Q(-x) = -Q(x), and the sign
// goes first as it does in the float row).  The 2 H bytes of a symbol are packed into one 64-bit word and leave in pieces:
// WIDE (the row buffer's address is a multiple of 4) dwords for H = 2, 4 and half-words for H = 1, 3 -- every symbol's
// address is then a multiple of the piece -- else single bytes, for a buffer at any byte address.
template <int H, typename A, bool MAXLOG, bool WIDE>
__global__ __launch_bounds__(kThreads) void demap_i8_kernel(const float *__restrict__ symbols, int8_t *__restrict__ llrs, uint32_t symbols_len,
                                                            uint64_t total, A scale, const uint32_t *__restrict__ c, const Axis<A> t) {
  const uint64_t id = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (id >= total) return;
  const typename Pair<float>::type s = *reinterpret_cast<const typename Pair<float>::type *>(symbols + 2 * id);
  A llr[2 * H];
  axis_llrs<H, A, MAXLOG>(static_cast<A>(s.x) * scale, static_cast<A>(s.y) * scale, t, llr);
  uint32_t flip = 0;
  if (c != nullptr) flip = gold_window<2 * H>(c, 2 * H * static_cast<uint32_t>(id % symbols_len));
  uint64_t w = 0;
#pragma unroll
  for (int j = 0; j < 2 * H; j++) {
    const float x = static_cast<float>(llr[j]);
    const int q = soft::soft_quantize(static_cast<double>(((flip >> j) & 1u) ? -x : x));
    w |= uint64_t(static_cast<uint8_t>(q)) << (8 * j);
  }
  int8_t *row = llrs + id * (2 * H);
  if constexpr (WIDE && H % 2 == 0) {
#pragma unroll
    for (int i = 0; i < 2 * H; i += 4) demod::store_llr<MAXLOG>(reinterpret_cast<uint32_t *>(row + i), static_cast<uint32_t>(w >> (8 * i)));
  } else if constexpr (WIDE) {
#pragma unroll
    for (int i = 0; i < 2 * H; i += 2) demod::store_llr<MAXLOG>(reinterpret_cast<uint16_t *>(row + i), static_cast<uint16_t>(w >> (8 * i)));
  } else {
#pragma unroll
    for (int i = 0; i < 2 * H; i++) row[i] = static_cast<int8_t>(w >> (8 * i));
  }
}

// ---- the demappers with a scale per symbol (include/ldpc_toolbox.h, PART 10) ---------------------------------------------
// scale [frames][symbols_len], s = 1 / sigma_s^2 of the symbol, one coalesced load per lane beside the symbol's; sx = x * s and
// K_u = (0.5 * s) * Q_u take the place of the call's scale and table.  Everything behind the LLRs is that of demap_kernel and
// demap_i8_kernel, whose bodies stay as they are written above: moved into these helpers their loads are scheduled
// differently, and a kernel that exists keeps its instructions (tools/kernel_digest.py).

// the 2 H LLRs of symbol `id`, each rounded once to IO and negated where its bit of c is set, to their place in llrs
template <int H, typename IO, typename A, bool MAXLOG>
__device__ __forceinline__ void store_llrs(const A (&llr)[2 * H], const uint32_t *c, uint64_t id, uint32_t symbols_len, IO *llrs) {
  uint32_t flip = 0;
  if (c != nullptr) flip = gold_window<2 * H>(c, 2 * H * static_cast<uint32_t>(id % symbols_len));
  IO out[2 * H];
#pragma unroll
  for (int j = 0; j < 2 * H; j++) {
    const IO x = static_cast<IO>(llr[j]);
    out[j] = ((flip >> j) & 1u) ? -x : x;
  }
  store_row<MAXLOG>(llrs + id * (2 * H), out);
}

// ... each rounded once to float, signed and quantised, in the pieces of demap_i8_kernel
template <int H, typename A, bool MAXLOG, bool WIDE>
__device__ __forceinline__ void store_soft_bits(const A (&llr)[2 * H], const uint32_t *c, uint64_t id, uint32_t symbols_len, int8_t *llrs) {
  uint32_t flip = 0;
  if (c != nullptr) flip = gold_window<2 * H>(c, 2 * H * static_cast<uint32_t>(id % symbols_len));
  uint64_t w = 0;
#pragma unroll
  for (int j = 0; j < 2 * H; j++) {
    const float x = static_cast<float>(llr[j]);
    const int q = soft::soft_quantize(static_cast<double>(((flip >> j) & 1u) ? -x : x));
    w |= uint64_t(static_cast<uint8_t>(q)) << (8 * j);
  }
  int8_t *row = llrs + id * (2 * H);
  if constexpr (WIDE && H % 2 == 0) {
#pragma unroll
    for (int i = 0; i < 2 * H; i += 4) demod::store_llr<MAXLOG>(reinterpret_cast<uint32_t *>(row + i), static_cast<uint32_t>(w >> (8 * i)));
  } else if constexpr (WIDE) {
#pragma unroll
    for (int i = 0; i < 2 * H; i += 2) demod::store_llr<MAXLOG>(reinterpret_cast<uint16_t *>(row + i), static_cast<uint16_t>(w >> (8 * i)));
  } else {
#pragma unroll
    for (int i = 0; i < 2 * H; i++) row[i] = static_cast<int8_t>(w >> (8 * i));
  }
}

template <int H, typename IO, typename A, bool MAXLOG>
__global__ __launch_bounds__(kThreads) void demap_csi_kernel(const IO *__restrict__ symbols, const IO *__restrict__ scale,
                                                             IO *__restrict__ llrs, uint32_t symbols_len, uint64_t total,
                                                             const uint32_t *__restrict__ c, const AxisCsi<A> t) {
  const uint64_t id = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (id >= total) return;
  const typename Pair<IO>::type s = *reinterpret_cast<const typename Pair<IO>::type *>(symbols + 2 * id);
  const A sc = static_cast<A>(scale[id]);
  A llr[2 * H];
  axis_llrs_csi<H, A, MAXLOG>(static_cast<A>(s.x) * sc, static_cast<A>(s.y) * sc, static_cast<A>(0.5) * sc, t, llr);
  store_llrs<H, IO, A, MAXLOG>(llr, c, id, symbols_len, llrs);
}

// demap_csi_kernel<H, float, A, MAXLOG> up to the float it would store, then the soft bits of demap_i8_kernel
template <int H, typename A, bool MAXLOG, bool WIDE>
__global__ __launch_bounds__(kThreads) void demap_csi_i8_kernel(const float *__restrict__ symbols, const float *__restrict__ scale,
                                                                int8_t *__restrict__ llrs, uint32_t symbols_len, uint64_t total,
                                                                const uint32_t *__restrict__ c, const AxisCsi<A> t) {
  const uint64_t id = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (id >= total) return;
  const typename Pair<float>::type s = *reinterpret_cast<const typename Pair<float>::type *>(symbols + 2 * id);
  const A sc = static_cast<A>(scale[id]);
  A llr[2 * H];
  axis_llrs_csi<H, A, MAXLOG>(static_cast<A>(s.x) * sc, static_cast<A>(s.y) * sc, static_cast<A>(0.5) * sc, t, llr);
  store_soft_bits<H, A, MAXLOG, WIDE>(llr, c, id, symbols_len, llrs);
}

// ---- the simulator's generator ----------------------------------------------------------------------------------------

// the per-axis table of a generator: the call's K_u, or (FADING) Q_u for the symbol's own scale
template <bool FADING>
struct GeneratorAxis {
  typedef Axis<double> type;
};
template <>
struct GeneratorAxis<true> {
  typedef AxisCsi<double> type;
};

// One symbol of a generator over the Rayleigh block-fading channel: sym_bits -> (A_uI, A_uQ) -> the gain of block
// pair / block (gen::fading_scale) gives the symbol's sigma_e and scale -> + sigma_e * (double)z per coordinate, z =
// gen::normal_pair(seed, frame, pair) -> axis_llrs_csi in f64: ldpc_toolbox_fading_run_f64 and ldpc_toolbox_nr_demap_csi_f64 in
// one.  The symbol and its scale are never stored.
template <int H, bool MAXLOG>
__device__ __forceinline__ void fading_symbol_llrs(uint32_t sym_bits, uint64_t seed, uint64_t frame, uint32_t pair, double sigma, double a,
                                                   const AxisCsi<double> &t, uint32_t block, double (&llr)[2 * H]) {
  float z0, z1;
  gen::normal_pair(seed, frame, pair, &z0, &z1);
  double sigma_e, scale_s;
  gen::fading_scale(seed, frame, pair / block, sigma, &sigma_e, &scale_s);
  const double re = static_cast<double>(axis_level<H>(sym_bits, 0)) * a + sigma_e * static_cast<double>(z0);
  const double im = static_cast<double>(axis_level<H>(sym_bits, 1)) * a + sigma_e * static_cast<double>(z1);
  axis_llrs_csi<H, double, MAXLOG>(re * scale_s, im * scale_s, 0.5 * scale_s, t, llr);
}

// Frame first_frame + f: the pooled transmitted row's 2 H bits of symbol `sym` -> (A_uI, A_uQ) -> + sigma * (double)z per
// coordinate, z = gen::normal_pair(seed, frame, sym) -> axis_llrs in f64 -> each LLR rounded once to float, in
// transmitted order.  No scrambling; the symbol is never stored.  (The destination may be a caller's buffer of any float
// alignment: scalar stores.)  FADING: the channel and demapper of fading_symbol_llrs with `block` symbols per gain; `scale`
// is not used and t holds Q_u.
template <int H, bool MAXLOG, bool FADING>
__global__ __launch_bounds__(kThreads) void qam_llr_kernel(const uint8_t *__restrict__ tx_bits, uint32_t pool, uint32_t n_tx, uint64_t seed,
                                                           uint64_t first_frame, uint64_t total, double sigma, double scale, double a,
                                                           const typename GeneratorAxis<FADING>::type t, float *__restrict__ llrs,
                                                           uint32_t block) {
  const uint64_t id = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (id >= total) return;
  const uint32_t symbols = n_tx / (2 * H);
  const uint64_t f = id / symbols;
  const uint32_t sym = static_cast<uint32_t>(id - f * symbols);
  const uint64_t frame = first_frame + f;
  const uint8_t *b = tx_bits + size_t(gen::pool_index(seed, frame, pool)) * n_tx + size_t(2 * H) * sym;
  uint32_t sym_bits = 0;
#pragma unroll
  for (int j = 0; j < 2 * H; j++) sym_bits |= (b[j] == 1 ? 1u : 0u) << j;
  double llr[2 * H];
  if constexpr (FADING) {
    fading_symbol_llrs<H, MAXLOG>(sym_bits, seed, frame, sym, sigma, a, t, block, llr);
  } else {
    float z0, z1;
    gen::normal_pair(seed, frame, sym, &z0, &z1);
    const double re = static_cast<double>(axis_level<H>(sym_bits, 0)) * a + sigma * static_cast<double>(z0);
    const double im = static_cast<double>(axis_level<H>(sym_bits, 1)) * a + sigma * static_cast<double>(z1);
    axis_llrs<H, double, MAXLOG>(re * scale, im * scale, t, llr);
  }
  float *row = llrs + f * n_tx + size_t(2 * H) * sym;
#pragma unroll
  for (int j = 0; j < 2 * H; j++) row[j] = static_cast<float>(llr[j]);
}

// One transmission of a HARQ sequence (nr_harq.h): qam_llr_kernel for a list of frames at a pair offset.  tx_bits
// [pool][e]: this transmission's pooled transmitted rows; row r of llrs [frames][e] is frame frame_ids[r], or
// first_frame + r without a list; symbol s of the row takes the normal pair first_symbol + s, the pair of that symbol in
// the frame's concatenated row -- and (FADING) the gain of block (first_symbol + s) / block of that row.  The arithmetic is
// qam_llr_kernel's.
template <int H, bool MAXLOG, bool FADING>
__global__ __launch_bounds__(kThreads) void qam_llr_harq_kernel(const uint8_t *__restrict__ tx_bits, uint32_t pool, uint32_t e,
                                                                uint32_t first_symbol, uint64_t seed, uint64_t first_frame,
                                                                const uint64_t *__restrict__ frame_ids, uint64_t total, double sigma,
                                                                double scale, double a, const typename GeneratorAxis<FADING>::type t,
                                                                float *__restrict__ llrs, uint32_t block) {
  const uint64_t id = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (id >= total) return;
  const uint32_t symbols = e / (2 * H);
  const uint64_t f = id / symbols;
  const uint32_t sym = static_cast<uint32_t>(id - f * symbols);
  const uint64_t frame = frame_ids ? frame_ids[f] : first_frame + f;
  const uint8_t *b = tx_bits + size_t(gen::pool_index(seed, frame, pool)) * e + size_t(2 * H) * sym;
  uint32_t sym_bits = 0;
#pragma unroll
  for (int j = 0; j < 2 * H; j++) sym_bits |= (b[j] == 1 ? 1u : 0u) << j;
  double llr[2 * H];
  if constexpr (FADING) {
    fading_symbol_llrs<H, MAXLOG>(sym_bits, seed, frame, first_symbol + sym, sigma, a, t, block, llr);
  } else {
    float z0, z1;
    gen::normal_pair(seed, frame, first_symbol + sym, &z0, &z1);
    const double re = static_cast<double>(axis_level<H>(sym_bits, 0)) * a + sigma * static_cast<double>(z0);
    const double im = static_cast<double>(axis_level<H>(sym_bits, 1)) * a + sigma * static_cast<double>(z1);
    axis_llrs<H, double, MAXLOG>(re * scale, im * scale, t, llr);
  }
  float *row = llrs + f * e + size_t(2 * H) * sym;
#pragma unroll
  for (int j = 0; j < 2 * H; j++) row[j] = static_cast<float>(llr[j]);
}

}  // namespace nrqam
}  // namespace ldpc
