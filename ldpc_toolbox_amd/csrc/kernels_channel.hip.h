// Kernels of the transmit side of a constellation handle (demodulator.h has the definitions): the batched modulator,
// the AWGN and the Rayleigh block-fading channel, and the simulator's fused generator for any table constellation.  One thread per symbol, indexed by
// a 64-bit id.  Compiled with -ffp-contract=off: sigma * z and x + (sigma * z) are rounded once each.
//
// In the demapper the point index V is wave-uniform and the table is read from the kernel arguments with scalar loads.
// A mapper's V differs from lane to lane, so the points go through LDS (32 points: 512 B in f64): the threads of a
// block's first half-wave copy one point each -- every index into the kernel arguments a compile-time constant -- and each
// thread then reads the point of its own V.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "frame_gen.hip.h"
#include "kernels_demod.hip.h"

namespace ldpc {
namespace chan {

constexpr int kThreads = demod::kThreads;

// the points of one call in the type of the symbols
template <typename T>
struct Points {
  T re[32], im[32];
};

// thread v < 32 of the block writes point v; the barrier is the block's: no thread may have left before it
template <typename T>
__device__ __forceinline__ void stage_points(const T (&src_re)[32], const T (&src_im)[32], T *lds_re, T *lds_im) {
  if (threadIdx.x < 32) {  // (false for the whole of every wave but the block's first: they go straight to the barrier)
    T re = 0, im = 0;
#pragma unroll
    for (uint32_t v = 0; v < 32; v++)
      if (threadIdx.x == v) {
        re = src_re[v];
        im = src_im[v];
      }
    lds_re[threadIdx.x] = re;
    lds_im[threadIdx.x] = im;
  }
  __syncthreads();
}

// V of symbol `sym`: bit j is the one at codeword position pos[j] = deinterleaved_position(m sym + j)
__device__ __forceinline__ uint32_t symbol_index(const uint8_t *__restrict__ cw, uint32_t m, uint32_t sym, uint32_t len,
                                                 int32_t interleaving) {
  uint32_t v = 0;
  for (uint32_t j = 0; j < m; j++)
    v |= (cw[gen::deinterleaved_position(m * sym + j, len, interleaving)] == 1 ? 1u : 0u) << (m - 1 - j);
  return v;
}

// bits [frames][bits_len] -> symbols [frames][symbols_len] (re, im)
template <typename T>
__global__ __launch_bounds__(kThreads) void mod_kernel(const uint8_t *__restrict__ bits, T *__restrict__ symbols, uint32_t m,
                                                       uint32_t symbols_len, uint32_t bits_len, uint64_t total,
                                                       int32_t interleaving, const Points<T> t) {
  __shared__ T lds_re[32], lds_im[32];
  stage_points(t.re, t.im, lds_re, lds_im);
  const uint64_t id = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (id >= total) return;
  const uint64_t f = id / symbols_len;
  const uint32_t sym = static_cast<uint32_t>(id - f * symbols_len);
  const uint32_t v = symbol_index(bits + f * bits_len, m, sym, bits_len, interleaving);
  symbols[2 * id] = lds_re[v];
  symbols[2 * id + 1] = lds_im[v];
}

// BPSK: reals, +1 for a one, -1 for a zero (modulation.rs:87-95)
template <typename T>
__global__ __launch_bounds__(kThreads) void bpsk_mod_kernel(const uint8_t *__restrict__ bits, T *__restrict__ symbols,
                                                            uint32_t bits_len, uint64_t total, int32_t interleaving) {
  const uint64_t id = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (id >= total) return;
  const uint64_t f = id / bits_len;
  const uint32_t i = static_cast<uint32_t>(id - f * bits_len);
  symbols[id] = bits[f * bits_len + gen::deinterleaved_position(i, bits_len, interleaving)] == 1 ? T(1) : T(-1);
}

// channel.rs:76-81 in place: symbol s of row r gets the normal pair (seed, first_frame + r, s)
template <typename T>
__global__ __launch_bounds__(kThreads) void awgn_kernel(T *__restrict__ symbols, uint32_t symbols_len, uint64_t total, T sigma,
                                                        uint64_t seed, uint64_t first_frame) {
  const uint64_t id = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (id >= total) return;
  const uint64_t f = id / symbols_len;
  const uint32_t sym = static_cast<uint32_t>(id - f * symbols_len);
  float z0, z1;
  gen::normal_pair(seed, first_frame + f, sym, &z0, &z1);
  symbols[2 * id] = symbols[2 * id] + sigma * static_cast<T>(z0);
  symbols[2 * id + 1] = symbols[2 * id + 1] + sigma * static_cast<T>(z1);
}

// real symbols: one thread per pair of positions (2 pair, 2 pair + 1), the keying of gen::awgn_llr_kernel
template <typename T>
__global__ __launch_bounds__(kThreads) void awgn_real_kernel(T *__restrict__ symbols, uint32_t symbols_len, uint32_t pairs,
                                                             uint64_t total, T sigma, uint64_t seed, uint64_t first_frame) {
  const uint64_t id = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (id >= total) return;
  const uint64_t f = id / pairs;
  const uint32_t pair = static_cast<uint32_t>(id - f * pairs);
  float z0, z1;
  gen::normal_pair(seed, first_frame + f, pair, &z0, &z1);
  T *row = symbols + f * symbols_len;
  const uint32_t j = 2 * pair;
  row[j] = row[j] + sigma * static_cast<T>(z0);
  if (j + 1 < symbols_len) row[j + 1] = row[j + 1] + sigma * static_cast<T>(z1);
}

// Rayleigh block fading behind a one-tap equaliser, in place: symbol s of row r gets the noise pair (seed, first_frame + r, s)
// of awgn_kernel at sigma_e = sigma / af, af the gain of its block s / block (gen::fading_scale), and scale[s] = 1 / sigma_e^2:
// what the CSI demapper takes.  A wave's lanes mostly share a block; each lane computes the gain for itself -- a Philox
// block and a logf beside the ones its noise pair costs, and no LDS or cross-lane traffic.  One (re, im) load and store.
template <typename T>
__global__ __launch_bounds__(kThreads) void fading_kernel(T *__restrict__ symbols, T *__restrict__ scale, uint32_t symbols_len,
                                                          uint64_t total, double sigma, uint32_t block, uint64_t seed,
                                                          uint64_t first_frame) {
  typedef T pair __attribute__((ext_vector_type(2)));
  const uint64_t id = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (id >= total) return;
  const uint64_t f = id / symbols_len;
  const uint32_t sym = static_cast<uint32_t>(id - f * symbols_len);
  double sigma_e, scale_s;
  gen::fading_scale(seed, first_frame + f, sym / block, sigma, &sigma_e, &scale_s);
  float z0, z1;
  gen::normal_pair(seed, first_frame + f, sym, &z0, &z1);
  const T se = static_cast<T>(sigma_e);
  pair p = *reinterpret_cast<const pair *>(symbols + 2 * id);
  p.x = p.x + se * static_cast<T>(z0);
  p.y = p.y + se * static_cast<T>(z1);
  *reinterpret_cast<pair *>(symbols + 2 * id) = p;
  scale[id] = static_cast<T>(scale_s);
}

// The simulator's generator for a table constellation of M bits, fused: pooled codeword -> the M bits of the symbol at
// their deinterleaved positions -> p_V -> + sigma * (double)z per coordinate -> the f64 demapper of
// demod::table_kernel<M, double, double, MAXLOG> (the same d_V expression, the same folds through demod::fold_step) ->
// each LLR rounded once to float, at its codeword position.  The symbol itself is never stored.  t.c[V] = (0.5 * scale) * e_V.
// As in table_kernel, M <= 3 unrolls over V and M = 4, 5 loop over V at run time.
template <int M, bool MAXLOG>
__global__ __launch_bounds__(kThreads) void table_llr_kernel(const uint8_t *__restrict__ tx_bits, uint32_t pool, uint32_t n_tx,
                                                             int32_t interleaving, uint64_t seed, uint64_t first_frame,
                                                             uint64_t total, double sigma, double scale, int32_t energy,
                                                             const demod::Table<double> t, float *__restrict__ llrs) {
  __shared__ double lds_re[32], lds_im[32];
  stage_points(t.re, t.im, lds_re, lds_im);
  const uint64_t id = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (id >= total) return;
  const uint32_t symbols = n_tx / M;
  const uint64_t f = id / symbols;
  const uint32_t sym = static_cast<uint32_t>(id - f * symbols);
  const uint64_t frame = first_frame + f;
  const uint8_t *cw = tx_bits + size_t(gen::pool_index(seed, frame, pool)) * n_tx;
  uint32_t pos[M], v_tx = 0;
#pragma unroll
  for (int j = 0; j < M; j++) {
    pos[j] = gen::deinterleaved_position(M * sym + j, n_tx, interleaving);
    v_tx |= (cw[pos[j]] == 1 ? 1u : 0u) << (M - 1 - j);
  }
  float z0, z1;
  gen::normal_pair(seed, frame, sym, &z0, &z1);
  const double re = lds_re[v_tx] + sigma * static_cast<double>(z0);
  const double im = lds_im[v_tx] + sigma * static_cast<double>(z1);
  const double sr = re * scale, si = im * scale;
  auto dist = [&](uint32_t v) {
    double d = sr * t.re[v] + si * t.im[v];
    if (energy) d = d - t.c[v];
    return d;
  };
  double acc0[M], acc1[M];
  const double d0 = dist(0);
#pragma unroll
  for (int j = 0; j < M; j++) acc0[j] = acc1[j] = d0;
#pragma unroll M <= 3 ? (1 << M) - 1 : 1
  for (uint32_t v = 1; v < (1u << M); v++) {
    const double d = dist(v);
#pragma unroll
    for (int j = 0; j < M; j++) {
      const uint32_t first = 1u << (M - 1 - j);
      if (v & first)
        acc1[j] = v == first ? d : demod::fold_step<MAXLOG>(acc1[j], d);
      else
        acc0[j] = demod::fold_step<MAXLOG>(acc0[j], d);
    }
  }
  float *row = llrs + f * n_tx;
#pragma unroll
  for (int j = 0; j < M; j++) row[pos[j]] = static_cast<float>(acc0[j] - acc1[j]);
}

}  // namespace chan
}  // namespace ldpc
