// Kernels of the batched soft demapper (demodulator.h has the definition).  One thread per symbol, indexed by a 64-bit
// id; no LDS.  The constellation table travels in the kernel arguments and its indices are wave-uniform, so a point is
// read with scalar loads.  Compiled with -ffp-contract=off: a d_V is two products and a sum, as in the reference.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "frame_gen.hip.h"

namespace ldpc {
namespace demod {

constexpr int kThreads = 256;

// the table of one call in the arithmetic type A: c[V] = (0.5 * scale) * e_V (read only when the table has an energy term)
template <typename A>
struct Table {
  A re[32], im[32], c[32];
};

template <bool MAXLOG>
__device__ __forceinline__ double fold_step(double a, double b) {
  if constexpr (MAXLOG)
    return __builtin_fmax(a, b);
  else
    return gen::maxstar(a, b);
}
template <bool MAXLOG>
__device__ __forceinline__ float fold_step(float a, float b) {
  static_assert(MAXLOG, "the exact fold is f64 arithmetic");
  return __builtin_fmaxf(a, b);
}

template <bool NT, typename T>
__device__ __forceinline__ void store_llr(T *p, T x) {
  if constexpr (NT)
    __builtin_nontemporal_store(x, p);
  else
    *p = x;
}

// BPSK: symbols [frames][llrs_len] reals; llr = scale * x at the deinterleaved position
template <typename T>
__global__ __launch_bounds__(kThreads) void bpsk_kernel(const T *__restrict__ symbols, T *__restrict__ llrs, uint32_t llrs_len,
                                                        uint64_t total, T scale, int32_t interleaving) {
  const uint64_t id = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (id >= total) return;
  const uint64_t f = id / llrs_len;
  const uint32_t i = static_cast<uint32_t>(id - f * llrs_len);
  store_llr<true>(llrs + f * llrs_len + gen::deinterleaved_position(i, llrs_len, interleaving), scale * symbols[id]);
}

// Table constellations of M bits: IO = type of the symbols and LLRs, A = type of the arithmetic.  The 2 M fold
// accumulators stay in registers: j is always unrolled, and every test on V is wave-uniform.  M <= 3 unrolls over V
// completely; for M = 4, 5 the loop over V runs at run time (2^M * M inlined maxstar bodies would not fit the instruction cache).
// acc1[j] starts at its first element, V = 1 << (M-1-j); acc0[j] at V = 0.
template <int M, typename IO, typename A, bool MAXLOG>
__global__ __launch_bounds__(kThreads) void table_kernel(const IO *__restrict__ symbols, IO *__restrict__ llrs,
                                                         uint32_t symbols_len, uint32_t llrs_len, uint64_t total, A scale,
                                                         int32_t interleaving, int32_t energy, const Table<A> t) {
  const uint64_t id = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (id >= total) return;
  const uint64_t f = id / symbols_len;
  const uint32_t sym = static_cast<uint32_t>(id - f * symbols_len);
  const A sr = static_cast<A>(symbols[2 * id]) * scale, si = static_cast<A>(symbols[2 * id + 1]) * scale;
  auto dist = [&](uint32_t v) {
    A d = sr * t.re[v] + si * t.im[v];
    if (energy) d = d - t.c[v];
    return d;
  };
  A acc0[M], acc1[M];
  const A d0 = dist(0);
#pragma unroll
  for (int j = 0; j < M; j++) acc0[j] = acc1[j] = d0;
#pragma unroll M <= 3 ? (1 << M) - 1 : 1
  for (uint32_t v = 1; v < (1u << M); v++) {
    const A d = dist(v);
#pragma unroll
    for (int j = 0; j < M; j++) {
      const uint32_t first = 1u << (M - 1 - j);
      if (v & first)
        acc1[j] = v == first ? d : fold_step<MAXLOG>(acc1[j], d);
      else
        acc0[j] = fold_step<MAXLOG>(acc0[j], d);
    }
  }
  IO *row = llrs + f * llrs_len;
#pragma unroll
  for (int j = 0; j < M; j++)
    store_llr<MAXLOG>(row + gen::deinterleaved_position(M * sym + j, llrs_len, interleaving), static_cast<IO>(acc0[j] - acc1[j]));
}

}  // namespace demod
}  // namespace ldpc
