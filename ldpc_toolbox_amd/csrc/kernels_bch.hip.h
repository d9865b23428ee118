// Kernels of the batched BCH code (bch.h, device_bch.h).  A workgroup of 256 lanes owns one frame.
//
//   remainder_kernel<NW, DECODE>   stages the frame's bytes as bits in LDS (a ballot per 64 bytes; the normalised
//       bytes are copied to the output on the way), each lane divides its run of bits by g in a register of NW words
//       (bch::rem_step), the runs are combined through the table of x^(offset + i) mod g and XOR-reduced with wave
//       shuffles and LDS.  Encoder: the remainder is written behind the message.  Decoder: a frame whose remainder is
//       zero is finished (errors = 0); any other is appended to the list with one atomic, with its t odd syndromes.
//   locator_kernel   a lane per listed frame: bch::locator (fully unrolled, no indexed register arrays), the
//       coefficients left as logs.
//   chien_kernel     a workgroup per listed frame, lanes across the n positions of the shortened word: roots are
//       counted and at most t positions recorded; bits are flipped only when the count equals the locator's length.
// All stores are of one or four bytes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bch.h"

namespace ldpc {
namespace bch {

constexpr uint32_t kLocWords = kMaxT + 2;  // per listed frame: 13 logs and the length L

template <int NW>
struct GeneratorTop {
  uint32_t w[NW];
};

struct DecodeArgs {
  uint32_t m, t;
  const uint16_t *antilog;
  int32_t *errors;   // may be null
  uint32_t *list;    // frames with a non-zero remainder
  uint32_t *count;   // their number
  uint16_t *synd;    // [slot][kMaxT]: S(1), S(3), ...
};

// in [frames][bits], out [frames][out_stride]: bytes [0, copy_len) of a row are the normalised input.
// grid = frames, 256 threads.  table: remainder_table of geo.
template <int NW, bool DECODE>
__global__ __launch_bounds__(kThreads) void remainder_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                             uint32_t copy_len, uint32_t out_stride, uint32_t parity,
                                                             Geometry geo, GeneratorTop<NW> g_top,
                                                             const uint32_t *__restrict__ table, DecodeArgs d) {
  __shared__ uint32_t staged[kMaxStagedWords];
  __shared__ uint32_t partial[kThreads / 64][NW];
  __shared__ uint32_t total[kMaxParityWords];
  __shared__ uint32_t slot_shared;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint8_t *row = in + size_t(blockIdx.x) * geo.bits;
  uint8_t *orow = out + size_t(blockIdx.x) * out_stride;
  // bit q of the staged words is byte q - pad of the row (zero in front of it and behind it)
  for (uint32_t q = tid; q < geo.staged_words * 32; q += kThreads) {
    bool b = false;
    if (q >= geo.pad && q - geo.pad < geo.bits) {
      const uint32_t i = q - geo.pad;
      b = row[i] == 1;
      if (i < copy_len) orow[i] = b;
    }
    const unsigned long long mask = __ballot(b);
    if (lane == 0) {
      staged[q >> 5] = static_cast<uint32_t>(mask);
      staged[(q >> 5) + 1] = static_cast<uint32_t>(mask >> 32);
    }
  }
  __syncthreads();
  uint32_t acc[NW];
#pragma unroll
  for (int w = 0; w < NW; w++) acc[w] = 0;
  if (tid < geo.lanes) {
    uint32_t s[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) s[w] = 0;
    for (uint32_t w = 0; w < geo.run_words; w++) {
      const uint32_t x = staged[tid * geo.run_words + w];
      for (uint32_t b = 0; b < 32; b++) rem_step<NW>(s, g_top.w, (x >> b) & 1u);
    }
    // s holds the run's remainder left-aligned: bit j of s is the coefficient of x^(j - shift)
    const uint32_t shift = 32 * NW - parity;
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const uint32_t x = s[w];
      for (uint32_t b = 0; b < 32; b++) {
        const uint32_t j = 32 * w + b;
        if (j < shift) continue;
        const uint32_t keep = 0u - ((x >> b) & 1u);
        const uint32_t *entry = table + size_t(j - shift) * NW * geo.lanes + tid;
#pragma unroll
        for (int ww = 0; ww < NW; ww++) acc[ww] ^= keep & entry[size_t(ww) * geo.lanes];
      }
    }
  }
#pragma unroll
  for (int w = 0; w < NW; w++) {
    uint32_t v = acc[w];
#pragma unroll
    for (int dlt = 32; dlt >= 1; dlt >>= 1) v ^= __shfl_xor(v, dlt, 64);
    if (lane == 0) partial[wave][w] = v;
  }
  __syncthreads();
  if (tid < kMaxParityWords) {
    uint32_t v = 0;
    if (tid < NW)
      for (uint32_t wv = 0; wv < kThreads / 64; wv++) v ^= partial[wv][tid];
    total[tid] = v;
  }
  __syncthreads();
  if constexpr (!DECODE) {
    // byte bits + q of the codeword is the coefficient of x^(parity - 1 - q)
    for (uint32_t q = tid; q < parity; q += kThreads) {
      const uint32_t i = parity - 1 - q;
      orow[geo.bits + q] = static_cast<uint8_t>((total[i >> 5] >> (i & 31)) & 1u);
    }
  } else {
    uint32_t any = 0;
#pragma unroll
    for (uint32_t w = 0; w < kMaxParityWords; w++) any |= total[w];
    if (any == 0) {
      if (tid == 0 && d.errors) d.errors[blockIdx.x] = 0;
      return;
    }
    if (tid == 0) {
      const uint32_t slot = atomicAdd(d.count, 1u);
      d.list[slot] = blockIdx.x;
      slot_shared = slot;
    }
    __syncthreads();
    if (tid < d.t)
      d.synd[size_t(slot_shared) * kMaxT + tid] =
          static_cast<uint16_t>(syndrome_of_remainder(total, parity, 2 * tid + 1, d.m, d.antilog));
  }
}

// loc [slot][kLocWords]: the logs of lambda_0..lambda_12 (kNoLog for a zero) and L.  grid = ceil(frames / 64), 64 threads.
__global__ __launch_bounds__(64) void locator_kernel(const uint16_t *__restrict__ synd, const uint32_t *__restrict__ count,
                                                     const uint16_t *__restrict__ log, uint16_t *__restrict__ loc, uint32_t t,
                                                     uint32_t poly, uint32_t m) {
  const uint32_t slot = blockIdx.x * 64 + threadIdx.x;
  if (slot >= *count) return;
  uint32_t odd[kMaxT], lambda[kMaxT + 1];
#pragma unroll
  for (uint32_t j = 0; j < kMaxT; j++) odd[j] = j < t ? synd[size_t(slot) * kMaxT + j] : 0u;
  const uint32_t L = locator(odd, t, poly, m, lambda);
#pragma unroll
  for (uint32_t i = 0; i <= kMaxT; i++) loc[size_t(slot) * kLocWords + i] = log[lambda[i]];
  loc[size_t(slot) * kLocWords + kMaxT + 1] = static_cast<uint16_t>(L);
}

// out [frames][out_len], the normalised input already in it.  grid = frames (a block past the count returns), 256 threads.
// Roots count among the n positions of the shortened word only.
__global__ __launch_bounds__(kThreads) void chien_kernel(uint8_t *__restrict__ out, uint32_t out_len, uint32_t n, uint32_t t,
                                                         uint32_t m,
                                                         const uint16_t *__restrict__ antilog2, const uint32_t *__restrict__ list,
                                                         const uint32_t *__restrict__ count, const uint16_t *__restrict__ loc,
                                                         int32_t *__restrict__ errors) {
  __shared__ uint32_t found;
  __shared__ uint32_t position[kMaxT];
  const uint32_t slot = blockIdx.x, tid = threadIdx.x;
  if (slot >= *count) return;
  const uint32_t frame = list[slot];
  const uint32_t L = loc[size_t(slot) * kLocWords + kMaxT + 1];
  if (L > t) {
    if (tid == 0 && errors) errors[frame] = -1;
    return;
  }
  uint16_t loglambda[kMaxT + 1];
#pragma unroll
  for (uint32_t i = 0; i <= kMaxT; i++) loglambda[i] = loc[size_t(slot) * kLocWords + i];
  if (tid == 0) found = 0;
  __syncthreads();
  for (uint32_t p = tid; p < n; p += kThreads) {
    if (!is_root(loglambda, p, m, antilog2)) continue;
    const uint32_t at = atomicAdd(&found, 1u);
    if (at < kMaxT) position[at] = p;
  }
  __syncthreads();
  // (the flips come after the count is known: a frame that fails leaves as it came)
  const bool ok = found == L;
  if (ok && tid < L) {
    const uint32_t p = position[tid];
    if (p < n && n - 1 - p < out_len) out[size_t(frame) * out_len + (n - 1 - p)] ^= 1u;
  }
  if (tid == 0 && errors) errors[frame] = ok ? static_cast<int32_t>(L) : -1;
}

}  // namespace bch
}  // namespace ldpc
