// Kernels of 5G NR transport block segmentation, CRC attachment and checking, and code block concatenation
// (nr_transport_block.h, device_nr_tb.h).  Code block rows are block-major: row r * batch + b is block r of transport
// block b.  A launch covers one pass: the transport blocks b0 .. b0 + frames - 1 of the batch.
//
//   rows_kernel<SEGMENT>   a workgroup of 256 lanes per code block row, grid = C * frames.  Every byte of the row is loaded
//       once and normalised; 64 of them become a word pair by ballot, kept in LDS with the first bit on top.  Then a lane
//       owns a run of 32 bits counted from the end of what a CRC covers (run_from_end), so that a whole number of words
//       lies behind it: it multiplies the run by x^(32 w) from the tables and reduces it modulo the transport block's
//       polynomial and modulo gCRC24B in one register loop each (mul_mod_word), and the lanes' remainders are
//       XOR-reduced with wave shuffles and LDS.
//         segment:    the payload bits of the block are copied to the row and the F filler bytes zeroed.  A block that is
//             not the last gets its CRC24B here.  The block's share of the transport block CRC -- its remainder times
//             x^(bits of B behind it) -- goes to part[r * frames + f]; the last block's CRC24B over its payload bits alone,
//             payload(x) x^(L_tb + 24) mod gB, to part[C * frames + f].
//         desegment:  the first K' bytes are read (never the fillers), the payload bits copied out, cb_ok set from the
//             remainder of the K' bits, and the remainder of the block's S bits times x^(bits of B behind it) put in part.
//   finish_kernel<SEGMENT>  a wave per transport block, grid = frames: XORs the C parts (XOR has no order, the result is
//       exact).  segment: writes the L_tb CRC bits into the last block and, when C > 1, that block's CRC24B = its part
//       XOR p(x) x^24 mod gB.  desegment: tb_ok = (the XOR is zero), and cb_ok with C = 1.
//   concatenate_kernel      [frames][G] bytes gathered from the packed rows; a thread owns four output bytes aligned to a
//       dword of the output, as in nr_rm_match_kernel.
//   split_kernel<T>         the inverse on floats or doubles, a thread per element.
// All stores are of one, four or eight bytes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nr_transport_block.h"

namespace ldpc {
namespace nrtb {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kStagedWords = 8448 / 32 + 1;  // the longest K', and the word run_from_end may read behind it

struct RowArgs {
  uint32_t a, s, k_prime, k, c, l_tb, l_cb;
  Poly g_tb;
  const uint32_t *table_tb, *table_cb, *behind;  // device_tables
  uint64_t batch, b0;
  uint32_t frames;
};

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
  return v;
}

// run w from the end of the row's first `cover` bits, times x^(32 w), modulo g
__device__ __forceinline__ uint32_t run_share(const uint32_t *staged, uint32_t w, uint32_t cover, const uint32_t *table, Poly g) {
  return 32 * w < cover ? mul_mod_word(run_from_end(staged, cover, w), table[w], g) : 0;
}

// segment: in = payload [batch][A], out = rows [C * batch][K].  desegment: in = rows, out = payload; cb_ok may be null.
// part: (C + 1) * frames words.
template <bool SEGMENT>
__global__ __launch_bounds__(kThreads) void rows_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                        uint32_t *__restrict__ part, uint8_t *__restrict__ cb_ok, RowArgs p) {
  __shared__ uint32_t staged[kStagedWords];
  __shared__ uint32_t partial[2][kThreads / 64];
  __shared__ uint32_t crc_shared;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t r = blockIdx.x / p.frames, f = blockIdx.x - r * p.frames;
  const uint64_t b = p.b0 + f;
  const uint64_t first = uint64_t(r) * p.s;  // the block's first bit in (payload, transport block CRC)
  const uint32_t carried = payload_bits_of_block(p.a, p.s, r);
  const uint8_t *payload_in = in + b * p.a + first;
  uint8_t *payload_out = out + b * p.a + first;
  const uint8_t *row_in = in + (uint64_t(r) * p.batch + b) * p.k;
  uint8_t *row_out = out + (uint64_t(r) * p.batch + b) * p.k;
  const uint32_t loaded = SEGMENT ? carried : p.k_prime;
  for (uint32_t q = tid; q < ((loaded + 63) & ~63u); q += kThreads) {
    bool bit = false;
    if (q < loaded) {
      if constexpr (SEGMENT) {
        bit = payload_in[q] == 1;
        row_out[q] = bit;
      } else {
        bit = row_in[q] == 1;
        if (q < carried) payload_out[q] = bit;
      }
    }
    const unsigned long long mask = __ballot(bit);
    if (lane == 0) {
      staged[q >> 5] = __brev(static_cast<uint32_t>(mask));
      staged[(q >> 5) + 1] = __brev(static_cast<uint32_t>(mask >> 32));
    }
  }
  if constexpr (SEGMENT)
    for (uint32_t q = p.k_prime + tid; q < p.k; q += kThreads) row_out[q] = 0;
  __syncthreads();
  // segment: both CRCs cover the payload bits carried.  desegment: the S bits of B, and all K' bits.
  const uint32_t cover_tb = SEGMENT ? carried : p.s;
  const uint32_t cover_cb = SEGMENT ? carried : p.k_prime;
  uint32_t acc_tb = 0, acc_cb = 0;
  for (uint32_t w = tid; 32 * w < loaded; w += kThreads) {
    acc_tb ^= run_share(staged, w, cover_tb, p.table_tb, p.g_tb);
    if (p.l_cb) acc_cb ^= run_share(staged, w, cover_cb, p.table_cb, kCrc24B);
  }
  acc_tb = wave_xor(acc_tb);
  acc_cb = wave_xor(acc_cb);
  if (lane == 0) {
    partial[0][wave] = acc_tb;
    partial[1][wave] = acc_cb;
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t tb = 0, cb = 0;
    for (uint32_t wv = 0; wv < kThreads / 64; wv++) {
      tb ^= partial[0][wv];
      cb ^= partial[1][wv];
    }
    tb = mul_mod(tb, p.behind[r], p.g_tb);
    const bool last = r + 1 == p.c;
    if constexpr (SEGMENT) {
      // the payload polynomial is multiplied by x^L_tb: behind[] counts the CRC bits for every block but the last
      if (last) tb = rem_shift(tb, p.l_tb, p.g_tb);
      if (p.l_cb) {
        cb = rem_shift(cb, p.s - carried + 24, kCrc24B);
        if (last) part[size_t(p.c) * p.frames + f] = cb;
      }
    } else if (p.l_cb && cb_ok) {
      cb_ok[b * p.c + r] = cb == 0;
    }
    part[size_t(r) * p.frames + f] = tb;
    crc_shared = cb;
  }
  if constexpr (SEGMENT) {
    __syncthreads();
    if (p.l_cb && r + 1 != p.c && tid < 24) row_out[p.s + tid] = static_cast<uint8_t>((crc_shared >> (23 - tid)) & 1u);
  }
}

// segment: out = rows.  desegment: out = tb_ok [batch].  grid = frames, 64 threads.
template <bool SEGMENT>
__global__ __launch_bounds__(64) void finish_kernel(const uint32_t *__restrict__ part, uint8_t *__restrict__ out,
                                                    uint8_t *__restrict__ cb_ok, RowArgs p) {
  const uint32_t f = blockIdx.x, lane = threadIdx.x;
  const uint64_t b = p.b0 + f;
  uint32_t v = 0;
  for (uint32_t r = lane; r < p.c; r += 64) v ^= part[size_t(r) * p.frames + f];
  v = wave_xor(v);
  if constexpr (SEGMENT) {
    uint8_t *row = out + (uint64_t(p.c - 1) * p.batch + b) * p.k;
    const uint32_t carried = payload_bits_of_block(p.a, p.s, p.c - 1);
    if (lane < p.l_tb) row[carried + lane] = static_cast<uint8_t>((v >> (p.l_tb - 1 - lane)) & 1u);
    if (p.l_cb) {
      const uint32_t cb = part[size_t(p.c) * p.frames + f] ^ rem_shift(v, 24, kCrc24B);
      if (lane < 24) row[p.s + lane] = static_cast<uint8_t>((cb >> (23 - lane)) & 1u);
    }
  } else if (lane == 0) {
    out[b] = v == 0;
    if (p.l_cb == 0 && cb_ok) cb_ok[b] = v == 0;
  }
}

__device__ __forceinline__ uint32_t packed_bit(const uint8_t *in, const Packing &p, uint32_t idx) {
  return in[packed_index(p, idx)] == 1 ? 1u : 0u;
}

// grid = ceil((total + shift) / 4 / kThreads); out = the pass's first output byte, shift = the low two bits of its address
__global__ __launch_bounds__(kThreads) void concatenate_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, uint32_t total,
                                                               uint32_t shift, Packing p) {
  const int64_t g0 = 4 * int64_t(blockIdx.x * kThreads + threadIdx.x) - shift;
  if (g0 >= int64_t(total)) return;
  if (g0 >= 0 && g0 + 3 < int64_t(total)) {
    const uint32_t g = static_cast<uint32_t>(g0);
    const uint32_t w = packed_bit(in, p, g) | packed_bit(in, p, g + 1) << 8 | packed_bit(in, p, g + 2) << 16 | packed_bit(in, p, g + 3) << 24;
    *reinterpret_cast<uint32_t *>(out + g) = w;
    return;
  }
  for (int64_t g = g0 < 0 ? 0 : g0; g < g0 + 4 && g < int64_t(total); g++) out[g] = static_cast<uint8_t>(packed_bit(in, p, static_cast<uint32_t>(g)));
}

// in = the pass's first received value, out = the packed array.  grid = ceil(total / kThreads)
template <typename T>
__global__ __launch_bounds__(kThreads) void split_kernel(const T *__restrict__ in, T *__restrict__ out, uint32_t total, Packing p) {
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  if (g >= total) return;
  out[packed_index(p, g)] = in[g];
}

}  // namespace nrtb
}  // namespace ldpc
