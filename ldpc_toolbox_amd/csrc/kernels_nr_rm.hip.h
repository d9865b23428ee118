// Kernels of 5G NR rate matching and rate recovery (nr_rate_match.h, device_nr_rm.h).  Both are streams over one pass of
// frames: the element index g < total < 2^31 runs over the pass's output, and every division -- by the row length, L,
// E/Qm and Qm -- is by a launch-invariant value and goes through FastDiv.  Plain loads and stores only.
//
//   nr_rm_match_kernel       bits [frames][n] -> [frames][E].  A thread owns four consecutive output bytes, aligned to a
//       dword of the output (a pass need not begin on one: `shift` bytes of the first dword lie before it), gathers their
//       four codeword bytes and stores one dword; the threads at the two ends store bytes.
//   nr_rm_recover_kernel<T>  rx [frames][E] -> llrs [frames][n].  A thread owns one (frame, column): a filler column gets
//       the filler LLR; any other the sum of its repeats in ascending selection index, each sum rounded once, on top of
//       the old value when `combine` is set; a column no repeat carries keeps the old value or becomes +0.
//   nr_rm_recover_i8_kernel  the same on 8-bit soft bits with saturating sums: four output bytes per thread, as in the match
//       kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nr_rate_match.h"
#include "soft_i8.h"

namespace ldpc {
namespace nrrm {

constexpr uint32_t kThreads = 256;

__device__ __forceinline__ uint32_t match_bit(const uint8_t *in, const Plan &p, const FastDiv &div_e, uint32_t g) {
  const uint32_t frame = dev::fdiv_q(g, div_e);
  return in[size_t(frame) * p.n + column_of_position(p, g - frame * p.e)] == 1 ? 1u : 0u;
}

// grid = ceil((total + shift) / 4 / kThreads); shift = the low two bits of `out`'s address
__global__ __launch_bounds__(kThreads) void nr_rm_match_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, uint32_t total,
                                                               uint32_t shift, Plan p, FastDiv div_e) {
  const int64_t g0 = 4 * int64_t(blockIdx.x * kThreads + threadIdx.x) - shift;
  if (g0 >= int64_t(total)) return;
  if (g0 >= 0 && g0 + 3 < int64_t(total)) {
    const uint32_t g = static_cast<uint32_t>(g0);
    const uint32_t w = match_bit(in, p, div_e, g) | match_bit(in, p, div_e, g + 1) << 8 | match_bit(in, p, div_e, g + 2) << 16 |
                       match_bit(in, p, div_e, g + 3) << 24;
    *reinterpret_cast<uint32_t *>(out + g) = w;
    return;
  }
  for (int64_t g = g0 < 0 ? 0 : g0; g < g0 + 4 && g < int64_t(total); g++)
    out[g] = static_cast<uint8_t>(match_bit(in, p, div_e, static_cast<uint32_t>(g)));
}

// grid = ceil(total / kThreads), total = frames * n
template <typename T>
__global__ __launch_bounds__(kThreads) void nr_rm_recover_kernel(const T *__restrict__ rx, T *__restrict__ llrs, uint32_t total, Plan p,
                                                                 FastDiv div_n, T filler, int32_t combine) {
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  if (g >= total) return;
  const uint32_t frame = dev::fdiv_q(g, div_n);
  const uint32_t r = first_selection_of_column(p, g - frame * p.n);
  if (r == kFiller) {
    llrs[g] = filler;
    return;
  }
  if (r >= p.e) {  // (kNotSent included)
    if (!combine) llrs[g] = T(0);
    return;
  }
  const T *row = rx + size_t(frame) * p.e;
  T s = row[position_of_selection(p, r)];
  for (uint32_t j = r + p.l; j < p.e; j += p.l) s = s + row[position_of_selection(p, j)];
  llrs[g] = combine ? llrs[g] + s : s;
}

// ---- 8-bit soft bits (include/ldpc_toolbox.h, PART 9; soft_i8.h) --------------------------------------------------------

// The soft bit of one column of a soft row, which every 8-bit recover kernel computes through this function (the link
// handle's fused one, kernels_nr_link.hip.h, included).  row: the E received bytes of the column's frame or block, at any
// byte address, read only where a selection index carries the column; old: the byte there now (read only when `combine` is
// set).  The filler; else clip(old) or 0 on top of the left-to-right saturating sum of the column's repeats in ascending
// selection index, every received byte clipped first.
__device__ __forceinline__ int recover_i8_value(const int8_t *__restrict__ row, const Plan &p, uint32_t column, int filler, int32_t combine,
                                                int old) {
  const uint32_t r = first_selection_of_column(p, column);
  if (r == kFiller) return filler;
  const int kept = combine ? soft::soft_clip(old) : 0;
  if (r >= p.e) return kept;  // (kNotSent included)
  int s = soft::soft_clip(row[position_of_selection(p, r)]);
  for (uint32_t j = r + p.l; j < p.e; j += p.l) s = soft::soft_accumulate(s, soft::soft_clip(row[position_of_selection(p, j)]));
  return combine ? soft::soft_accumulate(kept, s) : s;
}

// the soft bit of output element g of the pass
__device__ __forceinline__ int recover_i8_column(const int8_t *__restrict__ rx, const Plan &p, const FastDiv &div_n, uint32_t g,
                                                 int filler, int32_t combine, int old) {
  const uint32_t frame = dev::fdiv_q(g, div_n);
  return recover_i8_value(rx + size_t(frame) * p.e, p, g - frame * p.n, filler, combine, old);
}

// rx [frames][E] -> llrs [frames][n], one byte per soft bit.  A thread owns four consecutive output bytes, aligned to a dword
// of the output as in nr_rm_match_kernel (`shift`: the low two bits of `llrs`' address): it computes their four columns, each
// a saturating left-to-right sum of its repeats, loads the old dword when `combine` is set and stores one dword; the threads
// at the two ends load and store bytes.  No atomics: a column belongs to one thread.
// grid = ceil((total + shift) / 4 / kThreads), total = frames * n
__global__ __launch_bounds__(kThreads) void nr_rm_recover_i8_kernel(const int8_t *__restrict__ rx, int8_t *llrs, uint32_t total,
                                                                    uint32_t shift, Plan p, FastDiv div_n, int32_t filler, int32_t combine) {
  const int64_t g0 = 4 * int64_t(blockIdx.x * kThreads + threadIdx.x) - shift;
  if (g0 >= int64_t(total)) return;
  if (g0 >= 0 && g0 + 3 < int64_t(total)) {
    const uint32_t g = static_cast<uint32_t>(g0);
    const uint32_t old = combine ? *reinterpret_cast<const uint32_t *>(llrs + g) : 0u;
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int v = recover_i8_column(rx, p, div_n, g + k, filler, combine, static_cast<int8_t>(old >> (8 * k)));
      w |= uint32_t(static_cast<uint8_t>(v)) << (8 * k);
    }
    *reinterpret_cast<uint32_t *>(llrs + g) = w;
    return;
  }
  for (int64_t g = g0 < 0 ? 0 : g0; g < g0 + 4 && g < int64_t(total); g++)
    llrs[g] = static_cast<int8_t>(recover_i8_column(rx, p, div_n, static_cast<uint32_t>(g), filler, combine, combine ? llrs[g] : 0));
}

}  // namespace nrrm
}  // namespace ldpc
