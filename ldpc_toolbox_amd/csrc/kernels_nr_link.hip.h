// Kernels of the NR link handle (nr_link.h, device_nr_link.h).  The HARQ slots' rows are block-major over the handle's
// slots: row r * slots + slot is block r of the slot; done flags and iteration counts are [slots][C].  A call covers the
// slots first_slot .. first_slot + batch - 1, and its own rows are block-major over the call: row r * batch + b.
// Plain loads and stores only; every element has one owner, so nothing depends on the order of the threads.
//
//   recover_kernel       the fused de-concatenation and rate recovery: rx [batch][G] demapper LLRs -> the slots' soft rows.  A
//       thread owns one (transport block, block r, column) of a pass (nr_link.h, Pass): it finds E_r and where block r
//       begins in the transport block's row of G, and then does what nr_rm_recover_kernel<float> does with the plan of that
//       length -- the filler LLR, the left-to-right sum of the column's repeats in ascending selection index, old + S when
//       combining -- through the same functions of nr_rate_match.h.  When combining it leaves a done block alone.
//   recover_i8_kernel    the same into 8-bit soft rows (include/ldpc_toolbox.h, PART 12): rx [batch][G] demapper soft bits at any
//       byte address.  A thread owns four consecutive columns of one (transport block, block) soft row and stores one dword,
//       which it loads first when combining, as in nr_rm_recover_i8_kernel; every column is nrrm::recover_i8_value, the
//       per-column body of that kernel.
//   active_list_kernel   one wave: the call's rows whose block is not done, as slot rows in ascending call row, by ballot
//       and prefix count; their number in *count.
//   gather_soft_kernel   the listed soft rows -> dense decoder input [count][n]; a workgroup per row, 16 bytes per lane.  A
//       copy: it moves float rows and the 8-bit rows whose n is a multiple of 16 alike.
//   gather_soft_dword_kernel  the same with 4 bytes per lane, for 8-bit rows that begin on a dword only (n = 260 at Zc = 5).
//   scatter_hard_kernel  the decoder's [count][K] hard decisions and [count] iteration counts -> the listed slots.
//   gather_hard_kernel   the slots' hard decisions of the call -> dense [C * batch][K], what desegment takes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_nr_rm.hip.h"
#include "nr_link.h"
#include "nr_rate_match.h"

namespace ldpc {
namespace nrlink {

constexpr uint32_t kThreads = 256;

struct SlotArgs {
  uint32_t c, slots, first_slot, batch;
};

// grid = ceil(pass.total / kThreads).  rx: the call's first row; soft, done: the handle's.
__global__ __launch_bounds__(kThreads) void recover_kernel(const float *__restrict__ rx, float *__restrict__ soft,
                                                           const uint8_t *__restrict__ done, Geometry k, Pass pass, SlotArgs sl,
                                                           nrrm::Plan p_lo, nrrm::Plan p_hi, float filler, int32_t combine) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= pass.total) return;
  const Element el = element_of(k, pass.within + i);
  const uint64_t b = pass.tb0 + el.tb;  // transport block of the call
  const uint64_t slot = sl.first_slot + b;
  if (combine && done[slot * k.c + el.r] != 0) return;
  // the plan of the block's length: the two are of one configuration, rv and Qm, and differ in E alone -- three selects
  // per lane, where a choice between the two structs would load every field per lane
  nrrm::Plan p = p_lo;
  if (el.r >= k.c_lo) {
    p.e = p_hi.e;
    p.cols = p_hi.cols;
    p.div_cols = p_hi.div_cols;
  }
  float *out = soft + (uint64_t(el.r) * sl.slots + slot) * k.n + el.column;
  const uint32_t r = nrrm::first_selection_of_column(p, el.column);
  if (r == nrrm::kFiller) {
    *out = filler;
    return;
  }
  if (r >= p.e) {  // (kNotSent included)
    if (!combine) *out = 0.0f;
    return;
  }
  const float *row = rx + b * k.g + start_of_block(k, el.r);
  float s = row[nrrm::position_of_selection(p, r)];
  for (uint32_t j = r + p.l; j < p.e; j += p.l) s = s + row[nrrm::position_of_selection(p, j)];
  *out = combine ? *out + s : s;
}

// grid = ceil(pass.total / 4 / kThreads); pass.within and pass.total are multiples of 4 (nrlink::dword_pass_elements).  n is a
// multiple of 4 and the slot array begins on 256 bytes, so every soft row begins on a dword and the four columns of a
// thread lie in one block of one transport block: one done flag, one plan, one received row.
__global__ __launch_bounds__(kThreads) void recover_i8_kernel(const int8_t *__restrict__ rx, int8_t *soft, const uint8_t *__restrict__ done,
                                                              Geometry k, Pass pass, SlotArgs sl, nrrm::Plan p_lo, nrrm::Plan p_hi,
                                                              int32_t filler, int32_t combine) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= pass.total / 4) return;
  const Element el = element_of(k, pass.within + 4 * i);
  const uint64_t b = pass.tb0 + el.tb;  // transport block of the call
  const uint64_t slot = sl.first_slot + b;
  if (combine && done[slot * k.c + el.r] != 0) return;
  nrrm::Plan p = p_lo;  // (as in recover_kernel)
  if (el.r >= k.c_lo) {
    p.e = p_hi.e;
    p.cols = p_hi.cols;
    p.div_cols = p_hi.div_cols;
  }
  uint32_t *out = reinterpret_cast<uint32_t *>(soft + (uint64_t(el.r) * sl.slots + slot) * k.n + el.column);
  const int8_t *row = rx + b * k.g + start_of_block(k, el.r);
  const uint32_t old = combine ? *out : 0u;
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int v = nrrm::recover_i8_value(row, p, el.column + j, filler, combine, static_cast<int8_t>(old >> (8 * j)));
    w |= uint32_t(static_cast<uint8_t>(v)) << (8 * j);
  }
  *out = w;
}

// <<<1, 64>>>.  list: room for C * batch words.  C * batch < 2^31.
__global__ __launch_bounds__(64) void active_list_kernel(const uint8_t *__restrict__ done, uint32_t *__restrict__ list,
                                                         uint32_t *__restrict__ count, SlotArgs sl, dev::FastDiv div_batch) {
  const uint32_t lane = threadIdx.x;
  const uint32_t rows = sl.c * sl.batch;
  uint32_t found = 0;
  for (uint32_t i0 = 0; i0 < rows; i0 += 64) {
    const uint32_t i = i0 + lane;
    uint32_t slot_row = 0;
    bool active = false;
    if (i < rows) {
      const uint32_t r = dev::fdiv_q(i, div_batch), slot = sl.first_slot + (i - r * sl.batch);
      slot_row = r * sl.slots + slot;
      active = done[uint64_t(slot) * sl.c + r] == 0;
    }
    const unsigned long long mask = __ballot(active);
    if (active) list[found + __popcll(mask & ((1ull << lane) - 1ull))] = slot_row;
    found += __popcll(mask);
  }
  if (lane == 0) *count = found;
}

// grid = count; n4 = n / 4 (n is 52 Zc or 68 Zc, and every row begins on 16 bytes)
__global__ __launch_bounds__(kThreads) void gather_soft_kernel(const float4 *__restrict__ soft, const uint32_t *__restrict__ list,
                                                               float4 *__restrict__ dense, uint32_t n4) {
  const float4 *from = soft + uint64_t(list[blockIdx.x]) * n4;
  float4 *to = dense + uint64_t(blockIdx.x) * n4;
  for (uint32_t j = threadIdx.x; j < n4; j += kThreads) to[j] = from[j];
}

// grid = count; n1 = n / 4 for 8-bit rows (every row begins on a dword)
__global__ __launch_bounds__(kThreads) void gather_soft_dword_kernel(const uint32_t *__restrict__ soft, const uint32_t *__restrict__ list,
                                                                     uint32_t *__restrict__ dense, uint32_t n1) {
  const uint32_t *from = soft + uint64_t(list[blockIdx.x]) * n1;
  uint32_t *to = dense + uint64_t(blockIdx.x) * n1;
  for (uint32_t j = threadIdx.x; j < n1; j += kThreads) to[j] = from[j];
}

// grid = count.  hard: the slots' [C * slots][K]; iterations: the slots' [slots][C]
__global__ __launch_bounds__(kThreads) void scatter_hard_kernel(const uint8_t *__restrict__ bits, const int32_t *__restrict__ its,
                                                                const uint32_t *__restrict__ list, uint8_t *__restrict__ hard,
                                                                int32_t *__restrict__ iterations, uint32_t k_len, SlotArgs sl,
                                                                dev::FastDiv div_slots) {
  const uint32_t slot_row = list[blockIdx.x];
  const uint8_t *from = bits + uint64_t(blockIdx.x) * k_len;
  uint8_t *to = hard + uint64_t(slot_row) * k_len;
  for (uint32_t j = threadIdx.x; j < k_len; j += kThreads) to[j] = from[j];
  if (threadIdx.x == 0) {
    const uint32_t r = dev::fdiv_q(slot_row, div_slots);
    iterations[uint64_t(slot_row - r * sl.slots) * sl.c + r] = its[blockIdx.x];
  }
}

// grid = C * batch: call row r * batch + b <- slot row r * slots + first_slot + b
__global__ __launch_bounds__(kThreads) void gather_hard_kernel(const uint8_t *__restrict__ hard, uint8_t *__restrict__ dense, uint32_t k_len,
                                                               SlotArgs sl, dev::FastDiv div_batch) {
  const uint32_t r = dev::fdiv_q(blockIdx.x, div_batch);
  const uint8_t *from = hard + (uint64_t(r) * sl.slots + sl.first_slot + (blockIdx.x - r * sl.batch)) * k_len;
  uint8_t *to = dense + uint64_t(blockIdx.x) * k_len;
  for (uint32_t j = threadIdx.x; j < k_len; j += kThreads) to[j] = from[j];
}

}  // namespace nrlink
}  // namespace ldpc
