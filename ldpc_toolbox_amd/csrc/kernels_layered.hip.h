// Layered schedule: one launch per dependency level (two-pass and register-resident rows), the flooding Tanh rule's
// register-resident rows (cn_reg_kernel: the same row handling), layered min-sum (streaming, register-resident, row records).
// Part of kernels.hip.h (include that).
#pragma once
namespace ldpc {
namespace dev {

// ---------------------------------------------------------------------------------------
// Layered schedule: one dependency level (rows that share no variable, so their serial
// order in horizontal_layered.rs:105-110 is immaterial).  In-place update of Qv and R.
//   Phi / Aminstar:                 R = out; Qv = x + out      (arithmetic.rs:284-291, 1052-1065)
//   Tanh / Minstarapprox / Minsum:  Qv += out - R; R = out     (arithmetic.rs:423-424, 570-573)
// The update pass re-reads Qv and R (L1/L2 hits: the same wave loaded them a moment ago)
// instead of keeping them in LDS, which would halve the occupancy.
// dynamic LDS: 2 * dmax * blockDim.x * sizeof(T)
// ---------------------------------------------------------------------------------------
// (f64: launched with at most 256 threads; telling the compiler so lifts its register cap from 128, where the 24-edge
// register-resident variants spilled up to 65 registers to scratch.  f32 keeps the default bound: its variants fit.)
#define LDPC_HL_BOUNDS(T) __launch_bounds__(sizeof(T) == 8 ? 256 : 1024)
// (register-resident f32 rows of at most 10 edges: 8 waves per SIMD asked for -- 64 registers -- where the compiler by
// itself stops at 67-71 and 7 waves: config 3 35.2k -> 35.9k cw/s fixed work, 328k -> 340k at +2 dB, HLPhif32 +2 %.
// Aminstar and Minstarapprox would spill for no gain (Minstarapprox: 0.211 -> 0.195 of the roofline) and keep the
// compiler's choice, as do the 12-edge variants (up to 17 registers spilled at 64; no BASELINE graph has such levels).
// A 20-edge bucket at 5-6 waves measured equal to the 24-edge one.)
#define LDPC_HL_REG_BOUNDS(RULE, T, DMAX)                               \
  __launch_bounds__(sizeof(T) == 8 ? 256 : (DMAX <= 12 ? 256 : 1024),   \
                    (sizeof(T) == 4 && DMAX <= 10 && RULE != kRuleAminstar && RULE != kRuleMinstarapprox) ? 8 : 1)

// hl_level_kernel for levels whose rows have at most DMAX edges: the row's Qv and R values are
// loaded into registers in one burst (all loads of the row in flight together, R nontemporal) and
// kept for the update, so there is no second pass over global memory; only the rule's inputs and
// outputs go through the LDS columns (the rules index them dynamically).  With trivial arithmetic
// the two-pass form takes 275 us per BG1 level where the streaming min-sum kernel takes 80: the
// staged structure -- three short load bursts, then three more for the update, at four waves per
// SIMD -- was the cost, not the transcendental functions.
// The rows come as records (slice_tasks.h, build_level_recs: first edge, degree, the edges' variables, 16 or 32 words
// per row in level order): one scalar load per row where the chain level_rows -> row_ptr -> edge_col took four dependent
// ones, and the record is simply loaded again for the update, so the variables' offsets are not held in scalar
// registers across the rule (at 8 waves per SIMD the compiler otherwise parks them in a vector register's lanes).
// f(i) for a row's slots i in [0, d).  Rows of at most 12 edges: one straight-line block per degree behind a switch
// (the chain of `if (i < d)` blocks made the compiler keep its ten conditions as 64-bit masks in scalar registers, and
// at 8 waves per SIMD it then parks scalar registers in a vector register's lanes).  Longer rows keep the chain: a
// block per degree would be the larger cost there.
template <typename F, int... I>
__device__ __forceinline__ void slots_seq(F &&f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int D, typename F>
__device__ __forceinline__ void slots_upto(F &&f) {
  slots_seq(f, std::make_integer_sequence<int, D>{});
}
template <typename F, int... I>
__device__ __forceinline__ void slots_below(uint32_t d, F &&f, std::integer_sequence<int, I...>) {
  ((uint32_t(I) < d ? (f(std::integral_constant<int, I>{}), 0) : 0), ...);
}
template <int DMAX, typename F>
__device__ __forceinline__ void for_slots(uint32_t d, F &&f) {
  if constexpr (DMAX <= 12) {
#define LDPC_DEG_CASE(k) \
  case k:                \
    if constexpr (DMAX >= k) slots_upto<k>(f); \
    break;
    switch (d) {
      LDPC_DEG_CASE(1) LDPC_DEG_CASE(2) LDPC_DEG_CASE(3) LDPC_DEG_CASE(4) LDPC_DEG_CASE(5) LDPC_DEG_CASE(6)
      LDPC_DEG_CASE(7) LDPC_DEG_CASE(8) LDPC_DEG_CASE(9) LDPC_DEG_CASE(10) LDPC_DEG_CASE(11) LDPC_DEG_CASE(12)
      default:
        break;
    }
#undef LDPC_DEG_CASE
  } else {
    slots_below(d, f, std::make_integer_sequence<int, DMAX>{});
  }
}
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
typedef const u32x16 __attribute__((address_space(4))) *RecPtr;
template <int DMAX>
__device__ __forceinline__ uint32_t rec_word(const u32x16 &w0, const u32x16 &w1, int i) {
  return i < 16 ? w0[i & 15] : w1[i & 15];
}

// Flooding check nodes (the Tanh rule), rows of at most DMAX edges in registers: cn_staged_kernel with hl_level_reg_kernel's row
// handling -- one record per row (slice_tasks.h, build_level_recs over all rows in order: first edge, degree, variables),
// the row's posterior and message values loaded in one burst through buffer descriptors, a straight-line block per degree.
// Same arithmetic per row as cn_staged_kernel (flooding.rs:95-127): x_i = L - c2v_old (the channel value in the first
// iteration), parity of the hard decisions, rule, new messages.
#define LDPC_CN_REG_BOUNDS(T, DMAX) __launch_bounds__(256, (sizeof(T) == 4 && DMAX <= 10) ? 8 : 1)
template <int RULE, typename T, int DMAX, bool FIRST>
__global__ LDPC_CN_REG_BOUNDS(T, DMAX) void cn_reg_kernel(Graph g, Sched sc, State st, const uint32_t *__restrict__ row_recs,
                              const T *__restrict__ L, T *__restrict__ msg, uint32_t *__restrict__ unsat_out, uint32_t dmax) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (group_finished(st)) return;
  constexpr uint32_t kRecVecs = DMAX <= 12 ? 1 : 2;
  const RecPtr recs = (RecPtr)row_recs;
  const uint32_t n_rows = g.n_rows, waves_per_chunk = sc.waves_per_chunk, tile = sc.tile;
  const uint32_t S = blockDim.x;
  T *A = reinterpret_cast<T *>(smem) + threadIdx.x;
  T *B = A + size_t(dmax) * S;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uniform((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  uint32_t chunk, node0;
  wave_slot(sc, wave, &chunk, &node0);
  if (chunk >= sc.nchunks) return;
  const uint32_t b0 = chunk * 64;
  if (b0 >= *st.n_slots) return;
  const size_t off = size_t(b0) + lane;
  if (__builtin_amdgcn_ballot_w64(st.done[off] == 0) == 0) return;
  const uint32_t row_bytes = tile * uint32_t(sizeof(T)), lane_off = lane * uint32_t(sizeof(T));
  const size_t tl = tile_base(b0, g.n_cols, sc), tm = tile_base(b0, g.n_edges, sc);
  const RowBuf Lb = row_buf(L + tl, uint64_t(g.n_cols) * row_bytes - in_tile_of(b0, sc) * sizeof(T));
  const RowBuf Mb = row_buf(msg + tm, uint64_t(g.n_edges) * row_bytes - in_tile_of(b0, sc) * sizeof(T));
  uint32_t odd_acc = 0;
  for (uint32_t c = node0; c < n_rows; c += waves_per_chunk) {
    u32x16 w0 = recs[c * kRecVecs], w1 = w0;
    if constexpr (kRecVecs == 2) w1 = recs[c * kRecVecs + 1];
    const uint32_t d = w0[1];
    if (d == 0) continue;
    const uint32_t moff = w0[0] * row_bytes;
    T lv[DMAX], mv[DMAX];
    for_slots<DMAX>(d, [&](auto slot) {
      constexpr int i = decltype(slot)::value;
      lv[i] = row_load<T, false>(Lb, lane_off, rec_word<DMAX>(w0, w1, i + 2) * row_bytes);
      if (!FIRST) mv[i] = row_load<T, true>(Mb, lane_off, moff + uint32_t(i) * row_bytes);  // streamed once
    });
    uint32_t par = 0;
    for_slots<DMAX>(d, [&](auto slot) {
      constexpr int i = decltype(slot)::value;
      A[i * S] = FIRST ? lv[i] : (lv[i] - mv[i]);
      if (lv[i] <= T(0.0)) par ^= 1u;
    });
    odd_acc |= par;
    const T *out = rule_check_node<RULE, T>(A, B, d, S);
    for_slots<DMAX>(d, [&](auto slot) {
      constexpr int i = decltype(slot)::value;
      row_store<T, true>(Mb, lane_off, moff + uint32_t(i) * row_bytes, out[i * S]);
    });
  }
  if (!FIRST && odd_acc) unsat_out[off] = 1u;
}





// The level kernels min-sum can take (hl_level, hl_level_reg, hl_minsum, hl_minsum_reg, hl_minsum_rec): kernels_layered_minsum.inc, once plain and once as the normalized / offset
// min-sum forms (*_kernel_corr) -- see the head of that file
#define LDPC_MINSUM_CORR 0
#define LDPC_MS_KERNEL(x) x##_kernel
#define LDPC_MS_PARAM(T)
#define LDPC_MS_ARG
#include "kernels_layered_minsum.inc"
#undef LDPC_MINSUM_CORR
#undef LDPC_MS_KERNEL
#undef LDPC_MS_PARAM
#undef LDPC_MS_ARG
#define LDPC_MINSUM_CORR 1
#define LDPC_MS_KERNEL(x) x##_kernel_corr
#define LDPC_MS_PARAM(T) , MinsumCorr<T> mc = MinsumCorr<T>{}
#define LDPC_MS_ARG , mc
#include "kernels_layered_minsum.inc"
#undef LDPC_MINSUM_CORR
#undef LDPC_MS_KERNEL
#undef LDPC_MS_PARAM
#undef LDPC_MS_ARG

}  // namespace dev
}  // namespace ldpc
