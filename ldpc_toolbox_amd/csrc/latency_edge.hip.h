// Small-batch (latency) path with the lanes across the EDGES of one codeword: the horizontal-layered schedule
// (every float rule) and the flooding schedule of the sum-product family (Phi, Tanh, Minstarapprox, Aminstar; flooding
// min-sum in f32 has the row-lane kernel of latency.hip.h), f32 and f64 arithmetic, and the 8-bit rules on both schedules.  The reference's own call pattern
// is ONE codeword per decode call (/root/reference/src/c_api/decoder.rs:50-67, src/simulation/ber.rs:462-466) -- and
// the decoder its command line defaults to is flooding Phif64 (src/cli/ber.rs:49) -- which through the batched kernels
// costs one launch per dependency level or two per flooding iteration with 1 lane in 64 useful.  Here, as in
// latency.hip.h:
//
//   * one persistent launch per call; a codeword is owned by one XCD (its soft values and messages stay in that
//     XCD's L2); up to 8 codewords of a call decode concurrently, one per XCD, and larger calls give every XCD a
//     BUNDLE of up to 8 codewords that share each phase and each barrier (64 codewords in about the time of 8);
//   * a LANE owns one EDGE of one row.  Rows are packed, whole, into wavefront-sized chunks of at most 64 edge
//     lanes; a row's d lanes sit next to each other in one wavefront and exchange their inputs with ds_bpermute (no
//     LDS memory, no workgroup barrier).  Every lane evaluates the reference's rule for ITS output only -- out_i is
//     a fold over the other inputs in slot order in every rule (arithmetic.rs:214-246, 347-379, 487-521, 942-999),
//     so the per-lane folds perform exactly the operations the row-at-a-time evaluation of kernels.hip.h
//     (rule_check_node) performs for that output: bit-identical results, with the O(d^2) work of a row spread over d
//     lanes and the transcendental function of an input evaluated once, by its own lane;
//   * messages are stored in lane order ([chunk][lane]): every access of the check side is a coalesced segment and
//     only ever written by the lane that owns it; soft values are gathered / scattered by variable index.  Data that
//     crosses a barrier is written with plain (write-through) stores and read with nontemporal loads (latency.hip.h);
//   * LAYERED: the rows of a dependency level share no variable, so their in-place updates commute
//     (horizontal_layered.rs:105-110 processes rows 0..m in order; device_decoder.hip builds the levels): a level is
//     one parallel step, levels are separated by the XCD-local barrier of latency.hip.h; the syndrome of hard(Qv)
//     after every iteration (:66-78);
//   * FLOODING (flooding.rs:51-125): check-node phase over all rows -- x = L - c2v is the variable node's own
//     subtraction (arithmetic.rs:152), evaluated by the consumer as in the batched kernels -- with the row parities of
//     hard(L) of the previous iteration fused in (the convergence vote rides on the barrier); variable-node phase with
//     a lane per variable: the slot-ordered sum from -0.0 (arithmetic.rs:140-156).  Two barriers per iteration.
//
// Per-codeword semantics are those of the batch path: pre-check on the raw input (iterations 0), stop at the first
// zero syndrome, -1 after max_iterations with the last hard decisions, the max_iterations = 0 corners.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "kernels.hip.h"
#include "kernels_i8.hip.h"
#include "latency.hip.h"

namespace ldpc {
namespace dev {

struct EdgeLatTables {
  uint32_t n, m, n_levels, n_chunks;
  const uint32_t *level_chunk;  // [n_levels+1] first chunk of a level (flooding: one level, all rows)
  const uint32_t *lane_var;     // [n_chunks*64] variable of the lane's edge, kNoLane for padding
  const uint32_t *lane_info;    // [n_chunks*64] slot of the edge in its row | degree of the row << 8 | largest degree in the chunk << 16
  const uint32_t *var_ptr;      // flooding: [n+1] slots of variable v in var_lane
  const uint32_t *var_lane;     // flooding: [E] lane index (chunk * 64 + lane) of the variable's j-th edge, cols[v] order
  const int32_t *src_block;     // depuncture map or null
  uint32_t block_size;
};
enum : uint32_t { kNoLane = 0xFFFFFFFFu };

struct EdgeLatState {  // 8 XCDs x kEdgeBundle codeword slots carved from one allocation: soft | msg | chan | rawhard
  char *base;
  size_t slot_bytes, off_msg, off_chan, off_rawhard;
  uint32_t *flags;  // [8 XCDs][2][kEdgeBundle] convergence votes of the bundled codewords (zeroed before every launch)
};

template <typename T>
__device__ __forceinline__ T lat_ld(const T *p) {
  return __builtin_nontemporal_load(p);  // bypasses the CU's L1: served by the XCD's L2
}

// the lane's output: the rule's fold over the OTHER inputs of its row, in slot order.
//   x     this lane's input (Qv - R)
//   first lane index (in the wavefront) of the row's slot 0;  i, d: this lane's slot and the row's degree
//   dmax  largest degree among the wavefront's rows (wave-uniform trip count)
// Inactive lanes (padding) pass d = 0 and take part in the exchanges only.
// mc: read by kRuleMinsumCorr only (normalized / offset min-sum: kernels_common.hip.h, MinsumCorr)
template <int RULE, typename T>
__device__ __forceinline__ T rule_edge(T x, uint32_t first, uint32_t i, uint32_t d, uint32_t dmax,
                                       const MinsumCorr<T> &mc = MinsumCorr<T>{}) {
  const int src0 = static_cast<int>(first);
  if constexpr (RULE == kRuleTanh) {
    // arithmetic.rs:347-379
    const T c = Limits<T>::tanh_clamp;
    T h = T(0.5) * x;
    if (h < -c) h = -c;
    if (h > c) h = c;
    const T t = m_tanh_clamped(h);
    T product = T(1.0);
    for (uint32_t j = 0; j < dmax; j++) {
      const T tj = __shfl(t, src0 + static_cast<int>(j), 64);
      if (j < d && j != i) product *= tj;
    }
    return two_atanh(product);
  } else if constexpr (RULE == kRulePhi) {
    // arithmetic.rs:214-246
    const T p = phi_fn(m_abs(x));
    const uint32_t neg = x < T(0.0) ? 1u : 0u;
    T sum = T(0.0);
    uint32_t sign = 0;
    for (uint32_t j = 0; j < dmax; j++) {
      const T pj = __shfl(p, src0 + static_cast<int>(j), 64);
      const uint32_t nj = static_cast<uint32_t>(__shfl(static_cast<int>(neg), src0 + static_cast<int>(j), 64));
      if (j < d) {
        sum += pj;
        sign ^= nj;
      }
    }
    const T y = phi_fn(sum - p);
    const uint32_t s = neg ? (sign ^ 1u) : sign;
    return s == 0 ? y : -y;
  } else if constexpr (RULE == kRuleMinstarapprox || RULE == kRuleMinsum || RULE == kRuleMinsumCorr) {
    // arithmetic.rs:487-521 (Minsum: SURVEY.md Appendix A.6)
    constexpr bool kMinsum = RULE == kRuleMinsum || RULE == kRuleMinsumCorr;
    uint32_t sign = 0;
    bool have = kMinsum;
    T acc = kMinsum ? Limits<T>::inf() : T(0.0);
    for (uint32_t j = 0; j < dmax; j++) {
      T v = __shfl(x, src0 + static_cast<int>(j), 64);
      if (j < d && j != i) {
        if (v < T(0.0)) sign ^= 1u;
        v = m_abs(v);
        if (!have) {
          acc = v;
          have = true;
        } else if constexpr (kMinsum) {
          acc = m_min(v, acc);
        } else {
          acc = m_max(m_min(v, acc) - m_corr(m_abs(v - acc)), T(0.0));
        }
      }
    }
    if constexpr (RULE == kRuleMinsumCorr) acc = minsum_corrected(acc, mc);
    return sign == 0 ? acc : -acc;
  } else {
    // Aminstar, arithmetic.rs:942-999: every lane of the row evaluates the row's quantities (argmin = FIRST minimum)
    uint32_t argmin = 0, sign = 0;
    T vmin = T(0.0), xmin = T(0.0);
    for (uint32_t j = 0; j < dmax; j++) {
      const T v = __shfl(x, src0 + static_cast<int>(j), 64);
      if (j < d) {
        if (v < T(0.0)) sign ^= 1u;
        const T a = m_abs(v);
        if (j == 0 || a < vmin) {
          vmin = a;
          xmin = v;
          argmin = j;
        }
      }
    }
    bool have = false;
    T delta = T(0.0);
    for (uint32_t j = 0; j < dmax; j++) {
      T v = __shfl(x, src0 + static_cast<int>(j), 64);
      if (j < d && j != argmin) {
        v = m_abs(v);
        if (!have) {
          delta = v;
          have = true;
        } else {
          delta = m_min(v, delta) - m_corr(m_abs(v - delta)) + m_corr(v + delta);
        }
      }
    }
    if (i == argmin) return ((sign != 0) != (xmin < T(0.0))) ? -delta : delta;
    delta = m_min(delta, vmin) - m_corr(m_abs(delta - vmin)) + m_corr(delta + vmin);
    return ((sign != 0) != (x < T(0.0))) ? -delta : delta;
  }
}

// The 8-bit arithmetics (Minstarapproxi8* / Aminstari8*, arithmetic.rs:603-848, 1003-1257) on this path: T = int32_t
// holds the i16 soft values and the i8 messages one per word (the values are those of the batched kernels of
// kernels_i8.hip.h: |soft| <= 127 (1 + degree), so no intermediate ever leaves 16 bits); RULE = kRuleEdgeI8 and the
// rule's options arrive at run time.
enum : int { kRuleEdgeI8 = 64 };

// the lane's output for the 8-bit rules: magnitudes fold in slot order from 255, an identity of both fold steps
// (kernels_i8.hip.h); the sign is the parity of the other inputs' signs, and a zero magnitude stays zero
__device__ __forceinline__ int rule_edge_i8(int x, uint32_t first, uint32_t i, uint32_t d, uint32_t dmax, I8Opts o) {
  const int src0 = static_cast<int>(first);
  const uint32_t neg = x < 0 ? 1u : 0u;
  const int w = (x < 0 ? -x : x) | static_cast<int>(neg << 8);  // magnitude | sign << 8: one exchange per input
  uint32_t sign = 0, mag;
  if (!o.aminstar) {
    // arithmetic.rs:722-753
    uint32_t acc = 255u;
    for (uint32_t j = 0; j < dmax; j++) {
      const uint32_t wj = static_cast<uint32_t>(__shfl(w, src0 + static_cast<int>(j), 64));
      if (j < d && j != i) {
        sign ^= wj >> 8;
        acc = i8_minstar(wj & 0xFFu, acc);
      }
    }
    mag = acc;
  } else {
    // arithmetic.rs:1134-1191: the row's first minimum is the minimum of (|x| << 16 | slot)
    uint32_t key = ~0u;
    for (uint32_t j = 0; j < dmax; j++) {
      const uint32_t wj = static_cast<uint32_t>(__shfl(w, src0 + static_cast<int>(j), 64));
      if (j < d) {
        sign ^= wj >> 8;
        key = min(key, ((wj & 0xFFu) << 16) | j);
      }
    }
    sign ^= neg;
    const uint32_t argmin = key & 0xFFFFu;
    uint32_t delta = 255u;
    for (uint32_t j = 0; j < dmax; j++) {
      const uint32_t wj = static_cast<uint32_t>(__shfl(w, src0 + static_cast<int>(j), 64));
      if (j < d && j != argmin) delta = i8_aminstar(wj & 0xFFu, delta);
    }
    mag = i == argmin ? delta : i8_aminstar(delta, key >> 16);
  }
  if (o.hardlimit) mag = mag >= 100u ? 127u : mag;
  return (sign & 1u) ? -static_cast<int>(mag) : static_cast<int>(mag);
}

// the variable node's message to a check: L - c2v (arithmetic.rs:152); 8-bit: clipped to +-127 (:648)
template <typename T>
__device__ __forceinline__ T edge_v2c(T l, T m) {
  if constexpr (std::is_integral<T>::value) return i8_clip(l - m);
  else return l - m;
}
// the caller's LLR in the decoder's arithmetic (arithmetic.rs:194-196; 8-bit: :690-699)
template <typename T, typename SrcT>
__device__ __forceinline__ T edge_quantize(SrcT raw) {
  if constexpr (std::is_integral<T>::value) return i8_quantize(static_cast<double>(raw));
  else return static_cast<T>(raw);
}

// parity of every row of the wavefront's chunk over `bit` (lane = edge): odd rows raise their first lane
__device__ __forceinline__ bool chunk_has_odd_row(bool bit, uint32_t lane, uint32_t i, uint32_t d) {
  const uint64_t b = __builtin_amdgcn_ballot_w64(bit);
  const uint64_t mask = d >= 64 ? ~0ull : ((1ull << d) - 1ull);
  return d != 0 && i == 0 && (__popcll((b >> lane) & mask) & 1u) != 0;
}

// BUNDLES: an XCD decodes up to `bundle` (<= kEdgeBundle) codewords of a call at once -- every phase walks the chunks
// of all of them, so a level's barrier is paid once per bundle, not once per codeword: 64 codewords take about the
// time of 8.  With one codeword per XCD the convergence vote rides on the barrier; with more, the wavefronts that
// saw an odd row write the vote's number into a flag per codeword (two flag sets, alternating: a set is rewritten
// only after every reader of its previous use has passed a later barrier).
enum : uint32_t { kEdgeBundle = 8 };


// The kernel (latency_edge): latency_edge.inc, once plain and once as the normalized / offset min-sum
// form (*_kernel_corr) -- see the head of that file
#define LDPC_MINSUM_CORR 0
#define LDPC_MS_KERNEL(x) x##_kernel
#define LDPC_MS_PARAM(T)
#define LDPC_MS_ARG
#define LDPC_MS_TARG
#include "latency_edge.inc"
#undef LDPC_MINSUM_CORR
#undef LDPC_MS_KERNEL
#undef LDPC_MS_PARAM
#undef LDPC_MS_ARG
#undef LDPC_MS_TARG
#define LDPC_MINSUM_CORR 1
#define LDPC_MS_KERNEL(x) x##_kernel_corr
#define LDPC_MS_PARAM(T) , MinsumCorr<T> mc = MinsumCorr<T>{}
#define LDPC_MS_ARG , mc
#define LDPC_MS_TARG , true
#include "latency_edge.inc"
#undef LDPC_MINSUM_CORR
#undef LDPC_MS_KERNEL
#undef LDPC_MS_PARAM
#undef LDPC_MS_ARG
#undef LDPC_MS_TARG

}  // namespace dev
}  // namespace ldpc
