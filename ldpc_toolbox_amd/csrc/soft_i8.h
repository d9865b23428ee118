// The 8-bit soft bit of the receive path (include/ldpc_toolbox.h, PART 9): one step is 1/8 of an LLR unit, a soft bit an
// int8_t in -127..127, positive = bit 0.  Host and device, no HIP types: tests/soft_i8_driver.cpp compiles this header
// alone under ASan/UBSan and checks every function below against the literal definition.
//
//   soft_clip(v)         min(max(v, -127), 127): symmetric, so a byte of -128 reads as -127 everywhere.  Not the decoder's
//                        i8_sat_add (kernels_i8.hip.h), which saturates to -128..127 inside the decoder.
//   soft_accumulate(s,t) clip(s + t) of two clipped values: the saturating sum of rate recovery and HARQ combining.  Not
//                        associative -- the order of a column's repeats is part of the definition.
//   soft_quantize(x)     Q(x) = clamp(round-half-away(8 x)) to +-127, NaN -> 0: the quantiser of the 8-bit decoders
//                        (kernels_i8.hip.h, i8_quantize; the reference's arithmetic.rs:690-699), here without libm.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDPC_SOFT_FN __host__ __device__ inline
#else
#define LDPC_SOFT_FN inline
#endif

namespace ldpc {
namespace soft {

constexpr int kSoftMax = 127;     // the largest soft bit; the smallest is -kSoftMax
constexpr int kStepsPerUnit = 8;  // steps per LLR unit

LDPC_SOFT_FN int soft_clip(int v) { return v > kSoftMax ? kSoftMax : (v < -kSoftMax ? -kSoftMax : v); }

// s, t: already clipped
LDPC_SOFT_FN int soft_accumulate(int s, int t) { return soft_clip(s + t); }

// the four bytes of a word clipped, byte k at bits 8 k: only 0x80 changes, to 0x81
LDPC_SOFT_FN uint32_t soft_clip4(uint32_t w) {
  const uint32_t low7_zero = ~((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) & 0x80808080u;  // bit 7 of a byte whose low seven bits are 0
  return w | ((low7_zero & w) >> 7);                                            // ... and whose bit 7 is set: 0x80
}

// round-half-away of |y| < 127 as an integer: the truncation, plus one where the fraction reaches one half.  8 x is exact
// in double for every float and double x, and y - trunc(y) is exact below 2^52, so this is Rust's f64::round.
LDPC_SOFT_FN int soft_quantize(double x) {
  const double y = 8.0 * x;
  if (y >= 127.0) return kSoftMax;
  if (y <= -127.0) return -kSoftMax;
  if (y != y) return 0;
  const double a = y < 0.0 ? -y : y;
  const int t = static_cast<int>(a);
  const int r = t + ((a - static_cast<double>(t)) >= 0.5 ? 1 : 0);
  return y < 0.0 ? -r : r;
}

}  // namespace soft
}  // namespace ldpc
