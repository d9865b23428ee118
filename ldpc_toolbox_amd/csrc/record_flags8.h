// The byte form of a flooding row record's flags (rows of at most 7 edges: graph_tables.h, record_flag_bytes), as the pair
// of functions that turns the record's registers into what memory holds and back, and the value a reader takes from the
// stored words directly (record_flags8_value, at the end).  Host and device compile the same code: the kernels' RowRec<T,
// VEC, 3, uint8_t> and RowRec8Once (kernels_flooding.hip.h), tests/record_flags8_driver.cpp and
// tests/record_flags8_value_driver.cpp on the CPU.
//
// In registers a record is the 16-bit form's: two magnitudes with clear sign bits and a half-word, flip bits 0..11 and the
// argmin in bits 12..15.  With at most 7 edges that is 7 flip bits and 3 argmin bits, and the stored magnitudes never use
// their sign bits (they are minima of absolute values, corrected ones clamped at 0, never NaN: RowRec::value relies on it),
// so memory holds
//   the byte      flip bits 0..6 | argmin bit 0 in bit 7
//   min1's word   the magnitude  | argmin bit 1 in the sign bit
//   min2's word   the magnitude  | argmin bit 2 in the sign bit
// W: the magnitude's bit pattern, uint32_t for f32 and uint64_t for f64.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define REC8_FN __host__ __device__ __forceinline__
#else
#define REC8_FN inline
#endif

namespace ldpc {

constexpr int kRecArgShift16 = 12;  // the half-word of the register form: flip bits at 0..11, argmin at 12..15
constexpr uint32_t kRecFlags8MaxRow = 7;  // the longest row whose flags fit: 7 flip bits + 3 argmin bits

template <typename W>
struct RecFlags8Stored {
  W min1, min2;
  uint8_t byte;
};
template <typename W>
struct RecFlags8Loaded {
  W min1, min2;
  uint16_t flags;
};

template <typename W>
REC8_FN RecFlags8Stored<W> record_flags8_encode(W min1, W min2, uint16_t flags) {
  constexpr int kSign = 8 * sizeof(W) - 1;
  const uint32_t f = flags, arg = f >> kRecArgShift16;
  return RecFlags8Stored<W>{W(min1 | (W((arg >> 1) & 1u) << kSign)), W(min2 | (W((arg >> 2) & 1u) << kSign)),
                            uint8_t((f & 0x7Fu) | ((arg & 1u) << 7))};
}
template <typename W>
REC8_FN RecFlags8Loaded<W> record_flags8_decode(W min1, W min2, uint8_t byte) {
  constexpr int kSign = 8 * sizeof(W) - 1;
  const W mag = ~(W(1) << kSign);
  const uint32_t b = byte;
  const uint32_t arg = (b >> 7) | (uint32_t(min1 >> kSign) << 1) | (uint32_t(min2 >> kSign) << 2);
  return RecFlags8Loaded<W>{W(min1 & mag), W(min2 & mag), uint16_t((b & 0x7Fu) | (arg << kRecArgShift16))};
}

// The message a stored record sends on `slot`, taken from the stored words themselves -- what the 16-bit form's `value`
// returns for record_flags8_decode's output, without building that output: the argmin once per record and codeword
// (record_flags8_arg), then per slot one select between the stored words, whose sign bits the flip bit replaces.
// (x with its sign bit replaced by s's.  Spelt as the floating-point copysign, a pure bit operation on every target: the
// GPU then has one bit-field insert, and knows that only s's top bit is read -- the flip bit need only be SHIFTED there)
REC8_FN uint32_t record_flags8_with_sign_of(uint32_t x, uint32_t s) {
  return __builtin_bit_cast(uint32_t, __builtin_copysignf(__builtin_bit_cast(float, x), __builtin_bit_cast(float, s)));
}
REC8_FN uint64_t record_flags8_with_sign_of(uint64_t x, uint64_t s) {
  return __builtin_bit_cast(uint64_t, __builtin_copysign(__builtin_bit_cast(double, x), __builtin_bit_cast(double, s)));
}
template <typename W>
REC8_FN uint32_t record_flags8_arg(W min1, W min2, uint8_t byte) {
  constexpr int kSign = 8 * sizeof(W) - 1;
  return (uint32_t(byte) >> 7) | (uint32_t(min1 >> kSign) << 1) | (uint32_t(min2 >> kSign) << 2);
}
template <typename W>
REC8_FN W record_flags8_value(W min1, W min2, uint8_t byte, uint32_t arg, uint32_t slot) {
  constexpr int kSign = 8 * sizeof(W) - 1;
  const W sel = (arg == slot) ? min2 : min1;
  return record_flags8_with_sign_of(sel, W(W(uint32_t(byte) >> slot) << kSign));
}
template <typename W>
REC8_FN W record_flags8_value(W min1, W min2, uint8_t byte, uint32_t slot) {
  return record_flags8_value<W>(min1, min2, byte, record_flags8_arg<W>(min1, min2, byte), slot);
}

}  // namespace ldpc
