// CPU check of the byte form of a row record's flags (csrc/graph_tables.h: record_flag_bytes; csrc/record_flags8.h: the
// encode / decode pair the kernels run), built under ASan/UBSan.
//   * record_flag_bytes: 1 where the flags are a half-word AND the flip bits and the argmin take at most 10 bits -- rows of
//     at most 7 edges --, else record_flag_bits / 8; restated here by counting.  record_flag_bits itself names the family and
//     keeps the values tests/record_flags_driver.cpp pins.
//   * encode -> decode over every (flip pattern, argmin, min1, min2): all 128 flip patterns, argmin 0..6, magnitudes from
//     {+0, smallest subnormal, 1, largest finite, +inf} in f32 and f64: flip, argmin and both magnitudes come back bit for bit,
//     the decoded magnitudes have clear sign bits, and memory holds what the format says (byte = flip | argmin bit 0 << 7,
//     argmin bits 1 and 2 in the sign bits of min1 and min2).
#include <cstdio>
#include <cstring>
#include <limits>

#include "../ldpc_toolbox_amd/csrc/graph_tables.h"

using namespace ldpc;

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) {                                                                          \
      std::fprintf(stderr, "%s:%d: %s failed (weight %u)\n", __FILE__, __LINE__, #c, w); \
      return 1;                                                                          \
    }                                                                                    \
  } while (0)

static uint32_t arg_bits_by_counting(uint32_t w) {
  uint32_t bits = 0;
  for (uint32_t reach = 1; reach < w; reach *= 2) bits++;  // smallest b with 2^b >= w
  return bits == 0 ? 1 : bits;
}
static uint32_t expected_bits(uint32_t w, bool f64) {
  const uint32_t word = f64 ? 64u : 32u;
  if (w == 0 || w > word) return 0;
  return w + arg_bits_by_counting(w) <= 16 ? 16u : word;
}
static uint32_t expected_bytes(uint32_t w, bool f64) {
  const uint32_t bits = expected_bits(w, f64);
  if (bits == 16 && w + arg_bits_by_counting(w) <= 10) return 1;
  return bits / 8;
}

template <typename F, typename W>
static int round_trips(const char *name) {
  const uint32_t w = 7;
  const F mags[5] = {F(0), std::numeric_limits<F>::denorm_min(), F(1), std::numeric_limits<F>::max(),
                     std::numeric_limits<F>::infinity()};
  constexpr int kSign = 8 * sizeof(W) - 1;
  unsigned long checked = 0;
  for (uint32_t flip = 0; flip < 128; flip++)
    for (uint32_t arg = 0; arg < 7; arg++)
      for (F f1 : mags)
        for (F f2 : mags) {
          W m1, m2;
          std::memcpy(&m1, &f1, sizeof(W));
          std::memcpy(&m2, &f2, sizeof(W));
          REQUIRE((m1 >> kSign) == 0 && (m2 >> kSign) == 0);
          const uint16_t reg = uint16_t(flip | (arg << kRecArgShift16));
          const RecFlags8Stored<W> st = record_flags8_encode<W>(m1, m2, reg);
          // what memory holds
          REQUIRE(st.byte == uint8_t(flip | ((arg & 1u) << 7)));
          REQUIRE(st.min1 == (m1 | (W((arg >> 1) & 1u) << kSign)));
          REQUIRE(st.min2 == (m2 | (W((arg >> 2) & 1u) << kSign)));
          const RecFlags8Loaded<W> ld = record_flags8_decode<W>(st.min1, st.min2, st.byte);
          REQUIRE(ld.flags == reg);
          REQUIRE((uint32_t(ld.flags) & 0xFFFu) == flip && (uint32_t(ld.flags) >> kRecArgShift16) == arg);
          REQUIRE(ld.min1 == m1 && ld.min2 == m2);
          REQUIRE((ld.min1 >> kSign) == 0 && (ld.min2 >> kSign) == 0);
          checked++;
        }
  REQUIRE(checked == 128ul * 7 * 25);
  std::printf("%s: %lu records round-trip\n", name, checked);
  return 0;
}

int main() {
  for (uint32_t w = 0; w <= 65; w++)
    for (bool f64 : {false, true}) {
      REQUIRE(record_flag_bytes(w, f64) == expected_bytes(w, f64));
      REQUIRE(record_flag_bits(w, f64) == expected_bits(w, f64));  // unchanged: it names the family
      REQUIRE((record_flag_bytes(w, f64) == 1) == (w >= 1 && w <= kRecFlags8MaxRow));
    }
  {
    const uint32_t w = 7;
    REQUIRE(record_flag_bytes(7, false) == 1 && record_flag_bytes(7, true) == 1);
    REQUIRE(record_flag_bytes(8, false) == 2 && record_flag_bytes(8, true) == 2);
    REQUIRE(record_flag_bits(7, false) == 16 && record_flag_bits(8, true) == 16);
    REQUIRE(record_flag_bytes(12, false) == 2 && record_flag_bytes(12, true) == 2);
    REQUIRE(record_flag_bytes(13, false) == 4 && record_flag_bytes(13, true) == 8);
    REQUIRE(record_flag_bytes(0, false) == 0 && record_flag_bytes(33, false) == 0 && record_flag_bytes(65, true) == 0);
  }
  std::printf("record_flag_bytes, weights 0..65: ok\n");
  if (round_trips<float, uint32_t>("f32")) return 1;
  if (round_trips<double, uint64_t>("f64")) return 1;
  std::printf("record flags8 driver: ok\n");
  return 0;
}
