// CPU check of the value a check row takes from a STORED byte-form record (csrc/record_flags8.h: record_flags8_arg and
// record_flags8_value, which cn_minsum_rec_kernel's byte form runs), built under ASan/UBSan.
// The reference is not the new code: a record is encoded, decoded by record_flags8_decode into the 16-bit form's registers,
// and the 16-bit form's `value(slot)` of those registers -- (slot == argmin ? min2 : min1) with the sign bit flip[slot],
// restated here from RowRec<T, VEC, 3, uint16_t>::value -- is what the value taken from the stored triple must equal, bit
// for bit: all 128 flip patterns x argmin 0..6 x magnitudes {+0, smallest subnormal, 1, largest finite, +inf}^2 x slot 0..6,
// in f32 and f64, through the one-call form and through the two halves the kernel calls (argmin once, value per slot).
#include <cstdio>
#include <cstring>
#include <limits>

#include "../ldpc_toolbox_amd/csrc/record_flags8.h"

using namespace ldpc;

#define REQUIRE(c)                                                                                                        \
  do {                                                                                                                    \
    if (!(c)) {                                                                                                           \
      std::fprintf(stderr, "%s:%d: %s failed (%s flip %u argmin %u slot %u)\n", __FILE__, __LINE__, #c, name, flip, arg, slot); \
      return 1;                                                                                                           \
    }                                                                                                                     \
  } while (0)

// the 16-bit form's value of a record in registers
template <typename W>
static W value16(W min1, W min2, uint16_t flags, uint32_t slot) {
  const uint32_t f = flags;
  const W mag = ((f >> kRecArgShift16) == slot) ? min2 : min1;
  const W sign = W(f >> slot) << (8 * sizeof(W) - 1);
  return mag | sign;
}

template <typename F, typename W>
static int values(const char *name) {
  const F mags[5] = {F(0), std::numeric_limits<F>::denorm_min(), F(1), std::numeric_limits<F>::max(),
                     std::numeric_limits<F>::infinity()};
  constexpr int kSign = 8 * sizeof(W) - 1;
  unsigned long checked = 0, negative = 0, second = 0;
  for (uint32_t flip = 0; flip < 128; flip++)
    for (uint32_t arg = 0; arg < 7; arg++)
      for (F f1 : mags)
        for (F f2 : mags) {
          W m1, m2;
          std::memcpy(&m1, &f1, sizeof(W));
          std::memcpy(&m2, &f2, sizeof(W));
          const RecFlags8Stored<W> st = record_flags8_encode<W>(m1, m2, uint16_t(flip | (arg << kRecArgShift16)));
          const RecFlags8Loaded<W> ld = record_flags8_decode<W>(st.min1, st.min2, st.byte);
          const uint32_t once = record_flags8_arg<W>(st.min1, st.min2, st.byte);
          for (uint32_t slot = 0; slot < 7; slot++) {
            const W want = value16<W>(ld.min1, ld.min2, ld.flags, slot);
            REQUIRE(once == arg);
            REQUIRE(record_flags8_value<W>(st.min1, st.min2, st.byte, slot) == want);
            REQUIRE(record_flags8_value<W>(st.min1, st.min2, st.byte, once, slot) == want);
            // what the value is, whatever computes it
            REQUIRE((want >> kSign) == ((flip >> slot) & 1u));
            REQUIRE(W(want << 1) == W((slot == arg ? m2 : m1) << 1));
            negative += want >> kSign;
            second += slot == arg;
            checked++;
          }
        }
  if (checked != 128ul * 7 * 25 * 7 || negative != checked / 2 || second != checked / 7) {
    std::fprintf(stderr, "%s: %lu values, %lu negative, %lu of min2\n", name, checked, negative, second);
    return 1;
  }
  std::printf("%s: %lu values equal the 16-bit form's\n", name, checked);
  return 0;
}

int main() {
  if (values<float, uint32_t>("f32")) return 1;
  if (values<double, uint64_t>("f64")) return 1;
  std::printf("record flags8 value driver: ok\n");
  return 0;
}
