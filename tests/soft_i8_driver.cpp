// Stand-alone check of csrc/soft_i8.h (built under ASan/UBSan by tests/test_soft_i8_host.py; this header only): clip on all
// 256 bytes, the packed clip on words built from all 256 bytes, the saturating accumulate on all 256 x 256 pairs against the
// literal definition, and Q against the literal rule -- clamp(round-half-away(8 x)) to +-127, NaN -> 0, with libm's round,
// which the header does without -- on every float within a few ulps of each half-step k / 16, k = -2040 .. 2040, and on
// +-inf, NaN, +-0 and subnormals.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <limits>

#include "../ldpc_toolbox_amd/csrc/soft_i8.h"

using namespace ldpc::soft;

static int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (failures++ < 20) {             \
        std::printf("FAIL %s: ", #cond); \
        std::printf(__VA_ARGS__);        \
        std::printf("\n");               \
      }                                  \
    }                                    \
  } while (0)

static int literal_clip(int v) { return v < -127 ? -127 : (v > 127 ? 127 : v); }

static int literal_q(double x) {
  const double y = 8.0 * x;
  if (std::isnan(y)) return 0;
  const double r = std::round(y);  // half away from zero
  if (r >= 127.0) return 127;
  if (r <= -127.0) return -127;
  return static_cast<int>(r);
}

int main() {
  for (int b = 0; b < 256; b++) {
    const int v = static_cast<int8_t>(b);
    CHECK(soft_clip(v) == literal_clip(v), "clip(%d) = %d", v, soft_clip(v));
    CHECK(soft_clip(v) == (v == -128 ? -127 : v), "only -128 changes: %d", v);
    // the packed form: the byte at each of the four positions, the other three cycling through all values too
    for (int k = 0; k < 4; k++) {
      const uint32_t others[3] = {uint32_t(b * 7 + 1) & 0xFFu, uint32_t(255 - b), 0x80u};
      uint32_t w = 0, want = 0;
      for (int j = 0, o = 0; j < 4; j++) {
        const uint32_t byte = j == k ? uint32_t(b) : others[o++];
        w |= byte << (8 * j);
        want |= uint32_t(static_cast<uint8_t>(literal_clip(static_cast<int8_t>(byte)))) << (8 * j);
      }
      CHECK(soft_clip4(w) == want, "clip4(%08x) = %08x, want %08x", w, soft_clip4(w), want);
    }
  }
  std::printf("clip: 256 bytes, packed at 4 positions\n");

  long pairs = 0, saturated = 0;
  for (int a = 0; a < 256; a++)
    for (int b = 0; b < 256; b++) {
      const int s = literal_clip(static_cast<int8_t>(a)), t = literal_clip(static_cast<int8_t>(b));
      const int want = literal_clip(s + t);
      CHECK(soft_accumulate(soft_clip(static_cast<int8_t>(a)), soft_clip(static_cast<int8_t>(b))) == want, "acc(%d, %d)", s, t);
      CHECK(want >= -127 && want <= 127, "range");
      pairs++;
      saturated += (s + t != want);
    }
  // not associative: the order is part of the definition
  CHECK(soft_accumulate(soft_accumulate(100, 100), -100) == 27 && soft_accumulate(100, soft_accumulate(100, -100)) == 100, "order");
  std::printf("accumulate: %ld pairs, %ld saturate\n", pairs, saturated);

  long values = 0;
  auto check_q = [&](double x) {
    CHECK(soft_quantize(x) == literal_q(x), "Q(%a) = %d, want %d", x, soft_quantize(x), literal_q(x));
    values++;
  };
  for (int k = -2040; k <= 2040; k++) {
    // floats: the half-step itself (exact in float) and the 4 floats on either side
    float f = static_cast<float>(k) / 16.0f, up = f, down = f;
    check_q(f);
    for (int u = 0; u < 4; u++) {
      up = std::nextafterf(up, std::numeric_limits<float>::infinity());
      down = std::nextafterf(down, -std::numeric_limits<float>::infinity());
      check_q(up);
      check_q(down);
    }
    // and the doubles around it
    double d = static_cast<double>(k) / 16.0, dup = d, ddown = d;
    for (int u = 0; u < 4; u++) {
      dup = std::nextafter(dup, std::numeric_limits<double>::infinity());
      ddown = std::nextafter(ddown, -std::numeric_limits<double>::infinity());
      check_q(dup);
      check_q(ddown);
    }
  }
  const double inf = std::numeric_limits<double>::infinity();
  CHECK(soft_quantize(inf) == 127 && soft_quantize(-inf) == -127, "infinities");
  CHECK(soft_quantize(std::numeric_limits<double>::quiet_NaN()) == 0 && soft_quantize(-std::numeric_limits<double>::quiet_NaN()) == 0, "NaN");
  CHECK(soft_quantize(0.0) == 0 && soft_quantize(-0.0) == 0, "zeros");
  for (double x : {inf, -inf, 0.0, -0.0, 1e300, -1e300, 15.875, -15.875, 15.8125, -15.8125, 15.9, 16.0, 1e-300, -1e-300,
                   static_cast<double>(std::numeric_limits<float>::denorm_min()), -static_cast<double>(std::numeric_limits<float>::denorm_min()),
                   std::numeric_limits<double>::denorm_min(), -std::numeric_limits<double>::denorm_min(),
                   static_cast<double>(std::numeric_limits<float>::min()), static_cast<double>(std::numeric_limits<float>::max()),
                   -static_cast<double>(std::numeric_limits<float>::max()), 0.0625, -0.0625, 0.062499999999999993, 0.06250000000000001})
    check_q(x);
  // Q of clip(v) / 8 as a float is clip(v): what the 8-bit decode entry's definition rests on
  for (int b = 0; b < 256; b++) {
    const int c = literal_clip(static_cast<int8_t>(b));
    CHECK(soft_quantize(static_cast<double>(static_cast<float>(c) / 8.0f)) == c, "Q(clip / 8) of %d", c);
  }
  std::printf("quantise: %ld values agree with the literal rule\n", values);
  if (failures) {
    std::printf("soft i8 driver: %d FAILURES\n", failures);
    return 1;
  }
  std::printf("soft i8 driver: ok\n");
  return 0;
}
