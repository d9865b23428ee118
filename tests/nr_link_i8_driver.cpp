// Stand-alone check of what csrc/nr_link.h adds for the 8-bit mode of the link handle (include/ldpc_toolbox.h, PART 12), built
// under ASan/UBSan by tests/test_nr_link_i8_host.py: the setter's refusals, the filler soft bit, the bytes of the slots, the
// dword passes of the 8-bit fused recover kernel against a literal walk, and that kernel's arithmetic -- four columns and one
// dword per thread, run here on the host -- against a split of the bytes followed by rate recovery block by block.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../ldpc_toolbox_amd/csrc/nr_link.h"

using namespace ldpc;

static int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      if (failures++ < 20) {                   \
        std::printf("FAIL %s: ", #cond);       \
        std::printf(__VA_ARGS__);              \
        std::printf("\n");                     \
      }                                        \
    }                                          \
  } while (0)

static nrlink::Config config(const char *spec) {
  nrlink::Config c;
  const char *why = nrlink::parse_spec(spec, &c);
  CHECK(why == nullptr, "%s: %s", spec, why ? why : "");
  return c;
}

static int clip(int v) { return v > 127 ? 127 : (v < -127 ? -127 : v); }

// one column of a soft row from the block's own E bytes, as PART 9 defines it: literal, no helper of soft_i8.h
static int column_value(const nrrm::Plan &p, const int8_t *row, uint32_t col, int filler, bool combine, int old) {
  const uint32_t r = nrrm::first_selection_of_column(p, col);
  if (r == nrrm::kFiller) return filler;
  const int kept = combine ? clip(old) : 0;
  if (r >= p.e) return kept;
  int s = clip(row[nrrm::position_of_selection(p, r)]);
  for (uint32_t j = r + p.l; j < p.e; j += p.l) s = clip(s + clip(row[nrrm::position_of_selection(p, j)]));
  return combine ? clip(kept + s) : s;
}

// The 8-bit fused kernel's body for thread i of a pass, on the host: soft rows block-major over `slots`, one dword.
static void fused_dword(const nrlink::Geometry &k, const nrlink::Pass &pass, uint32_t i, const int8_t *rx, std::vector<int8_t> &soft,
                        const std::vector<uint8_t> &done, uint32_t slots, uint32_t first_slot, const nrrm::Plan &p_lo, const nrrm::Plan &p_hi,
                        int filler, bool combine) {
  const nrlink::Element el = nrlink::element_of(k, pass.within + 4 * i);
  const uint64_t b = pass.tb0 + el.tb, slot = first_slot + b;
  if (combine && done[slot * k.c + el.r]) return;
  nrrm::Plan p = p_lo;
  if (el.r >= k.c_lo) {
    p.e = p_hi.e;
    p.cols = p_hi.cols;
    p.div_cols = p_hi.div_cols;
  }
  const uint64_t at = (uint64_t(el.r) * slots + slot) * k.n + el.column;
  CHECK(at % 4 == 0 && el.column + 3 < k.n, "a thread's dword: soft byte %llu, column %u of %u", (unsigned long long)at, el.column, k.n);
  CHECK(nrlink::start_of_block(k, el.r) + p.e <= k.g, "block %u ends behind G", el.r);
  const int8_t *row = rx + b * k.g + nrlink::start_of_block(k, el.r);
  for (uint32_t j = 0; j < 4; j++) {
    int8_t &out = soft.at(at + j);
    out = static_cast<int8_t>(column_value(p, row, el.column + j, filler, combine, out));
  }
}

static long check_fused(const char *spec, uint32_t batch, uint32_t slots, uint32_t first_slot, uint64_t pass_elements) {
  const nrlink::Config c = config(spec);
  const nrlink::Geometry k = nrlink::make_geometry(c);
  const uint32_t cc = c.tb.c, n = c.tb.n, g = c.len.g;
  CHECK(n % 4 == 0 && k.per_tb % 4 == 0, "n = %u", n);
  std::vector<int8_t> rx(size_t(batch) * g);
  uint32_t state = 777u + batch;
  for (int8_t &v : rx) {
    state = state * 1664525u + 1013904223u;
    v = static_cast<int8_t>(state >> 13);  // all 256 bytes, -128 among them
  }
  rx[5] = -128;
  std::vector<int8_t> soft(size_t(cc) * slots * n, -99), want(soft);
  std::vector<uint8_t> done(size_t(slots) * cc, 0);
  const uint64_t per_pass = nrlink::dword_pass_elements(pass_elements);
  long compared = 0;
  for (int call = 0; call < 3; call++) {  // a first transmission at rv 0, then two combining ones with some blocks done
    const bool combine = call > 0;
    const uint32_t rv = call == 0 ? 0 : (call == 1 ? 2 : 3);
    const int filler = 127;
    if (call == 1) {
      for (uint32_t b = 0; b < batch; b += 2) done[size_t(first_slot + b) * cc + (b % cc)] = 1;
      // a byte of -128 in a row that is combined into (transport block 1 has no done block): clip(old)
      soft[size_t(first_slot + 1) * n + 1] = want[size_t(first_slot + 1) * n + 1] = -128;
    }
    const nrrm::Plan p_lo = nrrm::make_plan(c.rm, c.len.e_lo, rv, c.qm), p_hi = nrrm::make_plan(c.rm, c.len.e_hi, rv, c.qm);
    // the composition: block r of transport block b is E_r bytes from the literal sum of the lengths on, recovered alone
    for (uint32_t b = 0; b < batch; b++)
      for (uint32_t r = 0; r < cc; r++) {
        if (combine && done[size_t(first_slot + b) * cc + r]) continue;
        uint32_t start = 0;
        for (uint32_t t = 0; t < r; t++) start += nrlink::block_length(c, t);
        const nrrm::Plan &p = r < c.len.c_lo ? p_lo : p_hi;
        int8_t *row = &want[(size_t(r) * slots + first_slot + b) * n];
        for (uint32_t col = 0; col < n; col++)
          row[col] = static_cast<int8_t>(column_value(p, &rx[size_t(b) * g + start], col, filler, combine, row[col]));
      }
    // the fused kernel in dword passes: every dword of the call once, in order
    const uint64_t elements = uint64_t(batch) * k.per_tb;
    uint64_t seen = 0;
    int passes = 0;
    for (uint64_t first = 0; first < elements; first += per_pass, passes++) {
      const nrlink::Pass pass = nrlink::make_pass(c, first, std::min<uint64_t>(per_pass, elements - first));
      CHECK(pass.within % 4 == 0 && pass.total % 4 == 0 && pass.total > 0, "pass %d: within %u, total %u", passes, pass.within, pass.total);
      for (uint32_t i = 0; i < pass.total / 4; i++, seen += 4) {
        const nrlink::Element el = nrlink::element_of(k, pass.within + 4 * i);
        const uint64_t at = ((pass.tb0 + el.tb) * cc + el.r) * n + el.column;
        CHECK(at == seen, "pass %d thread %u is element %llu of the call, not %llu", passes, i, (unsigned long long)at, (unsigned long long)seen);
        fused_dword(k, pass, i, rx.data(), soft, done, slots, first_slot, p_lo, p_hi, filler, combine);
      }
    }
    CHECK(seen == elements && passes == int((elements + per_pass - 1) / per_pass), "%llu elements in %d passes", (unsigned long long)seen, passes);
    for (size_t i = 0; i < soft.size(); i++, compared++)
      CHECK(soft[i] == want[i], "%s soft[%zu] = %d, want %d (call %d)", spec, i, soft[i], want[i], call);
  }
  CHECK(soft[size_t(first_slot + 1) * n + 1] >= -127, "-128 does not survive a combine");
  return compared;
}

int main() {
  // the dword passes against a literal search
  {
    long checked = 0;
    for (uint64_t v : {uint64_t(1), uint64_t(2), uint64_t(3), uint64_t(4), uint64_t(5), uint64_t(7), uint64_t(8), uint64_t(70001), (uint64_t(1) << 30) - 1,
                       uint64_t(1) << 30})
      for (uint64_t d = 0; d < 9 && d < v; d++, checked++) {
        const uint64_t x = v - d;
        uint64_t want = x;
        while (want % 4 != 0) want--;  // the largest multiple of 4 not above x
        if (want == 0) want = 4;
        CHECK(nrlink::dword_pass_elements(x) == want, "pass_elements %llu -> %llu, want %llu", (unsigned long long)x,
              (unsigned long long)nrlink::dword_pass_elements(x), (unsigned long long)want);
      }
    for (uint64_t x = 1; x < 5000; x++, checked++) {
      const uint64_t got = nrlink::dword_pass_elements(x);
      CHECK(got % 4 == 0 && got >= 4 && (x < 4 ? got == 4 : (got <= x && x - got < 4)), "pass_elements %llu -> %llu", (unsigned long long)x,
            (unsigned long long)got);
    }
    // every n is a multiple of 4: 52 Zc or 68 Zc
    for (uint32_t zc : {2u, 3u, 5u, 7u, 9u, 11u, 13u, 15u, 384u}) CHECK((52 * zc) % 4 == 0 && (68 * zc) % 4 == 0, "Zc %u", zc);
    std::printf("dword passes: %ld values agree with the literal search\n", checked);
  }
  // the mode
  {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    CHECK(nrlink::filler_soft_bit(inf) == 127 && nrlink::filler_soft_bit(20.0) == 127 && nrlink::filler_soft_bit(15.8125) == 127 &&
              nrlink::filler_soft_bit(15.8) == 126 && nrlink::filler_soft_bit(1.0) == 8 && nrlink::filler_soft_bit(0.0625) == 1 &&
              nrlink::filler_soft_bit(0.05) == 0 && nrlink::filler_soft_bit(nan) == 0,
          "Q(filler LLR)");
    CHECK(nrlink::filler_soft_bit_error(20.0) == nullptr && nrlink::filler_soft_bit_error(inf) == nullptr && nrlink::filler_soft_bit_error(0.0625) == nullptr &&
              nrlink::filler_soft_bit_error(0.05) != nullptr && nrlink::filler_soft_bit_error(0.06) != nullptr,
          "the filler soft bit of an 8-bit handle");
    // (value, current, 8-bit implementation, filler LLR, device state)
    CHECK(nrlink::soft_bits_error(8, 32, true, inf, false) == nullptr && nrlink::soft_bits_error(32, 8, true, inf, false) == nullptr &&
              nrlink::soft_bits_error(32, 8, false, 0.05, false) == nullptr,
          "a change before the device state");
    CHECK(nrlink::soft_bits_error(32, 32, false, 0.05, true) == nullptr && nrlink::soft_bits_error(8, 8, true, 20.0, true) == nullptr,
          "the current value, always");
    for (int64_t v : {int64_t(0), int64_t(1), int64_t(7), int64_t(16), int64_t(31), int64_t(33), int64_t(64), int64_t(-8), int64_t(1) << 40})
      CHECK(nrlink::soft_bits_error(v, 32, true, inf, false) != nullptr && nrlink::soft_bits_error(v, 8, true, inf, false) != nullptr, "soft_bits %lld accepted",
            (long long)v);
    CHECK(nrlink::soft_bits_error(8, 32, false, inf, false) != nullptr, "8 on a float implementation");
    CHECK(nrlink::soft_bits_error(8, 32, true, 0.05, false) != nullptr, "8 with a filler that quantises to 0");
    CHECK(nrlink::soft_bits_error(8, 32, true, inf, true) != nullptr && nrlink::soft_bits_error(32, 8, true, inf, true) != nullptr,
          "a change once the slots exist");
    const nrlink::Config c = config("nr5g-link:2:8016:18010:2");
    uint64_t bytes = 0;
    for (uint32_t slot = 0; slot < 8; slot++)
      for (uint32_t r = 0; r < c.tb.c; r++) bytes += c.tb.n;
    CHECK(bytes == uint64_t(3) * 8 * 14976 && nrlink::soft_bytes(c, 8, 8) == bytes && nrlink::soft_bytes(c, 8, 32) == 4 * bytes, "soft_bytes");
    CHECK(c.len.e_lo == 6002 && c.len.e_hi == 6004 && c.len.c_lo == 1 && nrlink::block_start(c, 1) == 6002 && nrlink::block_start(c, 2) == 12006,
          "2:8016:18010:2: blocks at 0 and 2 mod 4");
    std::printf("mode ok\n");
  }
  // the 8-bit fused kernel's arithmetic against the composition
  {
    long compared = 0;
    compared += check_fused("nr5g-link:2:8016:18010:2", 2, 5, 1, nrlink::kPassElements);
    compared += check_fused("nr5g-link:2:8016:18010:2", 3, 3, 0, 40001);  // passes of 40000 that end inside transport blocks
    compared += check_fused("nr5g-link:2:8016:18004:4", 2, 2, 0, 5);      // one dword per pass
    compared += check_fused("nr5g-link:2:12:122:2", 3, 5, 1, 3);          // n = 260; rows of G = 122 begin at 2 mod 4
    compared += check_fused("nr5g-link:2:176:4000:2", 4, 4, 0, 1001);     // E = 4000 over n = 1664: every sent column repeats
    compared += check_fused("nr5g-link:1:9000:30006:6", 2, 2, 0, 100001);
    std::printf("fused recover i8: %ld soft bits agree with split and recover, byte for byte\n", compared);
  }
  if (failures) {
    std::printf("nr link i8 driver: %d failures\n", failures);
    return 1;
  }
  std::printf("nr link i8 driver: ok\n");
  return 0;
}
