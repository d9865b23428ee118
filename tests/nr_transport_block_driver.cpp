// Stand-alone check of csrc/nr_transport_block.h (built under ASan/UBSan by tests/test_nr_transport_block_host.py): the
// segmentation plan against a literal loop over TS 38.212 5.2.2, the tables of x^j mod g and the rule that combines runs
// against bit-serial division, the packed index of concatenation, and the E_r of 5.4.2.1.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../ldpc_toolbox_amd/csrc/nr_transport_block.h"

using namespace ldpc::nrtb;

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

// Table 5.3.2-1, written out
static const int kSizes[51] = {2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12,  13,  14,  15,  16,  18,  20,  22,  24,  26,  28,  30,  32,  36,  40, 44,
                               48, 52, 56, 60, 64, 72, 80, 88, 96, 104, 112, 120, 128, 144, 160, 176, 192, 208, 224, 240, 256, 288, 320, 352, 384};

static void check_plans() {
  long accepted = 0, refused = 0;
  for (int bg = 1; bg <= 2; bg++)
    for (int a = 1; a <= 20000; a++) {
      // 5.1 and 5.2.2, literally
      const int l_tb = a > 3824 ? 24 : 16, b = a + l_tb, kcb = bg == 1 ? 8448 : 3840;
      int l_cb = 0, c = 1, b_prime = b;
      if (b > kcb) {
        l_cb = 24;
        c = 0;
        while (c * (kcb - l_cb) < b) c++;  // ceil(B / (Kcb - L))
        b_prime = b + c * l_cb;
      }
      Config got;
      const char *why = make_config(bg, a, &got);
      if (b_prime % c != 0) {
        refused++;
        CHECK(why != nullptr, "bg %d a %d should be refused", bg, a);
        continue;
      }
      accepted++;
      CHECK(why == nullptr, "bg %d a %d: %s", bg, a, why ? why : "");
      if (why) continue;
      const int k_prime = b_prime / c;
      const int kb = bg == 1 ? 22 : b > 640 ? 10 : b > 560 ? 9 : b > 192 ? 8 : 6;
      int zc = 0;
      for (int i = 0; i < 51 && !zc; i++)
        if (kb * kSizes[i] >= k_prime) zc = kSizes[i];
      const int k = (bg == 1 ? 22 : 10) * zc;
      CHECK(int(got.l_tb) == l_tb && int(got.b) == b && int(got.c) == c && int(got.l_cb) == l_cb, "bg %d a %d: crc / blocks", bg, a);
      CHECK(int(got.k_prime) == k_prime && int(got.kb) == kb && int(got.zc) == zc && int(got.k) == k, "bg %d a %d: K' %u Kb %u Zc %u", bg, a,
            got.k_prime, got.kb, got.zc);
      CHECK(got.kb * got.zc >= got.k_prime, "bg %d a %d: Kb Zc < K'", bg, a);
      for (int i = 0; i < 51; i++) CHECK(kSizes[i] >= zc || kb * kSizes[i] < k_prime, "bg %d a %d: Zc %d not minimal", bg, a, zc);
      CHECK(int(got.fillers) == k - k_prime && got.k_prime <= got.k && int(got.n) == (bg == 1 ? 68 : 52) * zc, "bg %d a %d: F, n", bg, a);
      CHECK(got.s == got.k_prime - got.l_cb && uint64_t(got.s) * got.c == got.b, "bg %d a %d: S", bg, a);
      uint32_t sum = 0;
      for (uint32_t r = 0; r < got.c; r++) sum += payload_bits_of_block(got.a, got.s, r);
      CHECK(sum == got.a, "bg %d a %d: payload bits of the blocks", bg, a);
    }
  Config big;
  CHECK(make_config(1, 1277992, &big) == nullptr && big.c == 152 && big.k_prime == 8432 && big.zc == 384 && big.fillers == 16, "largest A");
  Config none;
  CHECK(make_config(0, 100, &none) && make_config(3, 100, &none) && make_config(1, 0, &none) && make_config(1, 1277993, &none) &&
            make_config(2, -5, &none),
        "refusals");
  std::printf("plans: %ld accepted and %ld refused agree with the literal loop\n", accepted, refused);
}

// bit-serial long division of bits[0] x^(len-1) + ... by g
static uint32_t literal_remainder(const std::vector<uint8_t> &bits, size_t from, size_t to, Poly g) {
  const uint64_t full = (uint64_t(1) << g.len) | g.low;
  uint64_t s = 0;
  for (size_t i = from; i < to; i++) {
    s = (s << 1) | bits[i];
    if (s >> g.len) s ^= full;
  }
  return static_cast<uint32_t>(s);
}

// the kernels' path: words with the first bit on top, the runs counted from the end, one table entry per run
static uint32_t run_remainder(const std::vector<uint8_t> &bits, size_t from, size_t to, const uint32_t *table, Poly g) {
  const uint32_t cover = static_cast<uint32_t>(to - from);
  std::vector<uint32_t> words(cover / 32 + 1, 0);  // exactly what run_from_end may read: ASan sees one word more
  for (uint32_t i = 0; i < cover; i++) words[i / 32] |= uint32_t(bits[from + i]) << (31 - i % 32);
  uint32_t acc = 0;
  for (uint32_t w = 0; 32 * w < cover; w++) acc ^= mul_mod_word(run_from_end(words.data(), cover, w), table[w], g);
  return acc;
}

static void check_crc_arithmetic() {
  std::mt19937_64 rng(38212);
  const Poly polys[3] = {kCrc24A, kCrc24B, kCrc16};
  // the catalogue's check values: the CRC of "123456789"
  const uint32_t check[3] = {0xCDE703, 0x23EF52, 0x31C3};
  std::vector<uint8_t> msg;
  for (const char *p = "123456789"; *p; p++)
    for (int i = 7; i >= 0; i--) msg.push_back((*p >> i) & 1);
  long splits = 0;
  for (int pi = 0; pi < 3; pi++) {
    const Poly g = polys[pi];
    const size_t max_len = 20000;
    const std::vector<uint32_t> table = power_table(g, max_len / 32 + 2);
    CHECK(rem_shift(literal_remainder(msg, 0, msg.size(), g), g.len, g) == check[pi], "check value of polynomial %d", pi);
    // the table against repeated single steps
    uint32_t s = 1;
    for (size_t j = 0; j < 32 * 40; j++) {
      if (j % 32 == 0) CHECK(table[j / 32] == s, "x^%zu mod g%d", j, pi);
      CHECK(shift_by_table(1, j, table.data(), g) == s, "shift_by_table %zu g%d", j, pi);
      s = rem_step(s, 0, g);
    }
    const size_t lengths[] = {0, 1, 2, 23, 24, 25, 31, 32, 33, 63, 64, 65, 100, 577, 1949, 4249, 8432, 8448, 19999};
    for (size_t len : lengths) {
      std::vector<uint8_t> bits(len);
      for (auto &x : bits) x = rng() & 1;
      const uint32_t want = literal_remainder(bits, 0, len, g);
      CHECK(run_remainder(bits, 0, len, table.data(), g) == want, "g%d len %zu: word runs", pi, len);
      // two and three runs cut at random points, at the ends (runs of length 0) and next to them (runs of length 1)
      std::vector<size_t> cuts = {0, len, len ? size_t(1) : 0, len ? len - 1 : 0};
      for (int i = 0; i < 12; i++) cuts.push_back(len ? rng() % (len + 1) : 0);
      for (size_t c1 : cuts)
        for (size_t c2 : cuts) {
          if (c2 < c1) continue;
          const uint32_t r0 = run_remainder(bits, 0, c1, table.data(), g), r1 = run_remainder(bits, c1, c2, table.data(), g),
                         r2 = run_remainder(bits, c2, len, table.data(), g);
          const uint32_t got = shift_by_table(r0, len - c1, table.data(), g) ^ shift_by_table(r1, len - c2, table.data(), g) ^ r2;
          CHECK(got == want, "g%d len %zu cut at %zu, %zu", pi, len, c1, c2);
          CHECK(mul_mod(r0, shift_by_table(1, len - c1, table.data(), g), g) == shift_by_table(r0, len - c1, table.data(), g), "mul_mod");
          splits++;
        }
    }
  }
  // the device tables of a configuration: the bits of B behind block r, and the identity the last block's CRC24B rests on
  Config c;
  CHECK(make_config(2, 7641, &c) == nullptr, "config");
  const std::vector<uint32_t> t = device_tables(c);
  const uint32_t entries = power_entries(c);
  CHECK(t.size() == 2 * entries + c.c, "device_tables size");
  const Poly gt = tb_poly(c);
  for (uint32_t r = 0; r < c.c; r++) {
    uint32_t s = 1;
    for (uint64_t j = 0; j < uint64_t(c.c - 1 - r) * c.s; j++) s = rem_step(s, 0, gt);
    CHECK(t[2 * entries + r] == s, "behind[%u]", r);
  }
  std::vector<uint8_t> payload(1000), p(24);
  for (auto &x : payload) x = rng() & 1;
  for (auto &x : p) x = rng() & 1;
  std::vector<uint8_t> both = payload;
  both.insert(both.end(), p.begin(), p.end());
  const uint32_t whole = rem_shift(literal_remainder(both, 0, both.size(), kCrc24B), 24, kCrc24B);
  const uint32_t parts = rem_shift(literal_remainder(payload, 0, payload.size(), kCrc24B), 48, kCrc24B) ^
                         rem_shift(literal_remainder(p, 0, 24, kCrc24B), 24, kCrc24B);
  CHECK(whole == parts, "CRC24B over (payload, p) by linearity");
  std::printf("crc: %ld split runs agree with bit-serial division\n", splits);
}

static void check_block_lengths() {
  long cases = 0;
  const int as[] = {100, 3826, 7641, 8426, 100020, 1277992};
  for (int a : as) {
    Config c;
    const int bg = a == 100 || a == 3826 || a == 7641 ? 2 : 1;
    CHECK(make_config(bg, a, &c) == nullptr, "config %d", a);
    if (c.c == 0) continue;
    const uint64_t qs[] = {1, 2, 4, 6, 8, 16, 32};
    for (uint64_t q : qs)
      for (uint64_t symbols = c.c; symbols < c.c + 400; symbols += (symbols < c.c + 2 * uint64_t(c.c) + 3 ? 1 : 37)) {
        const uint64_t g = symbols * q;
        uint64_t e_lo, e_hi, c_lo;
        const char *why = block_lengths(c, g, q, &e_lo, &e_hi, &c_lo);
        CHECK(why == nullptr, "a %d g %llu q %llu: %s", a, (unsigned long long)g, (unsigned long long)q, why ? why : "");
        if (why) continue;
        uint64_t sum = 0;
        for (uint32_t r = 0; r < c.c; r++) {
          // 5.4.2.1
          const uint64_t e = r <= c.c - symbols % c.c - 1 ? q * (g / (q * c.c)) : q * ((g + q * c.c - 1) / (q * c.c));
          CHECK(e == (r < c_lo ? e_lo : e_hi), "a %d g %llu q %llu: E_%u", a, (unsigned long long)g, (unsigned long long)q, r);
          sum += e;
        }
        CHECK(sum == g, "a %d g %llu q %llu: the E_r sum to %llu", a, (unsigned long long)g, (unsigned long long)q, (unsigned long long)sum);
        // the packed index: a bijection that puts block r of transport block b at row r * batch + b
        if (g <= 3000) {
          Lengths l;
          CHECK(make_lengths(c, g, q, &l) == nullptr, "make_lengths");
          const uint64_t batch = 5, b0 = 2, frames = 3;
          const Packing p = make_packing(l, batch, b0);
          for (uint32_t idx = 0; idx < frames * g; idx += 7) {
            const uint64_t b = b0 + idx / g;
            uint64_t pos = idx % g, at = 0, r = 0;
            while (pos >= (r < c_lo ? e_lo : e_hi)) {
              pos -= r < c_lo ? e_lo : e_hi;
              at += batch * (r < c_lo ? e_lo : e_hi);
              r++;
            }
            CHECK(packed_index(p, idx) == at + b * (r < c_lo ? e_lo : e_hi) + pos, "packed index g %llu idx %u", (unsigned long long)g, idx);
          }
        }
        cases++;
      }
    uint64_t e_lo, e_hi, c_lo;
    CHECK(block_lengths(c, 0, 1, &e_lo, &e_hi, &c_lo) && block_lengths(c, 100 * uint64_t(c.c), 0, &e_lo, &e_hi, &c_lo) &&
              block_lengths(c, 2 * uint64_t(c.c) + 1, 2, &e_lo, &e_hi, &c_lo) && block_lengths(c, uint64_t(1) << 31, 1, &e_lo, &e_hi, &c_lo),
          "a %d: refusals", a);
    if (c.c > 1) CHECK(block_lengths(c, 2 * uint64_t(c.c) - 2, 2, &e_lo, &e_hi, &c_lo) != nullptr, "a %d: G / q below C", a);
  }
  std::printf("block lengths: %ld cases agree with the formula and sum to G\n", cases);
}

static void check_base_graph() {
  CHECK(base_graph(292, 0.9) == 2 && base_graph(293, 0.9) == 1 && base_graph(3824, 0.67) == 2 && base_graph(3824, 0.68) == 1 &&
            base_graph(3825, 0.67) == 1 && base_graph(3825, 0.25) == 2 && base_graph(3825, 0.26) == 1,
        "7.2.2");
}

int main() {
  check_plans();
  check_crc_arithmetic();
  check_block_lengths();
  check_base_graph();
  if (failures) {
    std::printf("nr transport block driver: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("nr transport block driver: ok\n");
  return 0;
}
