// Stand-alone check of csrc/nr_link.h (built under ASan/UBSan by tests/test_nr_link_host.py): the configurations a spec
// gives and the specs it refuses, where a block begins in a transport block's row against a literal sum, the passes of the
// fused recover kernel against a literal walk over (transport block, block, column), and that kernel's arithmetic, run here
// on the host, against de-concatenation followed by rate recovery block by block.
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

static uint32_t bits_of(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return u;
}

// rate recovery of one block as nr_rm_recover_kernel<float> does it, from the block's own row of E values
static void recover_block(const nrrm::Plan &p, const float *row, float *llrs, float filler, bool combine) {
  for (uint32_t col = 0; col < p.n; col++) {
    const uint32_t r = nrrm::first_selection_of_column(p, col);
    if (r == nrrm::kFiller) {
      llrs[col] = filler;
      continue;
    }
    if (r >= p.e) {
      if (!combine) llrs[col] = 0.0f;
      continue;
    }
    float s = row[nrrm::position_of_selection(p, r)];
    for (uint32_t j = r + p.l; j < p.e; j += p.l) s = s + row[nrrm::position_of_selection(p, j)];
    llrs[col] = combine ? llrs[col] + s : s;
  }
}

// The fused kernel's body for one element, on the host: soft rows block-major over `slots`.
static void fused_element(const nrlink::Config &c, const nrlink::Geometry &k, const nrlink::Pass &pass, uint32_t i, const float *rx,
                          std::vector<float> &soft, const std::vector<uint8_t> &done, uint32_t slots, uint32_t first_slot,
                          const nrrm::Plan &p_lo, const nrrm::Plan &p_hi, float filler, bool combine) {
  const nrlink::Element el = nrlink::element_of(k, pass.within + i);
  const uint64_t b = pass.tb0 + el.tb, slot = first_slot + b;
  if (combine && done[slot * k.c + el.r]) return;
  nrrm::Plan p = p_lo;
  if (el.r >= k.c_lo) {
    p.e = p_hi.e;
    p.cols = p_hi.cols;
    p.div_cols = p_hi.div_cols;
  }
  float *out = &soft.at((uint64_t(el.r) * slots + slot) * k.n + el.column);
  const uint32_t r = nrrm::first_selection_of_column(p, el.column);
  if (r == nrrm::kFiller) {
    *out = filler;
    return;
  }
  if (r >= p.e) {
    if (!combine) *out = 0.0f;
    return;
  }
  const float *row = rx + b * k.g + nrlink::start_of_block(k, el.r);
  CHECK(nrlink::start_of_block(k, el.r) + p.e <= k.g, "block %u ends behind G", el.r);
  float s = row[nrrm::position_of_selection(p, r)];
  for (uint32_t j = r + p.l; j < p.e; j += p.l) s = s + row[nrrm::position_of_selection(p, j)];
  *out = combine ? *out + s : s;
}

static long check_fused(const char *spec, uint32_t batch, uint32_t slots, uint32_t first_slot, uint64_t pass_elements) {
  const nrlink::Config c = config(spec);
  const nrlink::Geometry k = nrlink::make_geometry(c);
  const uint32_t cc = c.tb.c, n = c.tb.n, g = c.len.g;
  std::vector<float> rx(size_t(batch) * g);
  uint32_t state = 12345u + batch;
  for (float &v : rx) {
    state = state * 1664525u + 1013904223u;
    v = (int32_t(state >> 8) % 2001 - 1000) / 37.0f;
  }
  rx[3] = -0.0f;
  rx[g - 1] = std::numeric_limits<float>::quiet_NaN();
  std::vector<float> soft(size_t(cc) * slots * n, -99.0f), want(soft);
  std::vector<uint8_t> done(size_t(slots) * cc, 0);
  long compared = 0;
  for (int pass_no = 0; pass_no < 2; pass_no++) {  // a first transmission at rv 0, then a combining one at rv 2 with some blocks done
    const bool combine = pass_no == 1;
    const uint32_t rv = combine ? 2 : 0;
    const float filler = 20.0f;
    if (combine)
      for (uint32_t b = 0; b < batch; b++) done[size_t(first_slot + b) * cc + (b % cc)] = 1;
    const nrrm::Plan p_lo = nrrm::make_plan(c.rm, c.len.e_lo, rv, c.qm), p_hi = nrrm::make_plan(c.rm, c.len.e_hi, rv, c.qm);
    // the composition: block r of transport block b is E_r values from block_start on, recovered alone
    for (uint32_t b = 0; b < batch; b++)
      for (uint32_t r = 0; r < cc; r++) {
        if (combine && done[size_t(first_slot + b) * cc + r]) continue;
        uint32_t start = 0;
        for (uint32_t t = 0; t < r; t++) start += nrlink::block_length(c, t);
        CHECK(start == nrlink::block_start(c, r) && start == nrlink::start_of_block(k, r), "start of block %u", r);
        recover_block(r < c.len.c_lo ? p_lo : p_hi, &rx[size_t(b) * g + start], &want[(size_t(r) * slots + first_slot + b) * n], filler, combine);
      }
    // the fused kernel in passes, each element once
    const uint64_t elements = uint64_t(batch) * k.per_tb;
    uint64_t seen = 0;
    int passes = 0;
    for (uint64_t first = 0; first < elements; first += pass_elements, passes++) {
      const nrlink::Pass pass = nrlink::make_pass(c, first, std::min<uint64_t>(pass_elements, elements - first));
      for (uint32_t i = 0; i < pass.total; i++, seen++) {
        const nrlink::Element el = nrlink::element_of(k, pass.within + i);
        const uint64_t at = ((pass.tb0 + el.tb) * cc + el.r) * n + el.column;
        CHECK(at == seen, "pass %d element %u is element %llu of the call, not %llu", passes, i, (unsigned long long)at, (unsigned long long)seen);
        fused_element(c, k, pass, i, rx.data(), soft, done, slots, first_slot, p_lo, p_hi, filler, combine);
      }
    }
    CHECK(seen == elements && passes == int((elements + pass_elements - 1) / pass_elements), "%llu elements in %d passes",
          (unsigned long long)seen, passes);
    for (size_t i = 0; i < soft.size(); i++, compared++)
      CHECK(bits_of(soft[i]) == bits_of(want[i]), "%s soft[%zu] = %g, want %g (combine %d)", spec, i, soft[i], want[i], int(combine));
  }
  return compared;
}

int main() {
  // the configurations of the issue's table
  {
    const nrlink::Config c = config("nr5g-link:2:8016:18004:4");
    CHECK(c.tb.c == 3 && c.tb.zc == 288 && c.tb.k == 2880 && c.tb.fillers == 176 && c.tb.n == 14976, "2:8016: C %u Zc %u K %u F %u n %u", c.tb.c,
          c.tb.zc, c.tb.k, c.tb.fillers, c.tb.n);
    CHECK(c.len.e_lo == 6000 && c.len.e_hi == 6004 && c.len.c_lo == 2 && c.symbols == 4501 && c.q == 4 && c.layers == 1, "2:8016 lengths");
    CHECK(nrlink::block_start(c, 0) == 0 && nrlink::block_start(c, 1) == 6000 && nrlink::block_start(c, 2) == 12000, "2:8016 starts");
    const nrlink::Config d = config("nr5g-link:2:4000:6004:2");
    CHECK(d.tb.c == 2 && d.tb.zc == 208 && d.tb.k == 2080 && d.tb.fillers == 44 && d.tb.n == 10816, "2:4000");
    CHECK(d.len.e_lo == 3002 && d.len.e_hi == 3002 && d.len.c_lo == 2, "2:4000 lengths");
    const nrlink::Config e = config("nr5g-link:2:176:600:2");
    CHECK(e.tb.c == 1 && e.tb.n == 1664 && e.len.e_lo == 600 && e.len.c_lo == 1, "2:176");
    const nrlink::Config f = config("nr5g-link:2:8016:18024:4:2");  // two layers: q = 8, 2253 groups of 8 bits over three blocks
    CHECK(f.q == 8 && f.layers == 2 && f.len.e_lo == 6008 && f.len.e_hi == 6008 && f.len.c_lo == 3 && f.symbols == 4506, "layers");
    const nrlink::Config h = config("nr5g-link:2:8016:18032:4:2");  // 2254 groups: blocks of 751, 751 and 752 groups
    CHECK(h.len.e_lo == 6008 && h.len.e_hi == 6016 && h.len.c_lo == 2 && nrlink::block_start(h, 2) == 12016, "layers, two lengths");
    std::printf("configurations ok\n");
  }
  // starts against the literal sum, over many (A, G)
  {
    long cases = 0;
    for (int64_t a : {176, 4000, 8016, 30000, 100000})
      for (int64_t qm : {2, 4, 6, 8})
        for (int64_t nl : {1, 3})
          for (int64_t extra = 0; extra < 12; extra++) {
            nrlink::Config c;
            const int64_t g = qm * nl * (3 * ((a + qm * nl - 1) / (qm * nl)) + extra);
            if (nrlink::make_config(2, a, g, qm, nl, &c) != nullptr) continue;
            const nrlink::Geometry k = nrlink::make_geometry(c);
            uint32_t sum = 0;
            for (uint32_t r = 0; r < c.tb.c; r++) {
              CHECK(nrlink::block_start(c, r) == sum && nrlink::start_of_block(k, r) == sum, "A %lld G %lld block %u", (long long)a, (long long)g, r);
              sum += nrlink::block_length(c, r);
              CHECK(nrlink::block_length(c, r) % c.qm == 0, "E_r is a multiple of QM");
            }
            CHECK(sum == c.len.g, "the lengths sum to G");
            cases++;
          }
    CHECK(cases > 300, "%ld cases", cases);
    std::printf("starts: %ld configurations agree with the literal sum\n", cases);
  }
  // the fused kernel's arithmetic against the composition, in one pass and in passes that end inside a transport block
  {
    long compared = 0;
    compared += check_fused("nr5g-link:2:8016:18004:4", 2, 5, 1, nrlink::kPassElements);
    compared += check_fused("nr5g-link:2:8016:18004:4", 3, 4, 1, 40000);  // 14976 * 3 = 44928 per transport block: 4 passes
    compared += check_fused("nr5g-link:2:176:600:2", 5, 5, 0, 1000);
    compared += check_fused("nr5g-link:2:4000:6004:2", 2, 3, 1, 21632 + 7);
    compared += check_fused("nr5g-link:1:9000:30006:6", 2, 2, 0, 100001);  // base graph 1, 64QAM: blocks of 15000 and 15006
    compared += check_fused("nr5g-link:2:176:4000:2", 2, 3, 1, 1 << 20);   // E = 4000 over n = 1664: every column repeats
    std::printf("fused recover: %ld soft values agree with split and recover, bit for bit\n", compared);
  }
  // refusals
  {
    nrlink::Config c;
    for (const char *spec : {"nr5g-link:2:8016:18004", "nr5g-link:2:8016:18004:4:1:1", "nr5g-link:2:8016:18004:4:", "nr5g-link:2:8016::4",
                             "nr5g-link:2:8016:18004:+4", "nr5g-link:2:8016:18004: 4", "nr5g-tb:2:8016", "NR5G-LINK:2:8016:18004:4", "", "nr5g-link",
                             "nr5g-link:", "nr5g-link:2:8016:18004:0x4", "nr5g-link:2:8016:99999999999:4"})
      CHECK(nrlink::parse_spec(spec, &c) != nullptr, "%s accepted", spec);
    for (const char *spec : {"nr5g-link:3:8016:18004:4", "nr5g-link:2:0:18004:4", "nr5g-link:2:1277993:18004:4", "nr5g-link:2:8016:18004:3",
                             "nr5g-link:2:8016:18004:10", "nr5g-link:2:8016:18004:4:0", "nr5g-link:2:8016:18004:4:5", "nr5g-link:2:8016:18006:4",
                             "nr5g-link:2:8016:0:4", "nr5g-link:2:8016:8:4", "nr5g-link:2:8016:4294967296:4", "nr5g-link:2:8016:18004:4:2"})
      CHECK(nrlink::parse_spec(spec, &c) != nullptr, "%s accepted", spec);
    const nrlink::Config ok = config("nr5g-link:2:8016:18004:4");
    CHECK(nrlink::transmit_argument_error(ok, 4501, 8016, 3, -1) == nullptr && nrlink::transmit_argument_error(ok, 4501, 8016, 0, 0x7fffffff) == nullptr,
          "a good call");
    CHECK(nrlink::transmit_argument_error(ok, 4500, 8016, 0, -1) && nrlink::transmit_argument_error(ok, 4501, 8015, 0, -1) &&
              nrlink::transmit_argument_error(ok, 4501, 8016, 4, -1) && nrlink::transmit_argument_error(ok, 4501, 8016, 0, -2) &&
              nrlink::transmit_argument_error(ok, 4501, 8016, 0, int64_t(1) << 31),
          "transmit refusals");
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    CHECK(nrlink::receive_argument_error(ok, 4501, 8016, 0, -1, false, 0.5, 2, 5, 8) == nullptr, "a good receive");
    CHECK(nrlink::receive_argument_error(ok, 4501, 8016, 0, -1, false, 0.5, 3, 5, 8) == nullptr &&
              nrlink::receive_argument_error(ok, 4501, 8016, 0, -1, false, 0.5, 4, 5, 8) != nullptr,
          "first_slot + batch against slots");
    CHECK(nrlink::slots_error(0xffffffffu, 2, 0xffffffffu) != nullptr && nrlink::slots_error(9, 0, 8) != nullptr && nrlink::slots_error(8, 0, 8) == nullptr &&
              nrlink::slots_error(0, uint64_t(1) << 40, 8) != nullptr,
          "slot ranges at the ends");
    for (double sigma : {0.0, -1.0, nan, inf}) {
      CHECK(nrlink::receive_argument_error(ok, 4501, 8016, 0, -1, false, sigma, 0, 1, 8) != nullptr, "sigma %g accepted", sigma);
      CHECK(nrlink::receive_argument_error(ok, 4501, 8016, 0, -1, true, sigma, 0, 1, 8) == nullptr, "sigma %g read with a scale", sigma);
    }
    CHECK(nrlink::filler_llr_error(20.0) == nullptr && nrlink::filler_llr_error(inf) == nullptr && nrlink::filler_llr_error(0.0) &&
              nrlink::filler_llr_error(-1.0) && nrlink::filler_llr_error(nan) && nrlink::filler_llr_error(-inf),
          "filler LLR");
    CHECK(nrlink::pass_elements_error(1) == nullptr && nrlink::pass_elements_error(int64_t(1) << 30) == nullptr && nrlink::pass_elements_error(0) &&
              nrlink::pass_elements_error(-5) && nrlink::pass_elements_error((int64_t(1) << 30) + 1),
          "pass_elements");
    // the largest transport block: the kernel's index stays below 2^31 with the largest pass
    nrlink::Config big;
    CHECK(nrlink::make_config(1, 1277992, 2000000, 2, 1, &big) == nullptr, "the largest A");
    const nrlink::Geometry k = nrlink::make_geometry(big);
    CHECK(uint64_t(k.per_tb) + nrlink::kPassElements < (uint64_t(1) << 31), "C n = %u", k.per_tb);
    const nrlink::Pass last = nrlink::make_pass(big, uint64_t(7) * k.per_tb + k.per_tb - 1, nrlink::kPassElements);
    const nrlink::Element el = nrlink::element_of(k, last.within + last.total - 1);
    const uint64_t at = uint64_t(7) * k.per_tb + k.per_tb - 1 + nrlink::kPassElements - 1;
    CHECK(last.tb0 == 7 && ((last.tb0 + el.tb) * big.tb.c + el.r) * uint64_t(big.tb.n) + el.column == at, "the last element of the largest pass");
    std::printf("refusals ok\n");
  }
  if (failures) {
    std::printf("nr link driver: %d failures\n", failures);
    return 1;
  }
  std::printf("nr link driver: ok\n");
  return 0;
}
