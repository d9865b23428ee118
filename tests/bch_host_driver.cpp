// CPU driver of csrc/bch.h, built under ASan/UBSan by tests/test_bch_host.py: spec parsing and every refusal, the
// generator anchors, bch_argument_error, and a host loop over the kernels' own functions (the remainder register and the
// table that combines the lanes' runs, the syndromes of a remainder, the locator, the root count) arranged as the
// kernels arrange them -- against a syndrome-table decoder built here, exhaustively on the small codes.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../ldpc_toolbox_amd/csrc/bch.h"

using namespace ldpc::bch;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (failures++ < 20) {                              \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__);  \
        std::printf(__VA_ARGS__);                         \
        std::printf("\n");                                \
      }                                                   \
    }                                                     \
  } while (0)

static std::string hex_of(const std::vector<uint8_t> &g) {
  std::string s;
  for (size_t i = (g.size() + 3) / 4; i-- > 0;) {
    unsigned v = 0;
    for (size_t b = 0; b < 4; b++)
      if (4 * i + b < g.size() && g[4 * i + b]) v |= 1u << b;
    s += "0123456789abcdef"[v];
  }
  const size_t nz = s.find_first_not_of('0');
  return "0x" + s.substr(nz == std::string::npos ? s.size() - 1 : nz);
}

// what remainder_kernel leaves in `total`: (row(x) * x^parity) mod g, the row's `bits` bytes spread over the lanes of geo
template <int NW>
static void remainder_total(const Code &c, const Geometry &geo, const std::vector<uint32_t> &table, const uint8_t *row,
                            uint32_t *total) {
  std::vector<uint32_t> staged(geo.staged_words, 0);
  for (uint32_t q = 0; q < geo.staged_words * 32; q++)
    if (q >= geo.pad && q - geo.pad < geo.bits && row[q - geo.pad] == 1) staged[q >> 5] |= 1u << (q & 31);
  uint32_t g_all[kMaxParityWords], g_top[NW];
  generator_top(c, g_all);
  for (int w = 0; w < NW; w++) g_top[w] = g_all[w];
  for (uint32_t w = 0; w < kMaxParityWords; w++) total[w] = 0;
  const uint32_t shift = 32 * NW - c.parity;
  for (uint32_t lane = 0; lane < geo.lanes; lane++) {
    uint32_t s[NW] = {};
    for (uint32_t w = 0; w < geo.run_words; w++) {
      const uint32_t x = staged[lane * geo.run_words + w];
      for (uint32_t b = 0; b < 32; b++) rem_step<NW>(s, g_top, (x >> b) & 1u);
    }
    for (uint32_t j = shift; j < 32u * NW; j++)
      if ((s[j >> 5] >> (j & 31)) & 1u)
        for (int ww = 0; ww < NW; ww++) total[ww] ^= table.at((size_t(j - shift) * NW + ww) * geo.lanes + lane);
  }
}

static void remainder_any(const Code &c, const Geometry &geo, const std::vector<uint32_t> &table, const uint8_t *row, uint32_t *total) {
  switch (c.parity_words()) {
    case 1: return remainder_total<1>(c, geo, table, row, total);
    case 2: return remainder_total<2>(c, geo, table, row, total);
    case 3: return remainder_total<3>(c, geo, table, row, total);
    case 4: return remainder_total<4>(c, geo, table, row, total);
    case 5: return remainder_total<5>(c, geo, table, row, total);
    default: return remainder_total<6>(c, geo, table, row, total);
  }
}

struct HostCodec {
  Code c;
  Geometry enc_geo, dec_geo;
  std::vector<uint32_t> enc_table, dec_table;
  explicit HostCodec(const std::string &spec) {
    std::string err;
    if (!parse_spec(spec, &c, &err)) {
      std::printf("FAIL cannot parse %s: %s\n", spec.c_str(), err.c_str());
      std::exit(1);
    }
    enc_geo = geometry(c.k);
    dec_geo = geometry(c.n);
    enc_table = remainder_table(c, enc_geo);
    dec_table = remainder_table(c, dec_geo);
    if (dec_geo.staged_words > kMaxStagedWords || dec_geo.lanes > kThreads) {
      std::printf("FAIL geometry of %s does not fit the kernels\n", spec.c_str());
      std::exit(1);
    }
  }
  std::vector<uint8_t> encode(const std::vector<uint8_t> &msg) const {
    std::vector<uint8_t> cw(c.n, 0);
    for (uint32_t i = 0; i < c.k; i++) cw[i] = msg[i] == 1;
    uint32_t total[kMaxParityWords];
    remainder_any(c, enc_geo, enc_table, msg.data(), total);
    for (uint32_t q = 0; q < c.parity; q++) {
      const uint32_t i = c.parity - 1 - q;
      cw[c.k + q] = (total[i >> 5] >> (i & 31)) & 1u;
    }
    return cw;
  }
  // the three decoder kernels in a row
  int decode(const std::vector<uint8_t> &in, std::vector<uint8_t> *out) const {
    out->assign(c.n, 0);
    for (uint32_t i = 0; i < c.n; i++) (*out)[i] = in[i] == 1;
    uint32_t total[kMaxParityWords];
    remainder_any(c, dec_geo, dec_table, in.data(), total);
    uint32_t any = 0;
    for (uint32_t w = 0; w < kMaxParityWords; w++) any |= total[w];
    if (!any) return 0;
    uint32_t odd[kMaxT] = {}, lambda[kMaxT + 1];
    for (uint32_t j = 0; j < c.t; j++) odd[j] = syndrome_of_remainder(total, c.parity, 2 * j + 1, c.m, c.antilog.data());
    const uint32_t L = locator(odd, c.t, c.poly, c.m, lambda);
    if (L > c.t) return -1;
    uint16_t loglambda[kMaxT + 1];
    for (uint32_t i = 0; i <= kMaxT; i++) loglambda[i] = c.log[lambda[i]];
    uint32_t found = 0, position[kMaxT];
    for (uint32_t p = 0; p < c.n; p++) {
      if (!is_root(loglambda, p, c.m, c.antilog.data())) continue;
      if (found < kMaxT) position[found] = p;
      found++;
    }
    if (found != L) return -1;
    for (uint32_t i = 0; i < L; i++) (*out)[c.n - 1 - position[i]] ^= 1;
    return static_cast<int>(L);
  }
  // r(x) mod g as a bit string key, by plain division (independent of the functions under test)
  std::string plain_remainder(const std::vector<uint8_t> &row) const {
    std::vector<uint8_t> r(row.size());
    for (size_t i = 0; i < row.size(); i++) r[i] = row[i] == 1;
    for (size_t i = 0; i + c.parity < r.size(); i++)
      if (r[i])
        for (uint32_t q = 0; q <= c.parity; q++) r[i + q] ^= c.g[c.parity - q];
    return std::string(r.end() - c.parity, r.end());
  }
};

static void check_mod_order() {
  const uint32_t samples[] = {0u, 1u, 14u, 15u, 16u, 225u, 0xFFFFu, 0x10000u, 23u * 65534u, 0x7FFFFFFFu, 0xFFFFFFF0u, 0xFFFFFFFFu};
  for (uint32_t m = 4; m <= 16; m++)
    for (uint32_t x : samples) CHECK(mod_order(x, m) == x % ((1u << m) - 1u), "mod_order(%u, %u) = %u", x, m, mod_order(x, m));
}

static void check_refusals() {
  Code c;
  std::string err;
  const char *refused[] = {"",          "bch",           "bch:5:25:3",      "bch:5:25:3:31:1", "bch:3:b:1:7",   "bch:17:2002d:1:100",
                           "bch:5:45:3:31",  // degree 6, not 5
                           "bch:5:3f:3:31",  // x^5+x^4+x^3+x^2+x+1: not primitive
                           "bch:5:21:3:31",  // x^5+1: not primitive
                           "bch:4:13:8:15",  // 2T >= 2^M - 1
                           "bch:5:25:0:31",  // T < 1
                           "bch:5:25:3:32",  // N > 2^M - 1
                           "bch:5:25:3:15",  // N - deg g < 1
                           "bch:16:1002D:13:65535",  // T > 12
                           "bch:5:2g:3:31", "bch:x:25:3:31", "bch:5:25:3:-1", "dvbs2:R7_8", "dvbs2:", "nr5g:1:384"};
  for (const char *s : refused) {
    err.clear();
    CHECK(!parse_spec(s, &c, &err) && !err.empty(), "spec '%s' was not refused", s);
  }
  CHECK(parse_spec("bch:5:25:3:16", &c, &err) && c.k == 1, "N = parity + 1 must be accepted");
  CHECK(parse_spec("bch:4:13:7:15", &c, &err), "2T = 14 < 15 must be accepted: %s", err.c_str());
}

static void check_anchors() {
  struct A {
    const char *spec, *g;
    uint32_t k;
  } anchors[] = {{"bch:5:25:3:31", "0x8faf", 16},
                 {"bch:6:43:3:63", "0x782cf", 45},
                 {"bch:6:43:2:40", "0x1539", 28},
                 {"bch:16:1002D:8:65535", "0x11c07255f712797bd19fc6d7504f9662b", 65535 - 128},
                 {"bch:16:1002D:10:65535", "0x160150cedfc2a331f6a785703efd12301b8bb6591", 65535 - 160},
                 {"bch:16:1002D:12:65535", "0x14e260e83845c511c50cf2cd8dc350889034785f7660255e7", 65535 - 192},
                 {"bch:14:402B:8:16383", "0x192d612e23675eda463552df84609", 16383 - 112},
                 {"bch:14:402B:10:16383", "0x1dbfd25eb862e4274cbbd64bda7f7b65cc0f", 16383 - 140},
                 {"bch:14:402B:12:16383", "0x14062dbea9869b262cd23a39069528fe7d7d11905a5", 16383 - 168}};
  for (const A &a : anchors) {
    Code c;
    std::string err;
    CHECK(parse_spec(a.spec, &c, &err), "%s refused: %s", a.spec, err.c_str());
    CHECK(hex_of(c.g) == a.g && c.k == a.k, "%s: g = %s, k = %u", a.spec, hex_of(c.g).c_str(), c.k);
  }
  size_t count = 0;
  const Dvbs2Entry *e = dvbs2_entries(&count);
  CHECK(count == 21, "21 DVB-S2 names");
  for (size_t i = 0; i < count; i++) {
    Code c;
    std::string err;
    CHECK(parse_spec(std::string("dvbs2:") + e[i].name, &c, &err), "dvbs2:%s refused", e[i].name);
    CHECK(c.n == e[i].n && c.t == e[i].t && c.parity == c.m * c.t && c.k == c.n - c.parity, "dvbs2:%s parameters", e[i].name);
  }
  Code c;
  std::string err;
  parse_spec("dvbs2:R1_2short", &c, &err);
  CHECK(c.n == 7200 && c.k == 7032 && c.m == 14, "R1_2short");
  CHECK(bch_argument_error(c, false, 7200, 7032) == nullptr && bch_argument_error(c, false, 7200, 7200) != nullptr &&
            bch_argument_error(c, false, 7032, 7032) != nullptr,
        "encoder lengths");
  CHECK(bch_argument_error(c, true, 7032, 7200) == nullptr && bch_argument_error(c, true, 7200, 7200) == nullptr &&
            bch_argument_error(c, true, 7031, 7200) != nullptr && bch_argument_error(c, true, 7032, 7032) != nullptr &&
            bch_argument_error(c, true, 0, 7200) != nullptr,
        "decoder lengths");
}

// every pattern of weight <= max_weight (at most `sample` of each weight, evenly thinned) on a codeword, against the table
static void check_small(const std::string &spec, uint32_t max_weight, size_t sample) {
  HostCodec h(spec);
  const Code &c = h.c;
  std::mt19937 rng(7);
  std::vector<uint8_t> msg(c.k);
  for (auto &b : msg) b = rng() & 1;
  const std::vector<uint8_t> cw = h.encode(msg);
  CHECK(h.plain_remainder(cw) == std::string(c.parity, '\0'), "%s: the encoder's word is not a codeword", spec.c_str());
  // the definition: remainder of every pattern of weight <= t -> the pattern
  std::map<std::string, std::vector<uint32_t>> table;
  std::vector<uint32_t> pos;
  auto each_pattern = [&](uint32_t weight, auto &&fn) {
    pos.assign(weight, 0);
    for (uint32_t i = 0; i < weight; i++) pos[i] = i;
    while (true) {
      fn();
      int i = static_cast<int>(weight) - 1;
      while (i >= 0 && pos[i] == c.n - weight + i) i--;
      if (i < 0) break;
      pos[i]++;
      for (uint32_t q = i + 1; q < weight; q++) pos[q] = pos[q - 1] + 1;
    }
  };
  for (uint32_t w = 0; w <= c.t; w++)
    each_pattern(w, [&] {
      std::vector<uint8_t> e(c.n, 0);
      for (uint32_t p : pos) e[p] = 1;
      const bool fresh = table.emplace(h.plain_remainder(e), pos).second;
      CHECK(fresh, "%s: two patterns of weight <= t share a remainder", spec.c_str());
    });
  size_t corrected = 0, detected = 0, miscorrected = 0, total = 0;
  for (uint32_t w = 0; w <= max_weight; w++) {
    size_t all = 1;
    for (uint32_t i = 0; i < w; i++) all = all * (c.n - i) / (i + 1);
    const size_t stride = all > sample ? all / sample : 1;
    size_t index = 0;
    each_pattern(w, [&] {
      if (index++ % stride) return;
      std::vector<uint8_t> r = cw, out;
      for (uint32_t p : pos) r[p] ^= 1;
      r[0] = r[0] ? 1 : (index % 3 == 0 ? 255 : 0);  // (a zero may be any byte but 1)
      const int got = h.decode(r, &out);
      std::vector<uint8_t> e(c.n, 0);
      for (uint32_t p : pos) e[p] = 1;
      const auto it = table.find(h.plain_remainder(e));
      std::vector<uint8_t> want(c.n);
      for (uint32_t i = 0; i < c.n; i++) want[i] = r[i] == 1;
      int want_errors = -1;
      if (it != table.end()) {
        want_errors = static_cast<int>(it->second.size());
        for (uint32_t p : it->second) want[p] ^= 1;
      }
      CHECK(got == want_errors && out == want, "%s: weight %u pattern %zu: errors %d, expected %d", spec.c_str(), w, index - 1, got,
            want_errors);
      total++;
      if (want_errors < 0)
        detected++;
      else if (w <= c.t)
        corrected++;
      else
        miscorrected++;
    });
  }
  std::printf("%s: %zu patterns up to weight %u: %zu corrected, %zu detected, %zu miscorrected\n", spec.c_str(), total, max_weight,
              corrected, detected, miscorrected);
}

static void check_planted(const std::string &spec) {
  HostCodec h(spec);
  const Code &c = h.c;
  std::mt19937 rng(11);
  std::vector<uint8_t> msg(c.k);
  for (auto &b : msg) b = rng() & 1;
  const std::vector<uint8_t> cw = h.encode(msg);
  CHECK(h.plain_remainder(cw) == std::string(c.parity, '\0'), "%s: the encoder's word is not a codeword", spec.c_str());
  for (uint32_t i = 0; i < c.k; i++) CHECK(cw[i] == msg[i], "%s: not systematic", spec.c_str());
  const uint32_t weights[] = {0, 1, c.t, c.t + 1};
  for (uint32_t w : weights) {
    for (int trial = 0; trial < 3; trial++) {
      std::vector<uint8_t> r = cw, out;
      std::vector<uint32_t> where;
      while (where.size() < w) {
        const uint32_t p = trial == 0 ? static_cast<uint32_t>(where.size()) * (c.n - 1) / (w > 1 ? w - 1 : 1) : rng() % c.n;
        bool dup = false;
        for (uint32_t q : where) dup |= q == p;
        if (!dup) where.push_back(p);
      }
      for (uint32_t p : where) r[p] ^= 1;
      const int got = h.decode(r, &out);
      if (w <= c.t) {
        CHECK(got == static_cast<int>(w) && out == cw, "%s: %u planted errors: errors %d", spec.c_str(), w, got);
      } else if (got < 0) {
        CHECK(out == r, "%s: a failed word came back changed", spec.c_str());
      } else {  // a miscorrection: another codeword within t
        uint32_t dist = 0;
        for (uint32_t i = 0; i < c.n; i++) dist += out[i] != r[i];
        CHECK(h.plain_remainder(out) == std::string(c.parity, '\0') && dist == static_cast<uint32_t>(got) && dist <= c.t,
              "%s: errors %d but the output is no codeword at that distance", spec.c_str(), got);
      }
    }
  }
  std::printf("%s: planted errors ok\n", spec.c_str());
}

int main() {
  check_mod_order();
  check_refusals();
  check_anchors();
  check_small("bch:5:25:3:31", 5, 20000);
  check_small("bch:5:25:3:25", 5, 20000);
  check_small("bch:6:43:3:63", 5, 20000);
  check_small("bch:6:43:2:40", 4, 20000);
  check_planted("bch:14:402B:12:300");
  check_planted("bch:16:1002D:12:65535");
  check_planted("dvbs2:R9_10");
  if (failures) {
    std::printf("bch host driver: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("bch host driver: ok\n");
  return 0;
}
