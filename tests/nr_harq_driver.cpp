// Stand-alone check of csrc/nr_harq.h (built under ASan/UBSan by tests/test_nr_harq_host.py): the validation of a HARQ
// sequence, its offsets, pairs and per-transmission plans against a literal loop over the concatenated transmitted row.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ldpc_toolbox_amd/csrc/nr_harq.h"

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

// the concatenated row written out: for every position g its transmission, its position there and its codeword column
struct Where {
  int t, j, column;
};

static std::vector<Where> literal_row(const nrrm::Config &c, const std::vector<uint64_t> &e, const std::vector<uint32_t> &rv, uint32_t qm) {
  std::vector<Where> row;
  for (size_t t = 0; t < e.size(); t++) {
    const nrrm::Plan p = nrrm::make_plan(c, static_cast<uint32_t>(e[t]), rv[t], qm);
    for (uint64_t j = 0; j < e[t]; j++) row.push_back({int(t), int(j), int(nrrm::column_of_position(p, uint32_t(j)))});
  }
  return row;
}

static long check_sequence(const nrrm::Config &c, const std::vector<uint64_t> &e, const std::vector<uint32_t> &rv, uint32_t qm, uint32_t m) {
  const uint32_t T = static_cast<uint32_t>(e.size());
  const char *why = nrharq::sequence_error(e.data(), rv.data(), T, qm, m);
  CHECK(why == nullptr, "T %u qm %u m %u: %s", T, qm, m, why ? why : "");
  if (why) return 0;
  const nrharq::Sequence s = nrharq::make_sequence(e.data(), rv.data(), T, qm);
  const std::vector<Where> row = literal_row(c, e, rv, qm);
  CHECK(s.t == T && s.qm == qm && s.offset[T] == row.size(), "T %u: length %u, %zu", T, s.offset[T], row.size());
  long checked = 0;
  std::vector<int> used(2 * ((row.size() + 1) / 2), 0);  // how often each normal of each pair is used over the sequence
  for (uint32_t t = 0; t < T; t++) {
    CHECK(s.e[t] == e[t] && s.rv[t] == rv[t], "t %u", t);
    CHECK(row[s.offset[t]].t == int(t) && row[s.offset[t]].j == 0 && row[s.offset[t + 1] - 1].t == int(t), "t %u: offsets", t);
    const nrrm::Plan p = nrharq::plan_of(c, s, t);
    // BPSK, as the generator's threads walk it: pair q of the transmission, the positions it carries there
    const uint32_t first = nrharq::first_pair(s, t), pairs = nrharq::pairs(s, t);
    uint32_t covered = 0;
    for (uint32_t q = 0; q < pairs; q++) {
      const uint32_t g = 2 * (first + q);
      for (uint32_t h = 0; h < 2; h++) {
        if (g + h < s.offset[t] || g + h - s.offset[t] >= s.e[t]) continue;
        const uint32_t j = g + h - s.offset[t];
        CHECK(row[g + h].t == int(t) && row[g + h].j == int(j), "t %u pair %u half %u", t, first + q, h);
        CHECK(int(nrrm::column_of_position(p, j)) == row[g + h].column, "t %u position %u: column", t, j);
        CHECK(((s.offset[t] + j) >> 1) == first + q && ((s.offset[t] + j) & 1) == h, "t %u position %u: pair of the definition", t, j);
        used[g + h]++;
        covered++;
        checked++;
      }
    }
    CHECK(covered == s.e[t], "t %u: %u of %u positions covered", t, covered, s.e[t]);
    // a modulation of m bits: symbol sym of the transmission is symbol P_t / m + sym of the row
    const uint32_t fs = nrharq::first_symbol(s, t, m);
    CHECK(uint64_t(fs) * m == s.offset[t], "t %u: the offset is a multiple of m %u", t, m);
    for (uint32_t sym = 0; sym < s.e[t] / m; sym++)
      for (uint32_t b = 0; b < m; b++) {
        const Where &w = row[size_t(fs + sym) * m + b];
        CHECK(w.t == int(t) && w.j == int(sym * m + b), "t %u symbol %u bit %u", t, sym, b);
      }
  }
  for (size_t g = 0; g < row.size(); g++) CHECK(used[g] == 1, "normal %zu used %d times", g, used[g]);
  return checked;
}

int main() {
  nrrm::Config c;
  CHECK(nrrm::make_config(2, 16, 0, -1, &c) == nullptr, "nr5g:2:16");
  long checked = 0;
  int cases = 0;
  // seams at odd and even positions, one to eight transmissions, every rv, rows longer than the buffer (repeats)
  const std::vector<std::vector<uint64_t>> lengths = {{481, 95, 96}, {480, 96, 96, 96}, {1}, {1, 1, 1, 1, 1, 1, 1, 1}, {3, 5, 7, 2, 9},
                                                      {800, 800}, {1700, 33}, {95, 481}, {2, 2, 2}, {37}};
  for (const auto &e : lengths)
    for (uint32_t r0 = 0; r0 < 4; r0++) {
      std::vector<uint32_t> rv(e.size());
      static const uint32_t order[4] = {0, 2, 3, 1};
      for (size_t t = 0; t < e.size(); t++) rv[t] = order[(t + r0) & 3];
      checked += check_sequence(c, e, rv, 1, 1);
      cases++;
    }
  // Qm and modulation bits that divide every E
  for (uint32_t qm : {2u, 4u, 6u, 8u}) {
    const std::vector<uint64_t> e = {480, 96, 96, 96};
    const std::vector<uint32_t> rv = {0, 2, 3, 1};
    checked += check_sequence(c, e, rv, qm, qm);
    checked += check_sequence(c, e, rv, 1, qm);
    cases += 2;
  }
  std::printf("sequences: %d cases, %ld positions agree with the literal row\n", cases, checked);

  // refusals
  {
    const uint64_t e[9] = {480, 96, 96, 96, 96, 96, 96, 96, 96};
    const uint32_t rv[9] = {0, 2, 3, 1, 0, 2, 3, 1, 0};
    CHECK(nrharq::sequence_error(e, rv, 8, 1, 1) == nullptr, "eight transmissions");
    CHECK(nrharq::sequence_error(e, rv, 0, 1, 1) != nullptr, "T = 0");
    CHECK(nrharq::sequence_error(e, rv, 9, 1, 1) != nullptr, "T = 9");
    CHECK(nrharq::sequence_error(e, rv, uint64_t(1) << 32, 1, 1) != nullptr, "T = 2^32");
    CHECK(nrharq::sequence_error(nullptr, rv, 2, 1, 1) != nullptr && nrharq::sequence_error(e, nullptr, 2, 1, 1) != nullptr, "null arrays");
    const uint32_t rv4[2] = {0, 4};
    CHECK(nrharq::sequence_error(e, rv4, 2, 1, 1) != nullptr && nrharq::sequence_error(e, rv4, 1, 1, 1) == nullptr, "rv = 4");
    const uint64_t odd[2] = {480, 95};
    CHECK(nrharq::sequence_error(odd, rv, 2, 2, 1) != nullptr, "Qm does not divide E_1");
    CHECK(nrharq::sequence_error(odd, rv, 2, 1, 5) == nullptr && nrharq::sequence_error(odd, rv, 2, 1, 2) != nullptr, "bits per symbol and E_1");
    CHECK(nrharq::sequence_error(odd, rv, 2, 0, 1) != nullptr && nrharq::sequence_error(odd, rv, 2, 9, 1) != nullptr, "Qm out of range");
    CHECK(nrharq::sequence_error(odd, rv, 2, 1, 0) != nullptr, "no bits per symbol");
    const uint64_t zero[2] = {480, 0};
    CHECK(nrharq::sequence_error(zero, rv, 2, 1, 1) != nullptr, "E = 0");
    const uint64_t big[3] = {0x7fffffffull, 1, 1};
    CHECK(nrharq::sequence_error(big, rv, 1, 1, 1) == nullptr && nrharq::sequence_error(big, rv, 2, 1, 1) != nullptr, "sum above 0x7fffffff");
    const uint64_t huge[2] = {uint64_t(1) << 40, 1};
    CHECK(nrharq::sequence_error(huge, rv, 2, 1, 1) != nullptr, "E above 0x7fffffff");
    const uint64_t full[8] = {0x0fffffffull, 0x0fffffffull, 0x0fffffffull, 0x0fffffffull, 0x0fffffffull, 0x0fffffffull, 0x0fffffffull, 0x10000006ull};
    CHECK(nrharq::sequence_error(full, rv, 8, 1, 1) == nullptr, "sum exactly 0x7fffffff");
    const nrharq::Sequence s = nrharq::make_sequence(full, rv, 8, 1);
    CHECK(s.offset[8] == 0x7fffffffu && nrharq::first_pair(s, 7) + nrharq::pairs(s, 7) - 1 == 0x3fffffffu, "the largest row's last pair");
    std::printf("refusals ok\n");
  }
  if (failures) {
    std::printf("nr harq driver: %d failures\n", failures);
    return 1;
  }
  std::printf("nr harq driver: ok\n");
  return 0;
}
