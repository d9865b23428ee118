// Stand-alone check of csrc/nr_rate_match.h (built under ASan/UBSan by tests/test_nr_rate_match_host.py): the closed
// forms the kernels run -- selection rank, both mapping directions, the interleaver -- against a literal loop of
// TS 38.212 5.4.2 written here, and every refusal of the validators.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../ldpc_toolbox_amd/csrc/nr_rate_match.h"

using namespace ldpc::nrrm;

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

// the standard's pseudo-code: -1 marks NULL
static std::vector<int> literal_selection(int bg, int zc, int fillers, int ncb, int rv, int e) {
  const int n = (bg == 1 ? 68 : 52) * zc, k = (bg == 1 ? 22 : 10) * zc, nbuf = n - 2 * zc;
  std::vector<int> buffer(nbuf);
  for (int d = 0; d < nbuf; d++) buffer[d] = d + 2 * zc;
  for (int c = k - fillers; c < k; c++) buffer[c - 2 * zc] = -1;
  static const int a[2][4] = {{0, 17, 33, 56}, {0, 13, 25, 43}};
  const int k0 = (a[bg - 1][rv] * ncb / nbuf) * zc;
  std::vector<int> sel(e);
  int kk = 0, j = 0;
  while (kk < e) {
    const int d = (k0 + j) % ncb;
    if (buffer[d] != -1) sel[kk++] = buffer[d];
    j++;
  }
  return sel;
}

static long check_case(int bg, int zc, int fillers, int ncb, int rv, int qm, int e) {
  Config c;
  const char *why = make_config(bg, zc, fillers, ncb, &c);
  CHECK(why == nullptr, "make_config(%d, %d, %d, %d): %s", bg, zc, fillers, ncb, why ? why : "");
  if (why) return 0;
  CHECK(transmission_error(e, rv, qm) == nullptr, "e %d rv %d qm %d", e, rv, qm);
  const Plan p = make_plan(c, e, rv, qm);
  const std::vector<int> sel = literal_selection(bg, zc, fillers, ncb, rv, e);
  std::vector<int> f(e), pos_of(e);
  for (int i = 0; i < qm; i++)
    for (int q = 0; q < e / qm; q++) {
      f[i + q * qm] = sel[i * (e / qm) + q];
      pos_of[i * (e / qm) + q] = i + q * qm;
    }
  for (int j = 0; j < e; j++) {
    CHECK(column_of_selection(p, j) == uint32_t(sel[j]), "bg %d zc %d f %d ncb %d rv %d e %d: selection %d", bg, zc, fillers, ncb, rv, e, j);
    CHECK(position_of_selection(p, j) == uint32_t(pos_of[j]), "qm %d e %d: position of %d", qm, e, j);
    CHECK(selection_of_position(p, pos_of[j]) == uint32_t(j), "qm %d e %d: selection of %d", qm, e, pos_of[j]);
    CHECK(column_of_position(p, j) == uint32_t(f[j]), "bg %d zc %d f %d ncb %d rv %d qm %d e %d: position %d", bg, zc, fillers, ncb, rv, qm, e, j);
  }
  // the receive side: per column, the carriers in ascending order
  long carried = 0;
  for (uint32_t col = 0; col < c.n; col++) {
    std::vector<uint32_t> want;
    for (int j = 0; j < e; j++)
      if (uint32_t(sel[j]) == col) want.push_back(j);
    const uint32_t r = first_selection_of_column(p, col);
    const bool filler = col >= c.k - c.fillers && col < c.k;
    CHECK((r == kFiller) == filler, "column %u filler", col);
    if (filler) {
      CHECK(want.empty(), "filler column %u is transmitted", col);
      continue;
    }
    std::vector<uint32_t> got;
    for (uint64_t j = r; j < uint64_t(e); j += p.l) got.push_back(uint32_t(j));
    CHECK(got == want, "bg %d zc %d f %d ncb %d rv %d e %d: carriers of column %u (%zu, want %zu)", bg, zc, fillers, ncb, rv, e, col,
          got.size(), want.size());
    if (col < 2 * c.zc || col - 2 * c.zc >= c.ncb) CHECK(r == kNotSent, "column %u outside the buffer", col);
    carried += long(got.size());
  }
  CHECK(carried == e, "repeat counts sum to %ld, not E = %d", carried, e);
  return 1;
}

static void check_grid() {
  long cases = 0;
  bool k0_in_fillers = false;
  for (int bg = 1; bg <= 2; bg++)
    for (int zc = 2; zc <= 3; zc++) {
      const int n = (bg == 1 ? 68 : 52) * zc, k = (bg == 1 ? 22 : 10) * zc, nbuf = n - 2 * zc;
      const int fl[4] = {0, 1, 4, 2 * zc + 1};
      for (int fillers : fl) {
        // the whole buffer, an odd cut, the short one, and one that ends inside the filler run (or at half the buffer)
        const int ncbs[4] = {nbuf, nbuf - 7, 56, fillers > 1 ? k - 2 * zc - fillers + 2 : nbuf / 2};
        for (int ncb : ncbs) {
          Config c;
          if (make_config(bg, zc, fillers, ncb, &c)) {
            CHECK(false, "grid configuration refused");
            continue;
          }
          for (int rv = 0; rv < 4; rv++) {
            const uint32_t k0 = k0_of(c, rv);
            if (k0 >= c.fs && k0 < c.fs + c.fillers) k0_in_fillers = true;
            static const int qms[5] = {1, 2, 4, 6, 8};
            for (int qm : qms) {
              const int l = int(c.l);
              const int es[5] = {3 * qm, std::max(l / 2 / qm, 1) * qm, std::max(l / qm, 1) * qm, (l / qm + 1) * qm, (3 * nbuf / qm) * qm};
              for (int e : es) cases += check_case(bg, zc, fillers, ncb, rv, qm, e);
            }
          }
        }
      }
    }
  CHECK(k0_in_fillers, "no case with k0 inside the filler run");
  {  // the case the header's comment names: BG2, Zc 2, F 4, Ncb 56, rv 1 -> k0 = 14 inside the fillers 12..15
    Config c;
    CHECK(make_config(2, 2, 4, 56, &c) == nullptr && k0_of(c, 1) == 14 && c.fs == 12, "the k0-inside-the-fillers case");
  }
  std::printf("grid: %ld cases agree with the literal loop\n", cases);
}

static void check_k0_tables() {
  struct {
    int bg, ncb;
    uint32_t k0[4];
  } rows[] = {{1, 25344, {0, 6528, 12672, 21504}}, {2, 19200, {0, 4992, 9600, 16512}}, {1, 16896, {0, 4224, 8448, 14208}}};
  for (const auto &r : rows) {
    Config c;
    CHECK(make_config(r.bg, 384, 0, r.ncb, &c) == nullptr, "zc 384");
    for (uint32_t rv = 0; rv < 4; rv++) CHECK(k0_of(c, rv) == r.k0[rv], "bg %d ncb %d rv %u: %u", r.bg, r.ncb, rv, k0_of(c, rv));
  }
  Config c;
  CHECK(make_config(1, 384, 0, -1, &c) == nullptr && c.n == 26112 && c.k == 8448 && c.nbuf == 25344 && c.ncb == 25344 && c.l == 25344,
        "nr5g:1:384 defaults");
  std::printf("k0 tables ok\n");
}

static void check_refusals() {
  Config c;
  c.n = 77;  // (a refusal leaves *c as it was)
  CHECK(make_config(0, 2, 0, -1, &c) && make_config(3, 2, 0, -1, &c), "base graph");
  CHECK(make_config(1, 0, 0, -1, &c) && make_config(1, 385, 0, -1, &c) && make_config(1, -2, 0, -1, &c), "lifting size");
  CHECK(make_config(2, 2, -1, -1, &c) && make_config(2, 2, 17, -1, &c) && make_config(1, 2, 41, -1, &c), "fillers");
  CHECK(make_config(2, 2, 0, 0, &c) && make_config(2, 2, 0, 101, &c), "ncb");
  CHECK(make_config(2, 2, 16, 16, &c) && make_config(2, 2, 16, 3, &c), "a buffer of fillers only: L = 0");
  CHECK(c.n == 77, "a refused configuration was written");
  CHECK(make_config(2, 2, 16, 17, &c) == nullptr && c.l == 1 && c.fs == 0, "L = 1");
  CHECK(make_config(2, 2, 16, -1, &c) == nullptr && c.l == 84, "F = K - 2 Zc");
  CHECK(make_config(2, 2, 4, 100, &c) == nullptr && c.l == 96 && c.fs == 12 && c.n == 104 && c.k == 20, "BG2 Zc 2");
  CHECK(transmission_error(0, 0, 1) && transmission_error(12, 4, 1) && transmission_error(12, 0, 0) && transmission_error(12, 0, 9) &&
            transmission_error(13, 0, 2) && transmission_error(0x80000000ull, 0, 1) && transmission_error(uint64_t(1) << 32, 0, 1),
        "transmission refusals");
  CHECK(!transmission_error(0x7fffffffull, 3, 1) && !transmission_error(8, 0, 8) && !transmission_error(1, 0, 1), "transmissions");
  CHECK(match_argument_error(c, 103, 12, 0, 1) && match_argument_error(c, 0, 12, 0, 1) && !match_argument_error(c, 104, 12, 0, 1) &&
            match_argument_error(c, 104, 12, 0, 5),
        "match arguments");
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  CHECK(recover_argument_error(c, 104, 12, 0, 1, 0.0) && recover_argument_error(c, 104, 12, 0, 1, -1.0) &&
            recover_argument_error(c, 104, 12, 0, 1, nan) && recover_argument_error(c, 104, 12, 0, 1, -inf) &&
            recover_argument_error(c, 100, 12, 0, 1, 1.0) && recover_argument_error(c, 104, 12, 7, 1, 1.0),
        "recover refusals");
  CHECK(!recover_argument_error(c, 104, 12, 0, 1, inf) && !recover_argument_error(c, 104, 12, 0, 1, 1e-300), "recover arguments");
  std::printf("refusals ok\n");
}

// the largest E: the mappings stay inside [0, E) and invert each other where 32-bit products would wrap
static void check_large() {
  Config c;
  CHECK(make_config(1, 384, 100, 20000, &c) == nullptr, "config");
  const uint32_t e = 0x7fffffffu / 8 * 8;
  for (uint32_t qm : {1u, 8u}) {
    const Plan p = make_plan(c, e, 3, qm);
    for (uint64_t j = 0; j < e; j += 9999991) {
      const uint32_t pos = position_of_selection(p, uint32_t(j));
      CHECK(pos < e && selection_of_position(p, pos) == j, "qm %u: selection %llu", qm, (unsigned long long)j);
      CHECK(pos == (j % (e / qm)) * qm + j / (e / qm), "qm %u: position of %llu", qm, (unsigned long long)j);
      const uint32_t col = column_of_selection(p, uint32_t(j));
      const uint32_t r = first_selection_of_column(p, col);
      CHECK(col >= 768 && col < 768 + 20000 && r < p.l && (j - r) % p.l == 0, "selection %llu -> column %u -> rank %u", (unsigned long long)j, col, r);
    }
    CHECK(position_of_selection(p, e - 1) == e - 1, "the last selection index");
  }
  std::printf("large E ok\n");
}

int main() {
  check_grid();
  check_k0_tables();
  check_refusals();
  check_large();
  if (failures) {
    std::printf("nr rate match driver: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("nr rate match driver: ok\n");
  return 0;
}
