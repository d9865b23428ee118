// CPU check of the pure host functions of the constellation handle's transmit side (csrc/demodulator.h): the argument
// checks of the modulator and channel entries and what the simulator asks of a constellation.  A stand-alone program,
// built under ASan/UBSan.  Edges: length 0, INT32_MIN interleaving (its magnitude does not fit an int32_t), the largest
// length, a 32-point table, mean energies either side of the 1e-6 band.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../ldpc_toolbox_amd/csrc/demodulator.h"

using namespace ldpc;

#define REQUIRE(c)                                                        \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      return 1;                                                           \
    }                                                                     \
  } while (0)

// 2^bits points on rings of radius r0 and r1 (alternating), scaled by `gain`
static std::vector<double> rings(uint32_t bits, double r0, double r1, double gain) {
  const uint32_t n = 1u << bits;
  std::vector<double> p(2 * n);
  for (uint32_t v = 0; v < n; v++) {
    const double r = gain * ((v & 1u) ? r1 : r0), phi = 6.283185307179586 * v / n;
    p[2 * v] = r * std::cos(phi);
    p[2 * v + 1] = r * std::sin(phi);
  }
  return p;
}

int main() {
  const int32_t kMin = std::numeric_limits<int32_t>::min();
  Constellation bpsk, qpsk, psk8;
  REQUIRE(named_constellation("BPSK", &bpsk) && named_constellation("QPSK", &qpsk) && named_constellation("8PSK", &psk8));

  // ---- mod_argument_error ----
  REQUIRE(mod_argument_error(psk8, 24, 8, 0) == nullptr);
  REQUIRE(mod_argument_error(psk8, 24, 8, 3) == nullptr && mod_argument_error(psk8, 24, 8, -3) == nullptr);
  REQUIRE(mod_argument_error(psk8, 24, 8, 24) == nullptr && mod_argument_error(psk8, 24, 8, -24) == nullptr);
  REQUIRE(mod_argument_error(psk8, 24, 8, 5) != nullptr && mod_argument_error(psk8, 24, 8, -48) != nullptr);
  REQUIRE(mod_argument_error(psk8, 24, 7, 0) != nullptr && mod_argument_error(psk8, 25, 8, 0) != nullptr);
  REQUIRE(mod_argument_error(psk8, 23, 8, 0) != nullptr);
  // length 0: every column count divides it, INT32_MIN included (|INT32_MIN| is formed in 64 bits)
  REQUIRE(mod_argument_error(psk8, 0, 0, 0) == nullptr && mod_argument_error(psk8, 0, 0, 7) == nullptr);
  REQUIRE(mod_argument_error(psk8, 0, 0, kMin) == nullptr && mod_argument_error(bpsk, 0, 0, kMin) == nullptr);
  REQUIRE(mod_argument_error(psk8, 0, 1, 0) != nullptr);
  REQUIRE(mod_argument_error(psk8, 24, 8, kMin) != nullptr && mod_argument_error(bpsk, 0x7fffffffu, 0x7fffffffu, kMin) != nullptr);
  REQUIRE(mod_argument_error(bpsk, 0x7fffffffu, 0x7fffffffu, 0) == nullptr);
  REQUIRE(mod_argument_error(bpsk, 0x7fffffffu, 0x7fffffffu, 0x7fffffff) == nullptr);
  REQUIRE(mod_argument_error(bpsk, 0x80000000u, 0x80000000u, 0) != nullptr);
  REQUIRE(mod_argument_error(qpsk, 0x80000000u, 0x40000000u, 0) != nullptr);
  REQUIRE(mod_argument_error(qpsk, 0x7ffffffeu, 0x3fffffffu, 2) == nullptr);
  // a product that wraps in 64 bits must not pass for a match: 2 * (2^63 + 4) == 8 (mod 2^64)
  REQUIRE(mod_argument_error(qpsk, 8, (size_t(1) << 63) + 4, 0) != nullptr);

  // ---- awgn_argument_error ----
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  REQUIRE(awgn_argument_error(8, 0.0) == nullptr && awgn_argument_error(8, -0.0) == nullptr);
  REQUIRE(awgn_argument_error(0, 0.5) == nullptr && awgn_argument_error(0x7fffffffu, 5e-324) == nullptr);
  REQUIRE(awgn_argument_error(8, -5e-324) != nullptr && awgn_argument_error(8, -1.0) != nullptr);
  REQUIRE(awgn_argument_error(8, inf) != nullptr && awgn_argument_error(8, -inf) != nullptr && awgn_argument_error(8, nan) != nullptr);
  REQUIRE(awgn_argument_error(0x80000000u, 0.5) != nullptr);

  // ---- mean_energy / sim_constellation_error ----
  REQUIRE(mean_energy(bpsk) == 1.0 && std::fabs(mean_energy(qpsk) - 1.0) < 1e-15 && std::fabs(mean_energy(psk8) - 1.0) < 1e-15);
  REQUIRE(sim_constellation_error(bpsk, 7) == nullptr);  // BPSK: any length
  REQUIRE(sim_constellation_error(qpsk, 8) == nullptr && sim_constellation_error(qpsk, 7) != nullptr);
  REQUIRE(sim_constellation_error(psk8, 312) == nullptr && sim_constellation_error(psk8, 313) != nullptr);
  REQUIRE(sim_constellation_error(psk8, 0) == nullptr);
  std::string err;
  for (uint32_t bits = 1; bits <= 5; bits++) {
    // radii 0.6 and r1 with (0.36 + r1^2) / 2 = 1: unit mean energy, unequal point energies
    const double r1 = std::sqrt(2.0 - 0.36);
    Constellation c;
    const std::vector<double> unit = rings(bits, 0.6, r1, 1.0);
    REQUIRE(table_constellation(unit.data(), bits, true, &c, &err) && c.points() == (1u << bits));
    REQUIRE(std::fabs(mean_energy(c) - 1.0) < 1e-12);
    REQUIRE(sim_constellation_error(c, 780 * bits) == nullptr);
    REQUIRE((sim_constellation_error(c, 780 * bits + 1) == nullptr) == (bits == 1));
    // mean energy 1.1 and 0.9: refused; 1 +- 5e-7: inside the band; 1 +- 2e-6: outside
    for (double e : {1.1, 0.9, 1.0 + 2e-6, 1.0 - 2e-6}) {
      const std::vector<double> p = rings(bits, 0.6, r1, std::sqrt(e));
      REQUIRE(table_constellation(p.data(), bits, true, &c, &err));
      REQUIRE(sim_constellation_error(c, 780 * bits) != nullptr);
    }
    for (double e : {1.0 + 5e-7, 1.0 - 5e-7}) {
      const std::vector<double> p = rings(bits, 0.6, r1, std::sqrt(e));
      REQUIRE(table_constellation(p.data(), bits, false, &c, &err));
      REQUIRE(sim_constellation_error(c, 780 * bits) == nullptr);
    }
  }
  // a 32-point table fills the arrays to their last element
  {
    Constellation c;
    const std::vector<double> p = rings(5, 1.0, 1.0, 1.0);
    REQUIRE(table_constellation(p.data(), 5, false, &c, &err));
    REQUIRE(c.re[31] == p[62] && c.im[31] == p[63] && c.e[31] == p[62] * p[62] + p[63] * p[63]);
    REQUIRE(sim_constellation_error(c, 780) == nullptr && sim_constellation_error(c, 782) != nullptr);
    REQUIRE(mod_argument_error(c, 780, 156, -5) == nullptr && mod_argument_error(c, 780, 156, 7) != nullptr);
  }
  // an overflowing table: the mean energy is not finite, and it is refused
  {
    Constellation c;
    std::vector<double> p = rings(2, 1.0, 1.0, 1.0);
    p[0] = 1e200;
    REQUIRE(table_constellation(p.data(), 2, false, &c, &err));
    REQUIRE(sim_constellation_error(c, 8) != nullptr);
  }
  std::printf("channel args driver: ok\n");
  return 0;
}
