// 5G NR modulation mapper, soft demapper and scrambling (3GPP TS 38.211 5.1.3-5.1.6, 5.2.1, 6.3.1.1 / 7.3.1.1): the pure
// host part -- what a handle "nr5g-qam:QM" is made from, and what a call must satisfy before the GPU is touched.
// include/ldpc_toolbox.h, PART 8, is the definition; the kernels are in kernels_nr_qam.hip.h, their host side in
// device_nr_qam.h / .hip.h.
//
// A square QAM point is a pair of PAM levels: the even bits b_0, b_2, ... of a symbol select the I level, the odd ones the
// Q level.  With h = QM / 2 bits a_0 .. a_(h-1) per axis (a_0 the most significant bit of the level index u), the integer
// level is 38.211's nested form
//   L_u = (1 - 2 a_0) [2^(h-1) - (1 - 2 a_1) [2^(h-2) - ... (1 - 2 a_(h-1)) [1]]]
// and the amplitude A_u = L_u * a with a = sqrt(1.0 / norm), norm = 2, 10, 42, 170: unit mean symbol energy.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>

namespace ldpc {
namespace nrqam {

constexpr uint32_t kMaxAxisBits = 4, kMaxLevels = 16;

// L_u for h bits per axis
constexpr int32_t level(uint32_t h, uint32_t u) {
  int32_t v = 1;
  for (uint32_t t = h; t-- > 0;) {
    const int32_t sign = ((u >> (h - 1 - t)) & 1u) ? -1 : 1;
    v = t == h - 1 ? sign : sign * ((int32_t(1) << (h - 1 - t)) - v);
  }
  return v;
}
static_assert(level(1, 0) == 1 && level(1, 1) == -1, "QPSK");
static_assert(level(2, 0) == 1 && level(2, 1) == 3 && level(2, 2) == -1 && level(2, 3) == -3, "16QAM");
static_assert(level(3, 0) == 3 && level(3, 1) == 1 && level(3, 2) == 5 && level(3, 3) == 7 && level(3, 7) == -7, "64QAM");
static_assert(level(4, 0) == 5 && level(4, 3) == 1 && level(4, 4) == 11 && level(4, 7) == 15 && level(4, 15) == -15, "256QAM");

struct Config {
  uint32_t qm = 0;             // bits per symbol: 2, 4, 6, 8
  double a = 0.0;              // sqrt(1.0 / norm)
  double amp[kMaxLevels] = {};  // A_u = L_u * a, u < 2^h
  uint32_t h() const { return qm / 2; }
  uint32_t levels() const { return 1u << h(); }
  uint32_t points() const { return 1u << qm; }
};

// "nr5g-qam:QM" with QM in {2, 4, 6, 8}; false (and *err) for anything else
inline bool parse_spec(const std::string &spec, Config *c, std::string *err) {
  *c = Config();
  const std::string prefix = "nr5g-qam:";
  const std::string rest = spec.compare(0, prefix.size(), prefix) == 0 ? spec.substr(prefix.size()) : std::string();
  uint32_t qm = 0;
  if (rest.size() == 1 && rest[0] >= '0' && rest[0] <= '9') qm = static_cast<uint32_t>(rest[0] - '0');
  if (qm != 2 && qm != 4 && qm != 6 && qm != 8) {
    *err = "unknown NR modulation (expected nr5g-qam:QM with QM = 2, 4, 6 or 8)";
    return false;
  }
  const double norm[4] = {2.0, 10.0, 42.0, 170.0};
  c->qm = qm;
  c->a = std::sqrt(1.0 / norm[qm / 2 - 1]);
  for (uint32_t u = 0; u < c->levels(); u++) c->amp[u] = static_cast<double>(level(c->h(), u)) * c->a;
  return true;
}

// the level index of one axis of the point V = sum_j b_j << (QM-1-j): axis 0 takes b_0, b_2, ..., axis 1 b_1, b_3, ...
inline uint32_t axis_index(const Config &c, uint32_t v, uint32_t axis) {
  uint32_t u = 0;
  for (uint32_t t = 0; t < c.h(); t++) u |= ((v >> (c.qm - 1 - (2 * t + axis))) & 1u) << (c.h() - 1 - t);
  return u;
}

// c_init of a call: -1 = no scrambling, 0 .. 2^31 - 1 = the x2 seed of 38.211 5.2.1
inline bool c_init_ok(int64_t c_init) { return c_init >= -1 && c_init <= 0x7fffffffll; }

// What a run call must satisfy before the GPU is touched (nullptr), or why it does not.
inline const char *demod_argument_error(const Config &c, size_t llrs_len, size_t symbols_len, double sigma, int64_t c_init) {
  if (llrs_len % c.qm != 0 || llrs_len / c.qm != symbols_len) return "llrs_len is not QM * symbols_len";
  if (llrs_len > 0x7fffffffu) return "frame length out of range for the NR demapper";
  if (!(std::isfinite(sigma) && sigma > 0.0)) return "noise_sigma must be finite and greater than 0";
  if (!c_init_ok(c_init)) return "c_init must be -1 (no scrambling) or 0 .. 2^31 - 1";
  return nullptr;
}

// The demappers with a scale per symbol: the same without a sigma.  The scales are used as given and are not looked at.
inline const char *demap_csi_argument_error(const Config &c, size_t llrs_len, size_t symbols_len, int64_t c_init) {
  if (llrs_len % c.qm != 0 || llrs_len / c.qm != symbols_len) return "llrs_len is not QM * symbols_len";
  if (llrs_len > 0x7fffffffu) return "frame length out of range for the NR demapper";
  if (!c_init_ok(c_init)) return "c_init must be -1 (no scrambling) or 0 .. 2^31 - 1";
  return nullptr;
}

inline const char *mod_argument_error(const Config &c, size_t bits_len, size_t symbols_len, int64_t c_init) {
  if (bits_len % c.qm != 0 || bits_len / c.qm != symbols_len) return "bits_len is not QM * symbols_len";
  if (bits_len > 0x7fffffffu) return "frame length out of range for the NR mapper";
  if (!c_init_ok(c_init)) return "c_init must be -1 (no scrambling) or 0 .. 2^31 - 1";
  return nullptr;
}

inline const char *sequence_argument_error(size_t len, int64_t c_init) {
  if (len > 0x7fffffffu) return "sequence length out of range";
  if (c_init < 0 || c_init > 0x7fffffffll) return "c_init must be 0 .. 2^31 - 1";
  return nullptr;
}

// The vector accesses of the kernels: a symbol is one (re, im) load or store, the QM LLRs of a symbol 16-byte pieces.
inline const char *device_pointer_error(const void *symbols, const void *llrs, bool f64) {
  if (reinterpret_cast<uintptr_t>(symbols) % (f64 ? 16 : 8) != 0) return "the symbol buffer is not aligned to one (re, im) pair";
  if (llrs != nullptr && reinterpret_cast<uintptr_t>(llrs) % 16 != 0) return "the LLR buffer is not aligned to 16 bytes";
  return nullptr;
}

// a device scale array is one scalar load per lane: the alignment of its element
inline const char *scale_pointer_error(const void *scale, bool f64) {
  if (reinterpret_cast<uintptr_t>(scale) % (f64 ? 8 : 4) != 0) return "the scale buffer is not aligned to its element";
  return nullptr;
}

// What the simulator asks (nullptr), or why it refuses: whole symbols, and no DVB-S2 interleaver in front of the mapper
inline const char *sim_error(const Config &c, size_t n_tx, int64_t interleaving) {
  if (n_tx % c.qm != 0) return "the transmitted length is not a multiple of QM";
  if (interleaving != 0) return "the NR mapper takes no interleaving (NR's bit interleaver is the rate matcher's)";
  return nullptr;
}

}  // namespace nrqam
}  // namespace ldpc
