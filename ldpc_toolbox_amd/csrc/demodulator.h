// Batched soft demapper on the GPU, for the ldpc_toolbox_demod_* entries of the C ABI: received symbols
// [batch][symbols_len] -> channel LLRs [batch][llrs_len] in codeword order (deinterleaved), the layout the decoder's
// decode_batch*_device entries take.  A positive LLR means bit 0 (the reference's convention).
//
//   * BPSK (modulation.rs:123-141): real symbols, llr = scale * x with scale = -2 / sigma^2.
//   * table constellations of m = 1..5 bits, M = 2^m points: point p_V at index V = sum_j b_j << (m-1-j) (b0 the most
//     significant bit), complex symbols.  With scale = 1 / sigma^2 and sr = re * scale, si = im * scale:
//       d_V   = sr * p_V.re + si * p_V.im   [ - (0.5 * scale) * e_V  with e_V = |p_V|^2, when the table has an energy term ]
//       llr_j = F({d_V : bit j of V = 0}) - F({d_V : bit j of V = 1}),  F a left fold over ascending V
//     with the fold step maxstar (exact: modulation.rs:286-288) or, for max-log, the maximum that ignores a NaN operand
//     and orders -0 < +0 (IEEE 754-2019 maximumNumber: what v_max_f32 / v_max_f64 compute).  The 8PSK table and the exact
//     step give Psk8Demodulator::demodulate_symbol (modulation.rs:228-264) bit for bit.
//   * the LLR of interleaved position i = m * sym + j goes to gen::deinterleaved_position(i, llrs_len, interleaving).
//
// f64 entries: all of it in f64.  f32 entries: exact = symbols widened, the f64 arithmetic, one rounding per LLR;
// max-log = the same formulas in f32, scale and 0.5 * scale * e_V rounded to f32 once.
// The kernels are in kernels_demod.hip.h; the host side (demodulator.hip.h) is part of the simulator's translation unit.
//
// The same handle is the transmit side (reference: trait Modulator, modulation.rs:40-62, and AwgnChannel::add_noise,
// channel.rs:60-81); the kernels are in kernels_channel.hip.h.
//   * modulator: bits [batch][bits_len] (a byte equal to 1 is a one, anything else a zero) -> symbols [batch][symbols_len].
//     Interleaved position i = m * sym + j carries codeword position gen::deinterleaved_position(i, bits_len, interleaving)
//     (the interleaver of interleaving.rs:40-58, which the demapper undoes); V = sum_j b_j << (m-1-j); the symbol is
//     (p_V.re, p_V.im) -- the handle's doubles, or each rounded once to float.  BPSK: reals, +1 for a one, -1 for a zero.
//   * AWGN, in place, row r = frame first_frame + r: symbol s gets (z0, z1) = gen::normal_pair(seed, frame, s),
//     re += sigma * z0, im += sigma * z1; BPSK position j uses pair j / 2, z0 for even j and z1 for odd j (the keying of
//     gen::awgn_llr_kernel).  f64: x + sigma * (double)z.  f32: x + (float)sigma * z.  Each product and sum rounded once.
//   * Rayleigh block fading with perfect CSI behind a one-tap equaliser, in place, complex symbols only: the received
//     h x + sigma z divided by h is x + sigma z / h, and the phase of h does not change the law of z / h, so only a = |h| is
//     drawn: one gain per `block` consecutive symbols of a frame (gen::fading_scale: af, sigma_e = sigma / af, scale =
//     1 / sigma_e^2).  Symbol s gets the AWGN channel's pair at sigma_e, and scale[s] -- what the NR demapper with a scale per
//     symbol takes.  f64: x + sigma_e * (double)z.  f32: x + (float)sigma_e * z, scale rounded once to float.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "device_stage.h"

namespace ldpc {

constexpr uint32_t kDemodMaxBits = 5, kDemodMaxPoints = 32;

// what a demodulator handle is made from: pure host data
struct Constellation {
  uint32_t bits = 0;    // m
  bool bpsk = false;    // real symbols, no table
  bool energy = false;  // d_V carries the energy term
  double re[kDemodMaxPoints] = {}, im[kDemodMaxPoints] = {}, e[kDemodMaxPoints] = {};
  uint32_t points() const { return 1u << bits; }
};

// "BPSK" | "QPSK" | "8PSK" (the DVB-S2 mappings); false for any other name
inline bool named_constellation(const std::string &name, Constellation *c) {
  const double a = 0.70710678118654757;  // (0.5f64).sqrt()
  *c = Constellation();
  if (name == "BPSK") {
    c->bits = 1;
    c->bpsk = true;
    return true;
  }
  if (name == "QPSK") {  // 00 at pi/4, 10 at 3 pi/4
    c->bits = 2;
    for (uint32_t v = 0; v < 4; v++) {
      c->re[v] = (v & 2u) ? -a : a;
      c->im[v] = (v & 1u) ? -a : a;
    }
    return true;
  }
  if (name == "8PSK") {  // modulation.rs:168-179, indexed by V = b0 b1 b2
    const double p[8][2] = {{a, a}, {1.0, 0.0}, {-1.0, 0.0}, {-a, -a}, {0.0, 1.0}, {a, -a}, {-a, a}, {0.0, -1.0}};
    c->bits = 3;
    for (uint32_t v = 0; v < 8; v++) {
      c->re[v] = p[v][0];
      c->im[v] = p[v][1];
    }
    return true;
  }
  return false;
}

// 2^bits (re, im) pairs; false (and *err) for bits outside 1..5 or a point that is not finite
inline bool table_constellation(const double *points_re_im, uint32_t bits, bool energy, Constellation *c, std::string *err) {
  *c = Constellation();
  if (bits < 1 || bits > kDemodMaxBits) {
    *err = "bits_per_symbol must be 1..5";
    return false;
  }
  if (!points_re_im) {
    *err = "null constellation table";
    return false;
  }
  c->bits = bits;
  c->energy = energy;
  for (uint32_t v = 0; v < c->points(); v++) {
    const double re = points_re_im[2 * v], im = points_re_im[2 * v + 1];
    if (!std::isfinite(re) || !std::isfinite(im)) {
      *err = "constellation point is not finite";
      return false;
    }
    c->re[v] = re;
    c->im[v] = im;
    c->e[v] = re * re + im * im;
  }
  return true;
}

// What a run call must satisfy before the GPU is touched (nullptr), or why it does not.
inline const char *demod_argument_error(const Constellation &c, size_t llrs_len, size_t symbols_len, double sigma,
                                        int32_t interleaving) {
  if (llrs_len % c.bits != 0 || llrs_len / c.bits != symbols_len) return "llrs_len is not bits_per_symbol * symbols_len";
  if (llrs_len > 0x7fffffffu) return "frame length out of range for the demodulator";
  if (!(std::isfinite(sigma) && sigma > 0.0)) return "noise_sigma must be finite and greater than 0";
  const uint64_t columns = static_cast<uint64_t>(interleaving < 0 ? -static_cast<int64_t>(interleaving) : interleaving);
  if (columns != 0 && llrs_len % columns != 0) return "interleaving does not divide llrs_len";
  return nullptr;
}

// The same for a modulator call: bits [batch][bits_len] -> symbols [batch][symbols_len].
inline const char *mod_argument_error(const Constellation &c, size_t bits_len, size_t symbols_len, int32_t interleaving) {
  if (bits_len % c.bits != 0 || bits_len / c.bits != symbols_len) return "bits_len is not bits_per_symbol * symbols_len";
  if (bits_len > 0x7fffffffu) return "frame length out of range for the modulator";
  const uint64_t columns = static_cast<uint64_t>(interleaving < 0 ? -static_cast<int64_t>(interleaving) : interleaving);
  if (columns != 0 && bits_len % columns != 0) return "interleaving does not divide bits_len";
  return nullptr;
}

// ... and for an AWGN call on [batch][symbols_len] symbols (channel.rs:52-53: sigma >= 0; a noise pair is a 32-bit index)
inline const char *awgn_argument_error(size_t symbols_len, double sigma) {
  if (symbols_len > 0x7fffffffu) return "frame length out of range for the channel";
  if (!(std::isfinite(sigma) && sigma >= 0.0)) return "noise_sigma must be finite and not negative";
  return nullptr;
}

// ... and for a fading call (complex handles only): symbols and scale [batch][symbols_len], one gain per `block` symbols
inline const char *fading_argument_error(const Constellation &c, size_t symbols_len, double sigma, uint32_t block) {
  if (c.bpsk) return "the fading channel takes complex symbols, not a BPSK handle's reals";
  if (symbols_len > 0x7fffffffu) return "frame length out of range for the channel";
  if (!(std::isfinite(sigma) && sigma > 0.0)) return "noise_sigma must be finite and greater than 0";
  if (block == 0) return "the fading block must be at least one symbol";
  return nullptr;
}

// its device buffers: a symbol is one (re, im) load and store, a scale one scalar store
inline const char *fading_pointer_error(const void *symbols, const void *scale, bool f64) {
  if (reinterpret_cast<uintptr_t>(symbols) % (f64 ? 16 : 8) != 0) return "the symbol buffer is not aligned to one (re, im) pair";
  if (reinterpret_cast<uintptr_t>(scale) % (f64 ? 8 : 4) != 0) return "the scale buffer is not aligned to its element";
  return nullptr;
}

// mean symbol energy of a table: sum_V |p_V|^2 / 2^m (BPSK: 1)
inline double mean_energy(const Constellation &c) {
  if (c.bpsk) return 1.0;
  double sum = 0.0;
  for (uint32_t v = 0; v < c.points(); v++) sum += c.re[v] * c.re[v] + c.im[v] * c.im[v];
  return sum / static_cast<double>(c.points());
}

// What the simulator asks of a constellation for frames of n_tx bits (nullptr), or why it refuses it: whole symbols, and
// unit mean energy -- noise_sigma = sqrt(0.5 / (rate * m * EbN0)) (ber.rs:299-302) presumes it.
inline const char *sim_constellation_error(const Constellation &c, size_t n_tx) {
  if (c.bpsk) return nullptr;
  if (c.bits < 1 || c.bits > kDemodMaxBits) return "bits_per_symbol must be 1..5";
  if (n_tx % c.bits != 0) return "the transmitted length is not a multiple of bits_per_symbol";
  const double e = mean_energy(c);
  if (!(e >= 1.0 - 1e-6 && e <= 1.0 + 1e-6)) return "the constellation's mean energy is not 1 (the Eb/N0 axis presumes unit symbol energy)";
  return nullptr;
}

class DeviceDemodulator : public DeviceStage {
 public:
  // nullptr (and *err) when there is no usable GPU: there is no CPU path here.
  static DeviceDemodulator *create(const Constellation &c, int device, std::string *err);
  ~DeviceDemodulator();

  // symbols [batch][symbols_len] (re, im) pairs -- reals for BPSK -- and llrs [batch][llrs_len], float or double (f64),
  // the arguments already checked (demod_argument_error).  0, or -2 on a HIP failure.
  // Device pointers; stream: launch stream (nullptr = the handle's own stream, ordered after everything queued on the
  // legacy default stream at the time of the call, and synchronised on return).
  int run_device(const void *symbols, void *llrs, bool f64, size_t symbols_len, size_t llrs_len, size_t batch, double sigma,
                 int32_t interleaving, bool max_log, hipStream_t stream);
  // Host pointers: staged through device buffers of the handle, synchronous.
  int run_host(const void *symbols, void *llrs, bool f64, size_t symbols_len, size_t llrs_len, size_t batch, double sigma,
               int32_t interleaving, bool max_log);
  // Modulator: bits [batch][bits_len] -> symbols, the arguments already checked (mod_argument_error); pointers and
  // stream as in run_device / run_host.
  int mod_device(const uint8_t *bits, void *symbols, bool f64, size_t bits_len, size_t symbols_len, size_t batch,
                 int32_t interleaving, hipStream_t stream);
  int mod_host(const uint8_t *bits, void *symbols, bool f64, size_t bits_len, size_t symbols_len, size_t batch,
               int32_t interleaving);
  // AWGN in place on symbols [batch][symbols_len] (awgn_argument_error)
  int awgn_device(void *symbols, bool f64, size_t symbols_len, size_t batch, double sigma, uint64_t seed, uint64_t first_frame,
                  hipStream_t stream);
  int awgn_host(void *symbols, bool f64, size_t symbols_len, size_t batch, double sigma, uint64_t seed, uint64_t first_frame);
  // Rayleigh block fading in place on symbols [batch][symbols_len], writing scale [batch][symbols_len] (fading_argument_error)
  int fading_device(void *symbols, void *scale, bool f64, size_t symbols_len, size_t batch, double sigma, uint32_t block, uint64_t seed,
                    uint64_t first_frame, hipStream_t stream);
  int fading_host(void *symbols, void *scale, bool f64, size_t symbols_len, size_t batch, double sigma, uint32_t block, uint64_t seed,
                  uint64_t first_frame);

 private:
  explicit DeviceDemodulator(int device) : DeviceStage("demodulator", device) {}
  template <typename IO>
  void launch(const IO *symbols, IO *llrs, size_t symbols_len, size_t llrs_len, size_t batch, double sigma,
              int32_t interleaving, bool max_log, hipStream_t s);

  Constellation c_;
};

}  // namespace ldpc
