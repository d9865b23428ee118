// extern "C" boundary: the reference's nine symbols + the batched extension
// (include/ldpc_toolbox.h).  Behavioural model: /root/reference/src/c_api/decoder.rs and
// /root/reference/src/c_api/encoder.rs; every entry point below cites what it replaces.
#include "../../include/ldpc_toolbox.h"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "codes.h"
#include "demodulator.h"
#include "device_bch.h"
#include "device_decoder.h"
#include "device_encoder.h"
#include "device_nr_link.h"
#include "device_nr_qam.h"
#include "device_nr_rm.h"
#include "device_nr_tb.h"
#include "encoder.h"
#include "implementation.h"
#include "simulator.h"
#include "soft_i8.h"
#include "sparse.h"

namespace {

thread_local std::string g_last_error;

void set_error(const std::string &m) { g_last_error = m; }

bool parse_puncturing(const char *s, std::vector<uint8_t> *out) {
  return ldpc::parse_puncturing_pattern(s ? s : "", out);
}

bool read_file(const char *path, std::string *out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  std::ostringstream ss;
  ss << f.rdbuf();
  *out = ss.str();
  return true;
}

struct DecoderHandle {
  std::unique_ptr<ldpc::DeviceDecoder> dec;
};

struct EncoderHandle {
  ldpc::Encoder enc;
  std::vector<uint8_t> pattern;
  size_t out_len = 0;
  std::vector<uint8_t> scratch;
  // the batched entries' device state: made by the ..._on_device constructor, or at the first batched call
  std::unique_ptr<ldpc::DeviceEncoder> dev;
};

struct DemodHandle {
  ldpc::Constellation c;
  int device = 0;
  // the device state: made at the first run
  std::unique_ptr<ldpc::DeviceDemodulator> dev;
};

struct BchHandle {
  ldpc::bch::Code code;
  int device = 0;
  // the device state: made at the first batched call
  std::unique_ptr<ldpc::DeviceBch> dev;
};

struct NrRmHandle {
  ldpc::nrrm::Config c;
  int device = 0;
  // the device state: made at the first batched call
  std::unique_ptr<ldpc::DeviceNrRm> dev;
};

struct NrTbHandle {
  ldpc::nrtb::Config c;
  int device = 0;
  // the device state: made at the first batched call
  std::unique_ptr<ldpc::DeviceNrTb> dev;
};

struct NrQamHandle {
  ldpc::nrqam::Config c;
  int device = 0;
  // the device state: made at the first run
  std::unique_ptr<ldpc::DeviceNrQam> dev;
};

struct NrLinkHandle {
  ldpc::nrlink::Config c;
  ldpc::Implementation impl;
  uint32_t slots = 0;
  int device = 0;
  // what the setters hold until the device state exists, and then hand on
  bool max_log = false;
  uint64_t pass_elements = ldpc::nrlink::kPassElements;
  double filler_llr = 0.0;  // (the constructor entry sets +inf)
  uint32_t soft_bits = 32;  // 8: the PART 12 mode; fixed once the device state exists
  // the device state, the HARQ slots included: made at the first batched call
  std::unique_ptr<ldpc::DeviceNrLink> dev;
};

// a device index: decimal digits only (no sign, no trailing characters)
bool parse_device_index(const char *s, int *out) {
  if (!s || !*s) return false;
  char *end = nullptr;
  errno = 0;
  const long v = std::strtol(s, &end, 10);
  if (errno != 0 || end == s || *end != '\0' || s[0] < '0' || s[0] > '9' || v < 0 || v > 1 << 20) return false;
  *out = static_cast<int>(v);
  return true;
}

// LDPC_TOOLBOX_DEVICE: GPU of the constructors that take no device argument; -1 = unusable value
int default_device() {
  const char *s = std::getenv("LDPC_TOOLBOX_DEVICE");
  if (!s || !*s) return 0;
  int d = 0;
  return parse_device_index(s, &d) ? d : -1;
}

void *make_decoder(const std::string &alist, const char *implementation, const char *puncturing,
                   int device) {
  g_last_error.clear();
  if (!implementation) {
    set_error("invalid decoder implementation");
    return nullptr;
  }
  std::string name = implementation;
  const size_t at = name.find("@hip");
  if (at != std::string::npos) {
    const std::string suffix = name.substr(at + 4);
    name = name.substr(0, at);
    if (!suffix.empty()) {
      if (suffix[0] != ':') {
        set_error("invalid device suffix (expected @hip or @hip:N)");
        return nullptr;
      }
      if (!parse_device_index(suffix.c_str() + 1, &device)) {
        set_error("invalid device suffix (expected @hip or @hip:N with N a decimal GPU index)");
        return nullptr;
      }
    }
  }
  if (device < 0) {
    set_error("LDPC_TOOLBOX_DEVICE is not a decimal GPU index");
    return nullptr;
  }
  ldpc::SparseMatrix h;
  std::string err;
  if (!ldpc::SparseMatrix::from_alist(alist, &h, &err)) {
    set_error(err);
    return nullptr;
  }
  ldpc::Implementation impl;
  if (!ldpc::parse_implementation(name, &impl, &err)) {
    set_error(err);
    return nullptr;
  }
  std::vector<uint8_t> pattern;
  if (!parse_puncturing(puncturing, &pattern)) {
    set_error("invalid puncturing pattern");
    return nullptr;
  }
  ldpc::DeviceDecoder *d = ldpc::DeviceDecoder::create(h, impl, pattern, device, &err);
  if (!d) {
    set_error(err);
    return nullptr;
  }
  auto *handle = new DecoderHandle();
  handle->dec.reset(d);
  return handle;
}

void *make_encoder(const std::string &alist, const char *puncturing) {
  g_last_error.clear();
  ldpc::SparseMatrix h;
  std::string err;
  if (!ldpc::SparseMatrix::from_alist(alist, &h, &err)) {
    set_error(err);
    return nullptr;
  }
  auto handle = std::make_unique<EncoderHandle>();
  if (!parse_puncturing(puncturing, &handle->pattern)) {
    set_error("invalid puncturing pattern");
    return nullptr;
  }
  if (!ldpc::Encoder::from_h(h, &handle->enc, &err)) {
    set_error(err);
    return nullptr;
  }
  const size_t n = handle->enc.n();
  handle->out_len = n;
  if (!handle->pattern.empty()) {
    size_t trues = 0;
    for (uint8_t p : handle->pattern) trues += p;
    // puncturing.rs:54-56: the codeword length must be divisible by the pattern length
    handle->out_len = (n % handle->pattern.size() == 0) ? n / handle->pattern.size() * trues : SIZE_MAX;
  }
  handle->scratch.resize(n);
  return handle.release();
}

bool make_device_encoder(EncoderHandle *h, int device) {
  if (device < 0) {
    set_error("LDPC_TOOLBOX_DEVICE is not a decimal GPU index");
    return false;
  }
  std::string err;
  h->dev.reset(ldpc::DeviceEncoder::create(h->enc, h->pattern, device, &err));
  if (!h->dev) set_error(err);
  return h->dev != nullptr;
}

int32_t encode_batch(void *encoder, uint8_t *output, size_t output_len, const uint8_t *input, size_t input_len,
                     size_t batch, bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<EncoderHandle *>(encoder);
  if (!h) {
    set_error("null encoder handle");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  // (a pattern that does not divide n has out_len == SIZE_MAX: no length matches it, as in the scalar call)
  if (input_len != h->enc.k() || output_len != h->out_len || h->out_len == SIZE_MAX) {
    set_error("message or output length does not match the code");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (batch == 0) return 0;
  if ((!input && input_len) || (!output && output_len)) {
    set_error("null message or output buffer");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (!h->dev && !make_device_encoder(h, default_device())) return LDPC_TOOLBOX_ERR_DEVICE;
  const int rc = on_device ? h->dev->encode_device(input, output, batch, static_cast<hipStream_t>(stream))
                           : h->dev->encode_host(input, output, batch);
  if (rc == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

void *make_demod(const ldpc::Constellation &c, int32_t device) {
  auto h = std::make_unique<DemodHandle>();
  h->c = c;
  h->device = device < 0 ? default_device() : device;
  return h.release();
}

int32_t demod_run(void *demod, void *llrs, size_t llrs_len, const void *symbols, size_t symbols_len, size_t batch, bool f64,
                  double sigma, int32_t interleaving, int32_t max_log, bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<DemodHandle *>(demod);
  if (!h) {
    set_error("null demodulator handle");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (const char *why = ldpc::demod_argument_error(h->c, llrs_len, symbols_len, sigma, interleaving)) {
    set_error(why);
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (batch == 0 || llrs_len == 0) return 0;
  if (!symbols || !llrs) {
    set_error("null symbol or LLR buffer");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (!h->dev) {
    if (h->device < 0) {
      set_error("LDPC_TOOLBOX_DEVICE is not a decimal GPU index");
      return LDPC_TOOLBOX_ERR_DEVICE;
    }
    std::string err;
    h->dev.reset(ldpc::DeviceDemodulator::create(h->c, h->device, &err));
    if (!h->dev) {
      set_error(err);
      return LDPC_TOOLBOX_ERR_DEVICE;
    }
  }
  const int rc = on_device ? h->dev->run_device(symbols, llrs, f64, symbols_len, llrs_len, batch, sigma, interleaving,
                                                max_log != 0, static_cast<hipStream_t>(stream))
                           : h->dev->run_host(symbols, llrs, f64, symbols_len, llrs_len, batch, sigma, interleaving, max_log != 0);
  if (rc == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

// the handle's device state, made at the first call that needs it: 0 or LDPC_TOOLBOX_ERR_DEVICE
int32_t demod_device_state(DemodHandle *h) {
  if (h->dev) return 0;
  if (h->device < 0) {
    set_error("LDPC_TOOLBOX_DEVICE is not a decimal GPU index");
    return LDPC_TOOLBOX_ERR_DEVICE;
  }
  std::string err;
  h->dev.reset(ldpc::DeviceDemodulator::create(h->c, h->device, &err));
  if (!h->dev) {
    set_error(err);
    return LDPC_TOOLBOX_ERR_DEVICE;
  }
  return 0;
}

int32_t mod_run(void *demod, void *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len, size_t batch, bool f64,
                int32_t interleaving, bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<DemodHandle *>(demod);
  if (!h) {
    set_error("null demodulator handle");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (const char *why = ldpc::mod_argument_error(h->c, bits_len, symbols_len, interleaving)) {
    set_error(why);
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (batch == 0 || bits_len == 0) return 0;
  if (!symbols || !bits) {
    set_error("null bit or symbol buffer");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (int32_t rc = demod_device_state(h)) return rc;
  const int rc = on_device ? h->dev->mod_device(bits, symbols, f64, bits_len, symbols_len, batch, interleaving,
                                                static_cast<hipStream_t>(stream))
                           : h->dev->mod_host(bits, symbols, f64, bits_len, symbols_len, batch, interleaving);
  if (rc == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

int32_t awgn_run(void *demod, void *symbols, size_t symbols_len, size_t batch, bool f64, double sigma, uint64_t seed,
                 uint64_t first_frame, bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<DemodHandle *>(demod);
  if (!h) {
    set_error("null demodulator handle");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (const char *why = ldpc::awgn_argument_error(symbols_len, sigma)) {
    set_error(why);
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (batch == 0 || symbols_len == 0) return 0;
  if (!symbols) {
    set_error("null symbol buffer");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (int32_t rc = demod_device_state(h)) return rc;
  const int rc = on_device ? h->dev->awgn_device(symbols, f64, symbols_len, batch, sigma, seed, first_frame,
                                                 static_cast<hipStream_t>(stream))
                           : h->dev->awgn_host(symbols, f64, symbols_len, batch, sigma, seed, first_frame);
  if (rc == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

int32_t fading_run(void *demod, void *symbols, void *scale, size_t symbols_len, size_t batch, bool f64, double sigma, uint32_t block,
                   uint64_t seed, uint64_t first_frame, bool on_device, void *stream) {
  g_last_error.clear();
  auto refuse = [](const char *why) {
    set_error(why);
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  };
  auto *h = static_cast<DemodHandle *>(demod);
  if (!h) return refuse("null demodulator handle");
  if (const char *why = ldpc::fading_argument_error(h->c, symbols_len, sigma, block)) return refuse(why);
  if (batch == 0 || symbols_len == 0) return 0;
  if (!symbols || !scale) return refuse("null symbol or scale buffer");
  if (on_device)
    if (const char *why = ldpc::fading_pointer_error(symbols, scale, f64)) return refuse(why);
  if (int32_t rc = demod_device_state(h)) return rc;
  const int rc = on_device ? h->dev->fading_device(symbols, scale, f64, symbols_len, batch, sigma, block, seed, first_frame,
                                                   static_cast<hipStream_t>(stream))
                           : h->dev->fading_host(symbols, scale, f64, symbols_len, batch, sigma, block, seed, first_frame);
  if (rc == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

// 0 with the handle's device state made, or LDPC_TOOLBOX_ERR_DEVICE
int32_t nr_qam_device_state(NrQamHandle *h) {
  if (h->dev) return 0;
  if (h->device < 0) {
    set_error("LDPC_TOOLBOX_DEVICE is not a decimal GPU index");
    return LDPC_TOOLBOX_ERR_DEVICE;
  }
  std::string err;
  h->dev.reset(ldpc::DeviceNrQam::create(h->c, h->device, &err));
  if (!h->dev) {
    set_error(err);
    return LDPC_TOOLBOX_ERR_DEVICE;
  }
  return 0;
}

int32_t nr_qam_refuse(const char *why) {
  set_error(why);
  return LDPC_TOOLBOX_ERR_ARGUMENT;
}

int32_t nr_qam_mod(void *qam, void *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len, size_t batch, bool f64,
                   int64_t c_init, bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<NrQamHandle *>(qam);
  if (!h) return nr_qam_refuse("null NR modulation handle");
  if (const char *why = ldpc::nrqam::mod_argument_error(h->c, bits_len, symbols_len, c_init)) return nr_qam_refuse(why);
  if (batch == 0 || bits_len == 0) return 0;
  if (!symbols || !bits) return nr_qam_refuse("null bit or symbol buffer");
  if (on_device)
    if (const char *why = ldpc::nrqam::device_pointer_error(symbols, nullptr, f64)) return nr_qam_refuse(why);
  if (int32_t rc = nr_qam_device_state(h)) return rc;
  const int rc = on_device ? h->dev->mod_device(bits, symbols, f64, bits_len, symbols_len, batch, c_init, static_cast<hipStream_t>(stream))
                           : h->dev->mod_host(bits, symbols, f64, bits_len, symbols_len, batch, c_init);
  if (rc == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

int32_t nr_qam_demod(void *qam, void *llrs, size_t llrs_len, const void *symbols, size_t symbols_len, size_t batch, bool f64,
                     double sigma, int32_t max_log, int64_t c_init, bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<NrQamHandle *>(qam);
  if (!h) return nr_qam_refuse("null NR modulation handle");
  if (const char *why = ldpc::nrqam::demod_argument_error(h->c, llrs_len, symbols_len, sigma, c_init)) return nr_qam_refuse(why);
  if (batch == 0 || llrs_len == 0) return 0;
  if (!symbols || !llrs) return nr_qam_refuse("null symbol or LLR buffer");
  if (on_device)
    if (const char *why = ldpc::nrqam::device_pointer_error(symbols, llrs, f64)) return nr_qam_refuse(why);
  if (int32_t rc = nr_qam_device_state(h)) return rc;
  const int rc = on_device ? h->dev->demod_device(symbols, llrs, f64, symbols_len, llrs_len, batch, sigma, max_log != 0, c_init,
                                                  static_cast<hipStream_t>(stream))
                           : h->dev->demod_host(symbols, llrs, f64, symbols_len, llrs_len, batch, sigma, max_log != 0, c_init);
  if (rc == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

int32_t nr_demap_i8(void *qam, int8_t *llrs, size_t llrs_len, const float *symbols, size_t symbols_len, size_t batch, double sigma,
                    int32_t max_log, int64_t c_init, bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<NrQamHandle *>(qam);
  if (!h) return nr_qam_refuse("null NR modulation handle");
  if (const char *why = ldpc::nrqam::demod_argument_error(h->c, llrs_len, symbols_len, sigma, c_init)) return nr_qam_refuse(why);
  if (batch == 0 || llrs_len == 0) return 0;
  if (!symbols || !llrs) return nr_qam_refuse("null symbol or LLR buffer");
  if (on_device)  // (the soft bits leave in pieces chosen from their address: no alignment asked of `llrs`)
    if (const char *why = ldpc::nrqam::device_pointer_error(symbols, nullptr, false)) return nr_qam_refuse(why);
  if (int32_t rc = nr_qam_device_state(h)) return rc;
  const int rc = on_device ? h->dev->demap_i8_device(symbols, llrs, symbols_len, llrs_len, batch, sigma, max_log != 0, c_init,
                                                     static_cast<hipStream_t>(stream))
                           : h->dev->demap_i8_host(symbols, llrs, symbols_len, llrs_len, batch, sigma, max_log != 0, c_init);
  if (rc == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

// the demappers with a scale per symbol (PART 10); out_elem: the bytes of one LLR -- 8 (double symbols), 4, or 1 (the 8-bit form)
int32_t nr_demap_csi(void *qam, void *llrs, size_t llrs_len, const void *symbols, const void *scale, size_t symbols_len, size_t batch,
                     size_t out_elem, int32_t max_log, int64_t c_init, bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<NrQamHandle *>(qam);
  if (!h) return nr_qam_refuse("null NR modulation handle");
  if (const char *why = ldpc::nrqam::demap_csi_argument_error(h->c, llrs_len, symbols_len, c_init)) return nr_qam_refuse(why);
  if (batch == 0 || llrs_len == 0) return 0;
  if (!symbols || !llrs) return nr_qam_refuse("null symbol or LLR buffer");
  if (!scale) return nr_qam_refuse("null scale buffer");
  const bool f64 = out_elem == 8;
  if (on_device) {  // (the soft bits of the 8-bit form leave in pieces chosen from their address)
    if (const char *why = ldpc::nrqam::device_pointer_error(symbols, out_elem == 1 ? nullptr : llrs, f64)) return nr_qam_refuse(why);
    if (const char *why = ldpc::nrqam::scale_pointer_error(scale, f64)) return nr_qam_refuse(why);
  }
  if (int32_t rc = nr_qam_device_state(h)) return rc;
  auto *st = static_cast<hipStream_t>(stream);
  int rc;
  if (!on_device)
    rc = h->dev->demap_csi_host(symbols, scale, llrs, out_elem, symbols_len, llrs_len, batch, max_log != 0, c_init);
  else if (out_elem == 1)
    rc = h->dev->demap_csi_i8_device(static_cast<const float *>(symbols), static_cast<const float *>(scale), static_cast<int8_t *>(llrs),
                                     symbols_len, llrs_len, batch, max_log != 0, c_init, st);
  else
    rc = h->dev->demap_csi_device(symbols, scale, llrs, f64, symbols_len, llrs_len, batch, max_log != 0, c_init, st);
  if (rc == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

int32_t bch_run(void *bch, bool decode, uint8_t *output, size_t output_len, const uint8_t *input, size_t input_len, size_t batch,
                int32_t *errors, bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<BchHandle *>(bch);
  if (!h) {
    set_error("null BCH handle");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (const char *why = ldpc::bch::bch_argument_error(h->code, decode, output_len, input_len)) {
    set_error(why);
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (batch == 0) return 0;
  if (!input || !output) {
    set_error("null input or output buffer");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (!h->dev) {
    if (h->device < 0) {
      set_error("LDPC_TOOLBOX_DEVICE is not a decimal GPU index");
      return LDPC_TOOLBOX_ERR_DEVICE;
    }
    std::string err;
    h->dev.reset(ldpc::DeviceBch::create(h->code, h->device, &err));
    if (!h->dev) {
      set_error(err);
      return LDPC_TOOLBOX_ERR_DEVICE;
    }
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc;
  if (decode)
    rc = on_device ? h->dev->decode_device(input, output, output_len, batch, errors, s)
                   : h->dev->decode_host(input, output, output_len, batch, errors);
  else
    rc = on_device ? h->dev->encode_device(input, output, batch, s) : h->dev->encode_host(input, output, batch);
  if (rc == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

// "nr5g:BG:ZC[:F[:NCB]]": decimal fields, nothing else
bool parse_nr_rm_spec(const char *spec, ldpc::nrrm::Config *c, std::string *err) {
  std::vector<std::string> parts;
  for (std::string rest = spec;;) {
    const size_t at = rest.find(':');
    parts.push_back(rest.substr(0, at));
    if (at == std::string::npos) break;
    rest = rest.substr(at + 1);
  }
  int64_t v[4] = {0, 0, 0, -1};
  bool ok = parts.size() >= 3 && parts.size() <= 5 && parts[0] == "nr5g";
  for (size_t i = 1; ok && i < parts.size(); i++) {
    const std::string &t = parts[i];
    ok = !t.empty() && t.size() <= 9 && t.find_first_not_of("0123456789") == std::string::npos;
    if (ok) v[i - 1] = std::strtoll(t.c_str(), nullptr, 10);
  }
  if (!ok) {
    *err = "invalid rate matcher spec (expected nr5g:BG:ZC[:F[:NCB]])";
    return false;
  }
  if (ldpc::codes::nr5g_set_index(static_cast<unsigned>(v[1])) < 0) {
    *err = "lifting size is none of the 51 of TS 38.212 Table 5.3.2-1";
    return false;
  }
  if (const char *why = ldpc::nrrm::make_config(v[0], v[1], v[2], v[3], c)) {
    *err = why;
    return false;
  }
  return true;
}

// 0 with the handle's device state made, or LDPC_TOOLBOX_ERR_DEVICE
int32_t nr_rm_device_state(NrRmHandle *h) {
  if (h->dev) return 0;
  if (h->device < 0) {
    set_error("LDPC_TOOLBOX_DEVICE is not a decimal GPU index");
    return LDPC_TOOLBOX_ERR_DEVICE;
  }
  std::string err;
  h->dev.reset(ldpc::DeviceNrRm::create(h->c, h->device, &err));
  if (!h->dev) {
    set_error(err);
    return LDPC_TOOLBOX_ERR_DEVICE;
  }
  return 0;
}

int32_t nr_rm_match(void *rm, uint8_t *output, size_t e, const uint8_t *codewords, size_t n, size_t batch, uint32_t rv, uint32_t qm,
                    bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<NrRmHandle *>(rm);
  if (!h) {
    set_error("null rate matcher handle");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (const char *why = ldpc::nrrm::match_argument_error(h->c, n, e, rv, qm)) {
    set_error(why);
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (batch == 0) return 0;
  if (!codewords || !output) {
    set_error("null input or output buffer");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (int32_t rc = nr_rm_device_state(h)) return rc;
  const uint32_t e32 = static_cast<uint32_t>(e);
  const int rc = on_device ? h->dev->match_device(codewords, output, batch, e32, rv, qm, static_cast<hipStream_t>(stream))
                           : h->dev->match_host(codewords, output, batch, e32, rv, qm);
  if (rc == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

int32_t nr_rm_recover(void *rm, void *llrs, size_t n, const void *rx, size_t e, size_t batch, uint32_t rv, uint32_t qm, bool f64,
                      double filler_llr, int32_t combine, bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<NrRmHandle *>(rm);
  if (!h) {
    set_error("null rate matcher handle");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (const char *why = ldpc::nrrm::recover_argument_error(h->c, n, e, rv, qm, filler_llr)) {
    set_error(why);
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (batch == 0) return 0;
  if (!rx || !llrs) {
    set_error("null input or output buffer");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (int32_t rc = nr_rm_device_state(h)) return rc;
  const uint32_t e32 = static_cast<uint32_t>(e);
  const int rc = on_device ? h->dev->recover_device(rx, llrs, f64, batch, e32, rv, qm, filler_llr, combine != 0, static_cast<hipStream_t>(stream))
                           : h->dev->recover_host(rx, llrs, f64, batch, e32, rv, qm, filler_llr, combine != 0);
  if (rc == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

int32_t nr_rm_recover_i8(void *rm, int8_t *llrs, size_t n, const int8_t *rx, size_t e, size_t batch, uint32_t rv, uint32_t qm,
                         int32_t filler, int32_t combine, bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<NrRmHandle *>(rm);
  if (!h) {
    set_error("null rate matcher handle");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  const char *why = ldpc::nrrm::match_argument_error(h->c, n, e, rv, qm);
  if (!why && (filler < 1 || filler > ldpc::soft::kSoftMax)) why = "filler soft bit must be 1 .. 127";
  if (why) {
    set_error(why);
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (batch == 0) return 0;
  if (!rx || !llrs) {
    set_error("null input or output buffer");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (int32_t rc = nr_rm_device_state(h)) return rc;
  const uint32_t e32 = static_cast<uint32_t>(e);
  const int rc = on_device ? h->dev->recover_i8_device(rx, llrs, batch, e32, rv, qm, filler, combine != 0, static_cast<hipStream_t>(stream))
                           : h->dev->recover_i8_host(rx, llrs, batch, e32, rv, qm, filler, combine != 0);
  if (rc == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

// "nr5g-tb:BG:A": decimal fields, nothing else
bool parse_nr_tb_spec(const char *spec, ldpc::nrtb::Config *c, std::string *err) {
  const std::string text = spec;
  const std::string digits = "0123456789";
  const size_t first = text.find(':'), second = first == std::string::npos ? first : text.find(':', first + 1);
  bool ok = second != std::string::npos && text.compare(0, first, "nr5g-tb") == 0;
  int64_t v[2] = {0, 0};
  if (ok) {
    const std::string t[2] = {text.substr(first + 1, second - first - 1), text.substr(second + 1)};
    for (int i = 0; ok && i < 2; i++) {
      ok = !t[i].empty() && t[i].size() <= 9 && t[i].find_first_not_of(digits) == std::string::npos;
      if (ok) v[i] = std::strtoll(t[i].c_str(), nullptr, 10);
    }
  }
  if (!ok) {
    *err = "invalid transport block spec (expected nr5g-tb:BG:A)";
    return false;
  }
  if (const char *why = ldpc::nrtb::make_config(v[0], v[1], c)) {
    *err = why;
    return false;
  }
  return true;
}

// 0 with the handle's device state made, or LDPC_TOOLBOX_ERR_DEVICE
int32_t nr_tb_device_state(NrTbHandle *h) {
  if (h->dev) return 0;
  if (h->device < 0) {
    set_error("LDPC_TOOLBOX_DEVICE is not a decimal GPU index");
    return LDPC_TOOLBOX_ERR_DEVICE;
  }
  std::string err;
  h->dev.reset(ldpc::DeviceNrTb::create(h->c, h->device, &err));
  if (!h->dev) {
    set_error(err);
    return LDPC_TOOLBOX_ERR_DEVICE;
  }
  return 0;
}

int32_t nr_tb_argument_error(const char *why) {
  set_error(why);
  return LDPC_TOOLBOX_ERR_ARGUMENT;
}

int32_t nr_tb_result(NrTbHandle *h, int rc) {
  if (rc == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

int32_t nr_tb_segment(void *tb, uint8_t *rows, size_t k, const uint8_t *payload, size_t a, size_t batch, bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<NrTbHandle *>(tb);
  if (!h) return nr_tb_argument_error("null transport block handle");
  if (const char *why = ldpc::nrtb::row_lengths_error(h->c, a, k)) return nr_tb_argument_error(why);
  if (batch == 0) return 0;
  if (!payload || !rows) return nr_tb_argument_error("null input or output buffer");
  if (int32_t rc = nr_tb_device_state(h)) return rc;
  return nr_tb_result(h, on_device ? h->dev->segment_device(payload, rows, batch, static_cast<hipStream_t>(stream))
                                   : h->dev->segment_host(payload, rows, batch));
}

int32_t nr_tb_desegment(void *tb, uint8_t *payload, size_t a, uint8_t *tb_ok, uint8_t *cb_ok, const uint8_t *rows, size_t k, size_t batch,
                        bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<NrTbHandle *>(tb);
  if (!h) return nr_tb_argument_error("null transport block handle");
  if (const char *why = ldpc::nrtb::row_lengths_error(h->c, a, k)) return nr_tb_argument_error(why);
  if (batch == 0) return 0;
  if (!payload || !rows || !tb_ok) return nr_tb_argument_error("null input or output buffer");
  if (int32_t rc = nr_tb_device_state(h)) return rc;
  return nr_tb_result(h, on_device ? h->dev->desegment_device(rows, payload, tb_ok, cb_ok, batch, static_cast<hipStream_t>(stream))
                                   : h->dev->desegment_host(rows, payload, tb_ok, cb_ok, batch));
}

// concatenate (bytes, packed -> [batch][G]) and split (floats or doubles, [batch][G] -> packed)
int32_t nr_tb_repack(void *tb, void *output, const void *input, size_t g, size_t q, size_t batch, bool split, bool f64, bool on_device,
                     void *stream) {
  g_last_error.clear();
  auto *h = static_cast<NrTbHandle *>(tb);
  if (!h) return nr_tb_argument_error("null transport block handle");
  ldpc::nrtb::Lengths l;
  if (const char *why = ldpc::nrtb::make_lengths(h->c, g, q, &l)) return nr_tb_argument_error(why);
  if (batch == 0) return 0;
  if (!input || !output) return nr_tb_argument_error("null input or output buffer");
  if (int32_t rc = nr_tb_device_state(h)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc;
  if (split)
    rc = on_device ? h->dev->split_device(input, output, f64, l, batch, s) : h->dev->split_host(input, output, f64, l, batch);
  else
    rc = on_device ? h->dev->concatenate_device(static_cast<const uint8_t *>(input), static_cast<uint8_t *>(output), l, batch, s)
                   : h->dev->concatenate_host(static_cast<const uint8_t *>(input), static_cast<uint8_t *>(output), l, batch);
  return nr_tb_result(h, rc);
}

int32_t nr_link_refuse(const char *why) {
  set_error(why);
  return LDPC_TOOLBOX_ERR_ARGUMENT;
}

// 0 with the handle's device state made, or LDPC_TOOLBOX_ERR_DEVICE
int32_t nr_link_device_state(NrLinkHandle *h) {
  if (!h->dev) {
    if (h->device < 0) {
      set_error("LDPC_TOOLBOX_DEVICE is not a decimal GPU index");
      return LDPC_TOOLBOX_ERR_DEVICE;
    }
    std::string err;
    h->dev.reset(ldpc::DeviceNrLink::create(h->c, h->impl, h->slots, h->soft_bits, h->device, &err));
    if (!h->dev) {
      set_error(err);
      return LDPC_TOOLBOX_ERR_DEVICE;
    }
  }
  h->dev->set_max_log(h->max_log);
  h->dev->set_pass_elements(h->pass_elements);
  h->dev->set_filler_llr(static_cast<float>(h->filler_llr));
  if (h->soft_bits == 8) h->dev->set_filler_soft_bit(ldpc::nrlink::filler_soft_bit(h->filler_llr));
  return 0;
}

// the entries that take or give soft rows of one mode, called on a handle of the other
int32_t nr_link_wrong_mode(const NrLinkHandle *h) {
  set_error(h->soft_bits == 8 ? "the handle's soft rows are 8-bit soft bits (soft_bits 8): use the _i8 entry"
                              : "the handle's soft rows are floats (soft_bits 32): use the float entry");
  return LDPC_TOOLBOX_ERR_UNSUPPORTED;
}

int32_t nr_link_result(NrLinkHandle *h, int rc) {
  if (rc == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

int32_t nr_link_transmit(void *link, float *symbols, size_t symbols_len, const uint8_t *payload, size_t a, size_t batch, uint32_t rv,
                         int64_t c_init, bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<NrLinkHandle *>(link);
  if (!h) return nr_link_refuse("null link handle");
  if (const char *why = ldpc::nrlink::transmit_argument_error(h->c, symbols_len, a, rv, c_init)) return nr_link_refuse(why);
  if (batch == 0) return 0;
  if (!payload || !symbols) return nr_link_refuse("null payload or symbol buffer");
  if (on_device)
    if (const char *why = ldpc::nrqam::device_pointer_error(symbols, nullptr, false)) return nr_link_refuse(why);
  if (int32_t rc = nr_link_device_state(h)) return rc;
  return nr_link_result(h, on_device ? h->dev->transmit_device(payload, symbols, batch, rv, c_init, static_cast<hipStream_t>(stream))
                                     : h->dev->transmit_host(payload, symbols, batch, rv, c_init));
}

// what every call into the slots checks: the range, and with `combine` that each slot of it holds a reception
const char *nr_link_slots_error(NrLinkHandle *h, uint32_t first_slot, size_t batch, int32_t combine) {
  if (const char *why = ldpc::nrlink::slots_error(first_slot, batch, h->slots)) return why;
  if (combine != 0 && batch > 0 && !(h->dev && h->dev->slots_used(first_slot, batch))) return "combine with a slot that has never been received into";
  return nullptr;
}

int32_t nr_link_receive(void *link, uint8_t *payload, size_t a, uint8_t *tb_ok, uint8_t *cb_ok, int32_t *iterations, const float *symbols,
                        const float *scale, size_t symbols_len, size_t batch, double noise_sigma, uint32_t rv, int64_t c_init,
                        uint32_t first_slot, int32_t combine, uint32_t max_iterations, bool on_device, void *stream) {
  g_last_error.clear();
  auto *h = static_cast<NrLinkHandle *>(link);
  if (!h) return nr_link_refuse("null link handle");
  if (const char *why = ldpc::nrlink::receive_argument_error(h->c, symbols_len, a, rv, c_init, scale != nullptr, noise_sigma, first_slot,
                                                             batch, h->slots))
    return nr_link_refuse(why);
  if (const char *why = nr_link_slots_error(h, first_slot, batch, combine)) return nr_link_refuse(why);
  if (batch == 0) return 0;
  if (!payload || !tb_ok || !symbols) return nr_link_refuse("null payload, tb_ok or symbol buffer");
  if (on_device) {
    if (const char *why = ldpc::nrqam::device_pointer_error(symbols, nullptr, false)) return nr_link_refuse(why);
    if (scale)
      if (const char *why = ldpc::nrqam::scale_pointer_error(scale, false)) return nr_link_refuse(why);
    if (reinterpret_cast<uintptr_t>(iterations) % sizeof(int32_t) != 0) return nr_link_refuse("the iterations buffer is not aligned to its element");
  }
  if (int32_t rc = nr_link_device_state(h)) return rc;
  return nr_link_result(h, on_device ? h->dev->receive_device(symbols, scale, payload, tb_ok, cb_ok, iterations, batch, noise_sigma, rv, c_init,
                                                              first_slot, combine != 0, max_iterations, static_cast<hipStream_t>(stream))
                                     : h->dev->receive_host(symbols, scale, payload, tb_ok, cb_ok, iterations, batch, noise_sigma, rv, c_init,
                                                            first_slot, combine != 0, max_iterations));
}

// rx: floats (soft_bits 32) or bytes (8), already known to be the handle's kind
int32_t nr_link_recover(NrLinkHandle *h, const void *rx, size_t elem, size_t g, size_t batch, uint32_t rv, uint32_t first_slot, int32_t combine,
                        void *stream) {
  if (g != h->c.len.g) return nr_link_refuse("row length is not the handle's G");
  if (rv > 3) return nr_link_refuse("rv must be 0 .. 3");
  if (const char *why = nr_link_slots_error(h, first_slot, batch, combine)) return nr_link_refuse(why);
  if (batch == 0) return 0;
  if (!rx) return nr_link_refuse("null LLR buffer");
  if (reinterpret_cast<uintptr_t>(rx) % elem != 0) return nr_link_refuse("the LLR buffer is not aligned to its element");
  if (int32_t rc = nr_link_device_state(h)) return rc;
  return nr_link_result(h, h->dev->recover_device(rx, batch, rv, first_slot, combine != 0, static_cast<hipStream_t>(stream)));
}

int32_t nr_link_slot_state(NrLinkHandle *h, void *soft, uint8_t *done, uint8_t *rows, uint32_t first_slot, size_t batch) {
  if (const char *why = ldpc::nrlink::slots_error(first_slot, batch, h->slots)) return nr_link_refuse(why);
  if (batch == 0 || (!soft && !done && !rows)) return 0;
  if (int32_t rc = nr_link_device_state(h)) return rc;
  return nr_link_result(h, h->dev->slot_state_host(soft, done, rows, first_slot, batch));
}

template <typename F>
int32_t decode_scalar(void *decoder, uint8_t *output, size_t output_len, const F *llrs, size_t llrs_len,
                      uint32_t max_iterations) {
  g_last_error.clear();
  auto *h = static_cast<DecoderHandle *>(decoder);
  // -1 is the reference's "no codeword found" (output filled).  A call that could not run at all
  // (where the reference would panic) returns a value BELOW -1 and leaves `output` untouched, so a
  // caller counting -1 as a decoding failure never counts a GPU fault as one.
  if (!h || !h->dec) {
    set_error("null decoder handle");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (llrs_len != h->dec->input_len() || output_len > h->dec->n()) {
    set_error("LLR or output length does not match the code");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  int32_t iterations = -1;
  const int rc = h->dec->decode_host(llrs, sizeof(F) == 8 ? ldpc::LlrType::F64 : ldpc::LlrType::F32, 1, max_iterations, output, output_len, &iterations,
                                     nullptr);
  if (rc != 0) {
    set_error(h->dec->last_error());
    return rc == -3 ? LDPC_TOOLBOX_ERR_UNSUPPORTED : LDPC_TOOLBOX_ERR_DEVICE;
  }
  return iterations;
}

// F: float, double, or int8_t soft bits (PART 9: the 8-bit implementations only; P = int16_t); P: the posterior's type
template <typename F, typename P>
int32_t decode_batch(void *decoder, uint8_t *output, size_t output_len, const F *llrs, size_t llrs_len,
                     size_t batch, uint32_t max_iterations, int32_t *iterations, P *posterior, bool on_device,
                     void *stream) {
  constexpr ldpc::LlrType kType = sizeof(F) == 8 ? ldpc::LlrType::F64 : (sizeof(F) == 4 ? ldpc::LlrType::F32 : ldpc::LlrType::I8);
  g_last_error.clear();
  auto *h = static_cast<DecoderHandle *>(decoder);
  // one error vocabulary for the scalar and the batch entries (include/ldpc_toolbox.h, LDPC_TOOLBOX_ERR_*)
  if (!h || !h->dec) {
    set_error("null decoder handle");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (llrs_len != h->dec->input_len() || output_len > h->dec->n()) {
    set_error("LLR or output length does not match the code");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (kType == ldpc::LlrType::I8 && !h->dec->implementation().i8) {
    set_error("8-bit soft-bit input needs a decoder with one of the 8-bit implementations");
    return LDPC_TOOLBOX_ERR_UNSUPPORTED;
  }
  const int rc = on_device ? h->dec->decode_device(llrs, kType, batch, max_iterations, output, output_len,
                                                   iterations, posterior, static_cast<hipStream_t>(stream))
                           : h->dec->decode_host(llrs, kType, batch, max_iterations, output, output_len,
                                                 iterations, posterior);
  if (rc == 0) return 0;
  set_error(h->dec->last_error());
  return rc == -3 ? LDPC_TOOLBOX_ERR_UNSUPPORTED : (rc == -1 ? LDPC_TOOLBOX_ERR_ARGUMENT : LDPC_TOOLBOX_ERR_DEVICE);
}

}  // namespace

extern "C" {

// ---- PART 1 ---------------------------------------------------------------------------------

void *ldpc_toolbox_decoder_ctor(const char *alist_file_path, const char *implementation,
                                const char *puncturing) {
  std::string text;
  if (!alist_file_path || !read_file(alist_file_path, &text)) {
    set_error("cannot read alist file");
    return nullptr;
  }
  return make_decoder(text, implementation, puncturing, default_device());
}

void *ldpc_toolbox_decoder_ctor_alist_string(const char *alist, const char *implementation,
                                             const char *puncturing) {
  if (!alist) {
    set_error("null alist");
    return nullptr;
  }
  return make_decoder(alist, implementation, puncturing, default_device());
}

void ldpc_toolbox_decoder_dtor(void *decoder) { delete static_cast<DecoderHandle *>(decoder); }

int32_t ldpc_toolbox_decoder_decode_f64(void *decoder, uint8_t *output, size_t output_len, const double *llrs,
                                        size_t llrs_len, uint32_t max_iterations) {
  return decode_scalar<double>(decoder, output, output_len, llrs, llrs_len, max_iterations);
}

int32_t ldpc_toolbox_decoder_decode_f32(void *decoder, uint8_t *output, size_t output_len, const float *llrs,
                                        size_t llrs_len, uint32_t max_iterations) {
  return decode_scalar<float>(decoder, output, output_len, llrs, llrs_len, max_iterations);
}

void *ldpc_toolbox_encoder_ctor(const char *alist_file_path, const char *puncturing) {
  std::string text;
  if (!alist_file_path || !read_file(alist_file_path, &text)) {
    set_error("cannot read alist file");
    return nullptr;
  }
  return make_encoder(text, puncturing);
}

void *ldpc_toolbox_encoder_ctor_alist_string(const char *alist, const char *puncturing) {
  if (!alist) {
    set_error("null alist");
    return nullptr;
  }
  return make_encoder(alist, puncturing);
}

void ldpc_toolbox_encoder_dtor(void *encoder) { delete static_cast<EncoderHandle *>(encoder); }

void ldpc_toolbox_encoder_encode(void *encoder, uint8_t *output, size_t output_len, const uint8_t *input,
                                 size_t input_len) {
  g_last_error.clear();
  auto *h = static_cast<EncoderHandle *>(encoder);
  if (!h) {
    set_error("null encoder handle");
    return;
  }
  // the reference panics on these (ndarray shape mismatch / assert_eq!, c_api/encoder.rs:50):
  // here nothing is written and the error is recorded
  if (input_len != h->enc.k() || output_len != h->out_len) {
    set_error("message or output length does not match the code");
    std::fprintf(stderr, "ldpc_toolbox: encoder: %s\n", g_last_error.c_str());
    return;
  }
  // c_api/encoder.rs:41-43: a byte equal to 1 is a one, anything else a zero
  std::vector<uint8_t> msg(input_len);
  for (size_t i = 0; i < input_len; i++) msg[i] = input[i] == 1;
  if (h->pattern.empty()) {
    h->enc.encode(msg.data(), output);
    return;
  }
  h->enc.encode(msg.data(), h->scratch.data());
  // puncturing.rs:47-75: keep the blocks whose pattern entry is true
  const size_t block = h->enc.n() / h->pattern.size();
  size_t j = 0;
  for (size_t k = 0; k < h->pattern.size(); k++) {
    if (!h->pattern[k]) continue;
    std::memcpy(output + j * block, h->scratch.data() + k * block, block);
    j++;
  }
}

// ---- PART 2 ---------------------------------------------------------------------------------

void *ldpc_toolbox_decoder_ctor_alist_string_on_device(const char *alist, const char *implementation,
                                                       const char *puncturing, int32_t device) {
  if (!alist) {
    set_error("null alist");
    return nullptr;
  }
  return make_decoder(alist, implementation, puncturing, device);
}

void *ldpc_toolbox_encoder_ctor_alist_string_on_device(const char *alist, const char *puncturing, int32_t device) {
  if (!alist) {
    set_error("null alist");
    return nullptr;
  }
  std::unique_ptr<EncoderHandle> h(static_cast<EncoderHandle *>(make_encoder(alist, puncturing)));
  if (!h) return nullptr;
  if (h->out_len == SIZE_MAX) {
    set_error("the puncturing pattern does not divide the codeword length");
    return nullptr;
  }
  if (device < 0) {
    set_error("HIP device index out of range");
    return nullptr;
  }
  if (!make_device_encoder(h.get(), device)) return nullptr;
  return h.release();
}

int32_t ldpc_toolbox_encoder_encode_batch(void *encoder, uint8_t *output, size_t output_len, const uint8_t *input,
                                          size_t input_len, size_t batch) {
  return encode_batch(encoder, output, output_len, input, input_len, batch, false, nullptr);
}

int32_t ldpc_toolbox_encoder_encode_batch_device(void *encoder, uint8_t *output, size_t output_len, const uint8_t *input,
                                                 size_t input_len, size_t batch, void *hip_stream) {
  return encode_batch(encoder, output, output_len, input, input_len, batch, true, hip_stream);
}

int32_t ldpc_toolbox_encoder_get(void *encoder, const char *key, int64_t *value) {
  auto *h = static_cast<EncoderHandle *>(encoder);
  if (!h || !key || !value) return -1;
  const std::string k = key;
  if (k == "k")
    *value = static_cast<int64_t>(h->enc.k());
  else if (k == "n")
    *value = static_cast<int64_t>(h->enc.n());
  else if (k == "output_len")  // (-1: the pattern does not divide n, no call can succeed)
    *value = h->out_len == SIZE_MAX ? -1 : static_cast<int64_t>(h->out_len);
  else if (k == "staircase")
    *value = h->enc.staircase() ? 1 : 0;
  else if (k == "staircase_form")  // (which of launch_staircase's three forms a batched call takes; -1: not a staircase code)
    *value = h->enc.staircase() ? ldpc::staircase_form(h->enc.k()) : -1;
  else if (k == "device")
    *value = h->dev ? h->dev->device() : -1;
  else
    return -1;
  return 0;
}

int32_t ldpc_toolbox_decoder_decode_batch_f32(void *decoder, uint8_t *output, size_t output_len,
                                              const float *llrs, size_t llrs_len, size_t batch,
                                              uint32_t max_iterations, int32_t *iterations, float *posterior) {
  return decode_batch<float>(decoder, output, output_len, llrs, llrs_len, batch, max_iterations, iterations,
                             posterior, false, nullptr);
}

int32_t ldpc_toolbox_decoder_decode_batch_f64(void *decoder, uint8_t *output, size_t output_len,
                                              const double *llrs, size_t llrs_len, size_t batch,
                                              uint32_t max_iterations, int32_t *iterations, double *posterior) {
  return decode_batch<double>(decoder, output, output_len, llrs, llrs_len, batch, max_iterations, iterations,
                              posterior, false, nullptr);
}

int32_t ldpc_toolbox_decoder_decode_batch_f32_device(void *decoder, uint8_t *output, size_t output_len,
                                                     const float *llrs, size_t llrs_len, size_t batch,
                                                     uint32_t max_iterations, int32_t *iterations,
                                                     float *posterior, void *hip_stream) {
  return decode_batch<float>(decoder, output, output_len, llrs, llrs_len, batch, max_iterations, iterations,
                             posterior, true, hip_stream);
}

int32_t ldpc_toolbox_decoder_decode_batch_f64_device(void *decoder, uint8_t *output, size_t output_len,
                                                     const double *llrs, size_t llrs_len, size_t batch,
                                                     uint32_t max_iterations, int32_t *iterations,
                                                     double *posterior, void *hip_stream) {
  return decode_batch<double>(decoder, output, output_len, llrs, llrs_len, batch, max_iterations, iterations,
                              posterior, true, hip_stream);
}

int32_t ldpc_toolbox_decoder_syndrome(void *decoder, const uint8_t *bits, size_t bits_len, size_t batch,
                                      uint8_t *syndrome, uint32_t *weight) {
  g_last_error.clear();
  auto *h = static_cast<DecoderHandle *>(decoder);
  if (!h || !h->dec) {
    set_error("null decoder handle");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (bits_len != h->dec->n() || (!bits && batch)) {
    set_error("hard decisions must cover the whole codeword (bits_len == n)");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  const int rc = h->dec->syndrome_host(bits, batch, syndrome, weight);
  if (rc == 0) return 0;
  set_error(h->dec->last_error());
  return rc == -1 ? LDPC_TOOLBOX_ERR_ARGUMENT : LDPC_TOOLBOX_ERR_DEVICE;
}

int32_t ldpc_toolbox_decoder_syndrome_device(void *decoder, const uint8_t *bits, size_t bits_len, size_t batch,
                                             uint8_t *syndrome, uint32_t *weight, void *hip_stream) {
  g_last_error.clear();
  auto *h = static_cast<DecoderHandle *>(decoder);
  if (!h || !h->dec) {
    set_error("null decoder handle");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  if (bits_len != h->dec->n() || (!bits && batch)) {
    set_error("hard decisions must cover the whole codeword (bits_len == n)");
    return LDPC_TOOLBOX_ERR_ARGUMENT;
  }
  const int rc = h->dec->syndrome_device(bits, batch, syndrome, weight, static_cast<hipStream_t>(hip_stream));
  if (rc == 0) return 0;
  set_error(h->dec->last_error());
  return rc == -1 ? LDPC_TOOLBOX_ERR_ARGUMENT : LDPC_TOOLBOX_ERR_DEVICE;
}

int32_t ldpc_toolbox_decoder_get(void *decoder, const char *key, int64_t *value) {
  auto *h = static_cast<DecoderHandle *>(decoder);
  if (!h || !h->dec || !key || !value) return -1;
  const std::string k = key;
  const ldpc::DeviceDecoder &d = *h->dec;
  if (k == "n")
    *value = static_cast<int64_t>(d.n());
  else if (k == "m")
    *value = static_cast<int64_t>(d.m());
  else if (k == "k")
    *value = static_cast<int64_t>(d.n()) - static_cast<int64_t>(d.m());
  else if (k == "edges")
    *value = static_cast<int64_t>(d.edges());
  else if (k == "input_len")
    *value = static_cast<int64_t>(d.input_len());
  else if (k == "device")
    *value = d.device();
  else if (k == "group_size")
    *value = static_cast<int64_t>(d.group_size());
  else if (k == "max_check_degree")
    *value = d.max_check_degree();
  else if (k == "max_variable_degree")
    *value = d.max_variable_degree();
  else if (k == "layers")
    *value = static_cast<int64_t>(d.layers());
  else if (k == "last_lanes")
    *value = d.last_lanes();
  else if (k == "last_pooled")
    *value = static_cast<int64_t>(d.last_pooled());
  else if (k == "last_group")
    *value = static_cast<int64_t>(d.last_group());
  else if (k == "preferred_group")
    *value = static_cast<int64_t>(d.preferred_group(size_t(1) << 20));
  else if (k == "row_records")
    *value = d.row_records();
  else if (k == "record_flag_bits")
    *value = d.record_flag_bits();
  else if (k == "last_vn_records")
    *value = d.last_vn_records();
  else if (k == "last_vn_bundles")
    *value = d.last_vn_bundles();
  else if (k == "vn_bundle_saved_permille")
    *value = d.vn_bundle_saved_permille();
  else if (k == "last_vn_chains")
    *value = d.last_vn_chains();
  else if (k == "vn_chain_saved_permille")
    *value = d.vn_chain_saved_permille();
  else if (k == "flags8")
    *value = d.flags8();
  else if (k == "cn_row_shape")
    *value = d.cn_row_shape();
  else if (k == "last_cn_row_shape")
    *value = d.last_cn_row_shape();
  else if (k == "cn_row_shape_runs")
    *value = d.cn_row_shape_runs();
  else if (k == "cn_row_shape_rows")
    *value = d.cn_row_shape_rows();
  else if (k == "last_record_flag_bytes")
    *value = d.last_record_flag_bytes();
  else if (k == "call_edges")
    *value = d.call_edges();
  else if (k == "last_call_edges")
    *value = d.last_call_edges();
  else if (k == "minsum_correction")
    *value = static_cast<int64_t>(d.implementation().correction);
  else if (k == "minsum_correction_int")  // the 8-bit min-sum names: a = 16 alpha or b = 8 beta, 0 for every other name
    *value = d.implementation().correction_int;
  else if (k == "last_persist" || k == "experiments")  // (the removed experiment builds: always 0)
    *value = 0;
  else
    return -1;
  return 0;
}

int32_t ldpc_toolbox_decoder_set(void *decoder, const char *key, int64_t value) {
  auto *h = static_cast<DecoderHandle *>(decoder);
  if (!h || !h->dec || !key) return -1;
  const std::string k = key;
  if (k == "group_size" && value >= 0)
    h->dec->set_group_size(static_cast<size_t>(value));
  else if (k == "profiling")
    h->dec->set_profiling(value != 0);
  else if (!h->dec->set_option(k, value))
    return -1;
  return 0;
}

int32_t ldpc_toolbox_decoder_kernel_stats(void *decoder, int32_t kind, uint64_t *launches, double *total_ms,
                                          int32_t reset) {
  auto *h = static_cast<DecoderHandle *>(decoder);
  if (!h || !h->dec || kind < 0 || kind >= ldpc::kKernelKinds) return -1;
  const ldpc::KernelStat s = h->dec->kernel_stat(kind);
  if (launches) *launches = s.launches;
  if (total_ms) *total_ms = s.total_ms;
  if (reset) h->dec->reset_kernel_stats();
  return 0;
}

// ---- PART 3: GPU-resident simulation step ----------------------------------------------------------

void *ldpc_toolbox_sim_ctor(const char *alist, const char *implementation, const char *puncturing, int32_t device,
                            uint32_t pool_size, uint64_t pool_seed) {
  g_last_error.clear();
  if (!alist || !implementation) {
    set_error("null argument");
    return nullptr;
  }
  std::string err;
  ldpc::Simulator *s = ldpc::Simulator::create(alist, implementation, puncturing ? puncturing : "", device,
                                               pool_size, pool_seed, &err);
  if (!s) set_error(err);
  return s;
}

void ldpc_toolbox_sim_dtor(void *sim) { delete static_cast<ldpc::Simulator *>(sim); }

int32_t ldpc_toolbox_sim_run(void *sim, double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames,
                             uint32_t max_iterations, uint64_t *counters) {
  g_last_error.clear();
  auto *s = static_cast<ldpc::Simulator *>(sim);
  if (!s || !counters) {
    set_error("null argument");
    return -1;
  }
  const int rc = s->run(ebn0_db, seed, first_frame, frames, max_iterations, counters);
  if (rc) set_error(s->last_error());
  return rc;
}

int32_t ldpc_toolbox_sim_run_bch(void *sim, double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames,
                                 uint32_t max_iterations, uint64_t bch_max_errors, uint64_t *counters) {
  g_last_error.clear();
  auto *s = static_cast<ldpc::Simulator *>(sim);
  if (!s || !counters) {
    set_error("null argument");
    return -1;
  }
  const int rc = s->run_bch(ebn0_db, seed, first_frame, frames, max_iterations, bch_max_errors, counters);
  if (rc) set_error(s->last_error());
  return rc;
}

int32_t ldpc_toolbox_sim_generate(void *sim, double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames,
                                  float *llrs, uint32_t *pool_index) {
  g_last_error.clear();
  auto *s = static_cast<ldpc::Simulator *>(sim);
  if (!s || !llrs) {
    set_error("null argument");
    return -1;
  }
  const int rc = s->generate(ebn0_db, seed, first_frame, frames, llrs, pool_index);
  if (rc) set_error(s->last_error());
  return rc;
}

int32_t ldpc_toolbox_sim_pool(void *sim, uint8_t *messages, uint8_t *tx_bits) {
  auto *s = static_cast<ldpc::Simulator *>(sim);
  if (!s) return -1;
  if (messages) std::memcpy(messages, s->messages().data(), s->messages().size());
  if (tx_bits) std::memcpy(tx_bits, s->tx_bits().data(), s->tx_bits().size());
  return 0;
}

int32_t ldpc_toolbox_sim_get(void *sim, const char *key, int64_t *value) {
  auto *s = static_cast<ldpc::Simulator *>(sim);
  if (!s || !key || !value) return -1;
  const std::string k = key;
  if (k == "k")
    *value = static_cast<int64_t>(s->k());
  else if (k == "n")
    *value = static_cast<int64_t>(s->n());
  else if (k == "n_tx")
    *value = static_cast<int64_t>(s->n_tx());
  else if (k == "pool")
    *value = s->pool();
  else if (k == "modulation")
    *value = s->modulation();
  else if (k == "interleaving")
    *value = s->interleaving();
  else if (k == "constellation")  // 1 while ldpc_toolbox_sim_set_constellation is in force
    *value = s->has_constellation() ? 1 : 0;
  else if (k == "nr_qam")  // 1 while ldpc_toolbox_sim_set_nr_qam is in force
    *value = s->has_nr_qam() ? 1 : 0;
  else if (k == "max_log")
    *value = s->max_log() ? 1 : 0;
  else if (k == "bch")  // 1 while ldpc_toolbox_sim_set_bch is in force
    *value = s->has_bch() ? 1 : 0;
  else if (k == "rate_match")  // 1 while ldpc_toolbox_sim_set_rate_match is in force
    *value = s->has_rate_match() ? 1 : 0;
  else if (k == "harq")  // transmissions of the sequence of ldpc_toolbox_sim_set_harq, 0 = none
    *value = s->harq().t;
  else if (k.size() == 7 && k.compare(0, 6, "harq_e") == 0 && k[6] >= '0' && k[6] <= '7')  // "harq_e0" .. "harq_e7": E_t, 0 beyond the sequence
    *value = uint32_t(k[6] - '0') < s->harq().t ? s->harq().e[k[6] - '0'] : 0;
  else if (k.size() == 8 && k.compare(0, 7, "harq_rv") == 0 && k[7] >= '0' && k[7] <= '7')  // "harq_rv0" .. "harq_rv7"
    *value = uint32_t(k[7] - '0') < s->harq().t ? s->harq().rv[k[7] - '0'] : 0;
  else if (k.size() == 15 && k.compare(0, 14, "harq_flushes_t") == 0 && k[14] >= '0' && k[14] <= '7')  // of the last run_harq call
    *value = static_cast<int64_t>(s->harq_flushes(k[14] - '0'));
  else if (k.size() == 12 && k.compare(0, 11, "harq_rows_t") == 0 && k[11] >= '0' && k[11] <= '7')  // rows its flushes of stage t decoded
    *value = static_cast<int64_t>(s->harq_flushed_rows(k[11] - '0'));
  else if (k == "streamed_frames" || k == "stream_iterations")  // (continuous batching: profiles/r03_continuous_batching.txt)
    *value = 0;
  else if (k == "fading_block")  // symbols per gain of the Rayleigh block-fading channel, 0 = none (PART 10)
    *value = s->fading_block();
  else if (k == "soft_bits")  // 32, or 8: run_harq keeps its soft buffers as 8-bit soft bits (PART 9)
    *value = s->soft_bits();
  else if (k == "pooled_frames")  // frames of the last run() call that went through the straggler pool
    *value = static_cast<int64_t>(s->pooled_frames());
  else if (k == "preferred_batch")  // frames per run() call that fill one group of the decoder (4096; more for small graphs)
    *value = static_cast<int64_t>(s->decoder()->preferred_group(size_t(1) << 20));
  else
    return -1;
  return 0;
}

int32_t ldpc_toolbox_sim_set(void *sim, const char *key, int64_t value) {
  auto *s = static_cast<ldpc::Simulator *>(sim);
  if (!s || !key) return -1;
  const std::string k = key;
  if (k == "group_size" && value >= 0) {
    s->decoder()->set_group_size(static_cast<size_t>(value));
    return 0;
  }
  if (k == "pooling") {  // 0: every chunk runs the full iteration budget (no straggler pool)
    s->set_pooling(value != 0);
    return 0;
  }
  if (k == "soft_bits") {  // 8 (the 8-bit implementations only) or 32
    g_last_error.clear();
    const bool ok = s->set_soft_bits(value);
    if (!ok) set_error(s->last_error());
    return ok ? 0 : -1;
  }
  if (k == "fading_block") {  // 0 (none) .. 0x7fffffff symbols per gain
    g_last_error.clear();
    const bool ok = s->set_fading_block(value);
    if (!ok) set_error(s->last_error());
    return ok ? 0 : -1;
  }
  if (k == "streaming") return 0;  // accepted, no effect (continuous batching: profiles/r03_continuous_batching.txt)
  if (k == "modulation" || k == "interleaving") {
    g_last_error.clear();
    const bool ok = k == "modulation" ? s->set_modulation(static_cast<int>(value)) : s->set_interleaving(value);
    if (!ok) set_error(s->last_error());
    return ok ? 0 : -1;
  }
  return s->decoder()->set_option(k, value) ? 0 : -1;
}

int32_t ldpc_toolbox_sim_set_constellation(void *sim, void *demod, int32_t max_log) {
  g_last_error.clear();
  auto *s = static_cast<ldpc::Simulator *>(sim);
  if (!s) {
    set_error("null argument");
    return -1;
  }
  auto *h = static_cast<DemodHandle *>(demod);
  if (s->set_constellation(h ? &h->c : nullptr, max_log != 0)) return 0;
  set_error(s->last_error());
  return -1;
}

int32_t ldpc_toolbox_sim_set_bch(void *sim, void *bch) {
  g_last_error.clear();
  auto *s = static_cast<ldpc::Simulator *>(sim);
  if (!s) {
    set_error("null argument");
    return -1;
  }
  auto *h = static_cast<BchHandle *>(bch);
  if (s->set_bch(h ? &h->code : nullptr)) return 0;
  set_error(s->last_error());
  return -1;
}

// ---- PART 4: batched soft demapper -----------------------------------------------------------------

void *ldpc_toolbox_demod_ctor(const char *modulation, int32_t device) {
  g_last_error.clear();
  ldpc::Constellation c;
  if (!modulation || !ldpc::named_constellation(modulation, &c)) {
    set_error("unknown modulation (expected BPSK, QPSK or 8PSK; other constellations through ldpc_toolbox_demod_ctor_table)");
    return nullptr;
  }
  return make_demod(c, device);
}

void *ldpc_toolbox_demod_ctor_table(const double *points_re_im, uint32_t bits_per_symbol, int32_t energy_term,
                                    int32_t device) {
  g_last_error.clear();
  ldpc::Constellation c;
  std::string err;
  if (!ldpc::table_constellation(points_re_im, bits_per_symbol, energy_term != 0, &c, &err)) {
    set_error(err);
    return nullptr;
  }
  return make_demod(c, device);
}

void ldpc_toolbox_demod_dtor(void *demod) { delete static_cast<DemodHandle *>(demod); }

int32_t ldpc_toolbox_demod_run_f32(void *demod, float *llrs, size_t llrs_len, const float *symbols, size_t symbols_len,
                                   size_t batch, double noise_sigma, int32_t interleaving, int32_t max_log) {
  return demod_run(demod, llrs, llrs_len, symbols, symbols_len, batch, false, noise_sigma, interleaving, max_log, false, nullptr);
}

int32_t ldpc_toolbox_demod_run_f64(void *demod, double *llrs, size_t llrs_len, const double *symbols, size_t symbols_len,
                                   size_t batch, double noise_sigma, int32_t interleaving, int32_t max_log) {
  return demod_run(demod, llrs, llrs_len, symbols, symbols_len, batch, true, noise_sigma, interleaving, max_log, false, nullptr);
}

int32_t ldpc_toolbox_demod_run_f32_device(void *demod, float *llrs, size_t llrs_len, const float *symbols,
                                          size_t symbols_len, size_t batch, double noise_sigma, int32_t interleaving,
                                          int32_t max_log, void *hip_stream) {
  return demod_run(demod, llrs, llrs_len, symbols, symbols_len, batch, false, noise_sigma, interleaving, max_log, true, hip_stream);
}

int32_t ldpc_toolbox_demod_run_f64_device(void *demod, double *llrs, size_t llrs_len, const double *symbols,
                                          size_t symbols_len, size_t batch, double noise_sigma, int32_t interleaving,
                                          int32_t max_log, void *hip_stream) {
  return demod_run(demod, llrs, llrs_len, symbols, symbols_len, batch, true, noise_sigma, interleaving, max_log, true, hip_stream);
}

int32_t ldpc_toolbox_mod_run_f32(void *demod, float *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len,
                                 size_t batch, int32_t interleaving) {
  return mod_run(demod, symbols, symbols_len, bits, bits_len, batch, false, interleaving, false, nullptr);
}

int32_t ldpc_toolbox_mod_run_f64(void *demod, double *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len,
                                 size_t batch, int32_t interleaving) {
  return mod_run(demod, symbols, symbols_len, bits, bits_len, batch, true, interleaving, false, nullptr);
}

int32_t ldpc_toolbox_mod_run_f32_device(void *demod, float *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len,
                                        size_t batch, int32_t interleaving, void *hip_stream) {
  return mod_run(demod, symbols, symbols_len, bits, bits_len, batch, false, interleaving, true, hip_stream);
}

int32_t ldpc_toolbox_mod_run_f64_device(void *demod, double *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len,
                                        size_t batch, int32_t interleaving, void *hip_stream) {
  return mod_run(demod, symbols, symbols_len, bits, bits_len, batch, true, interleaving, true, hip_stream);
}

int32_t ldpc_toolbox_awgn_run_f32(void *demod, float *symbols, size_t symbols_len, size_t batch, double noise_sigma,
                                  uint64_t seed, uint64_t first_frame) {
  return awgn_run(demod, symbols, symbols_len, batch, false, noise_sigma, seed, first_frame, false, nullptr);
}

int32_t ldpc_toolbox_awgn_run_f64(void *demod, double *symbols, size_t symbols_len, size_t batch, double noise_sigma,
                                  uint64_t seed, uint64_t first_frame) {
  return awgn_run(demod, symbols, symbols_len, batch, true, noise_sigma, seed, first_frame, false, nullptr);
}

int32_t ldpc_toolbox_awgn_run_f32_device(void *demod, float *symbols, size_t symbols_len, size_t batch, double noise_sigma,
                                         uint64_t seed, uint64_t first_frame, void *hip_stream) {
  return awgn_run(demod, symbols, symbols_len, batch, false, noise_sigma, seed, first_frame, true, hip_stream);
}

int32_t ldpc_toolbox_awgn_run_f64_device(void *demod, double *symbols, size_t symbols_len, size_t batch, double noise_sigma,
                                         uint64_t seed, uint64_t first_frame, void *hip_stream) {
  return awgn_run(demod, symbols, symbols_len, batch, true, noise_sigma, seed, first_frame, true, hip_stream);
}

int32_t ldpc_toolbox_fading_run_f32(void *demod, float *symbols, float *scale, size_t symbols_len, size_t batch, double noise_sigma,
                                    uint32_t block, uint64_t seed, uint64_t first_frame) {
  return fading_run(demod, symbols, scale, symbols_len, batch, false, noise_sigma, block, seed, first_frame, false, nullptr);
}

int32_t ldpc_toolbox_fading_run_f64(void *demod, double *symbols, double *scale, size_t symbols_len, size_t batch, double noise_sigma,
                                    uint32_t block, uint64_t seed, uint64_t first_frame) {
  return fading_run(demod, symbols, scale, symbols_len, batch, true, noise_sigma, block, seed, first_frame, false, nullptr);
}

int32_t ldpc_toolbox_fading_run_f32_device(void *demod, float *symbols, float *scale, size_t symbols_len, size_t batch, double noise_sigma,
                                           uint32_t block, uint64_t seed, uint64_t first_frame, void *hip_stream) {
  return fading_run(demod, symbols, scale, symbols_len, batch, false, noise_sigma, block, seed, first_frame, true, hip_stream);
}

int32_t ldpc_toolbox_fading_run_f64_device(void *demod, double *symbols, double *scale, size_t symbols_len, size_t batch, double noise_sigma,
                                           uint32_t block, uint64_t seed, uint64_t first_frame, void *hip_stream) {
  return fading_run(demod, symbols, scale, symbols_len, batch, true, noise_sigma, block, seed, first_frame, true, hip_stream);
}

int32_t ldpc_toolbox_demod_get(void *demod, const char *key, int64_t *value) {
  auto *h = static_cast<DemodHandle *>(demod);
  if (!h || !key || !value) return -1;
  const std::string k = key;
  if (k == "bits_per_symbol")
    *value = h->c.bits;
  else if (k == "points")
    *value = h->c.points();
  else if (k == "energy_term")
    *value = h->c.energy ? 1 : 0;
  else if (k == "device")
    *value = h->dev ? h->dev->device() : -1;
  else
    return -1;
  return 0;
}

// ---- PART 5: batched BCH outer code ----------------------------------------------------------------

void *ldpc_toolbox_bch_ctor(const char *spec, int32_t device) {
  g_last_error.clear();
  if (!spec) {
    set_error("null BCH spec");
    return nullptr;
  }
  auto h = std::make_unique<BchHandle>();
  std::string err;
  if (!ldpc::bch::parse_spec(spec, &h->code, &err)) {
    set_error(err);
    return nullptr;
  }
  h->device = device < 0 ? default_device() : device;
  return h.release();
}

void ldpc_toolbox_bch_dtor(void *bch) { delete static_cast<BchHandle *>(bch); }

int32_t ldpc_toolbox_bch_get(void *bch, const char *key, int64_t *value) {
  auto *h = static_cast<BchHandle *>(bch);
  if (!h || !key || !value) return -1;
  const std::string k = key;
  if (k == "n")
    *value = h->code.n;
  else if (k == "k")
    *value = h->code.k;
  else if (k == "t")
    *value = h->code.t;
  else if (k == "m")
    *value = h->code.m;
  else if (k == "parity")
    *value = h->code.parity;
  else if (k == "primitive")
    *value = h->code.poly;
  else if (k == "pass_frames")  // frames per pass of a batched call
    *value = static_cast<int64_t>(ldpc::kBchPassFrames);
  else if (k == "stage_frames")  // frames a host entry stages on the device at a time
    *value = static_cast<int64_t>(std::max<size_t>(std::min(ldpc::kBchStageFrames, ldpc::kBchStageBytes / h->code.n), 1));
  else if (k == "device")
    *value = h->dev ? h->dev->device() : -1;
  else
    return -1;
  return 0;
}

size_t ldpc_toolbox_bch_generator(void *bch, uint8_t *coefficients, size_t len) {
  auto *h = static_cast<BchHandle *>(bch);
  if (!h) return 0;
  const std::vector<uint8_t> &g = h->code.g;
  if (coefficients && len >= g.size()) std::memcpy(coefficients, g.data(), g.size());
  return g.size();
}

int32_t ldpc_toolbox_bch_encode_batch(void *bch, uint8_t *output, size_t output_len, const uint8_t *input, size_t input_len,
                                      size_t batch) {
  return bch_run(bch, false, output, output_len, input, input_len, batch, nullptr, false, nullptr);
}

int32_t ldpc_toolbox_bch_encode_batch_device(void *bch, uint8_t *output, size_t output_len, const uint8_t *input,
                                             size_t input_len, size_t batch, void *hip_stream) {
  return bch_run(bch, false, output, output_len, input, input_len, batch, nullptr, true, hip_stream);
}

int32_t ldpc_toolbox_bch_decode_batch(void *bch, uint8_t *output, size_t output_len, const uint8_t *input, size_t input_len,
                                      size_t batch, int32_t *errors) {
  return bch_run(bch, true, output, output_len, input, input_len, batch, errors, false, nullptr);
}

int32_t ldpc_toolbox_bch_decode_batch_device(void *bch, uint8_t *output, size_t output_len, const uint8_t *input,
                                             size_t input_len, size_t batch, int32_t *errors, void *hip_stream) {
  return bch_run(bch, true, output, output_len, input, input_len, batch, errors, true, hip_stream);
}

// ---- PART 6: batched 5G NR rate matching and rate recovery -----------------------------------------

void *ldpc_toolbox_nr_rm_ctor(const char *spec, int32_t device) {
  g_last_error.clear();
  if (!spec) {
    set_error("null rate matcher spec");
    return nullptr;
  }
  auto h = std::make_unique<NrRmHandle>();
  std::string err;
  if (!parse_nr_rm_spec(spec, &h->c, &err)) {
    set_error(err);
    return nullptr;
  }
  h->device = device < 0 ? default_device() : device;
  return h.release();
}

void ldpc_toolbox_nr_rm_dtor(void *rm) { delete static_cast<NrRmHandle *>(rm); }

int32_t ldpc_toolbox_nr_rm_get(void *rm, const char *key, int64_t *value) {
  auto *h = static_cast<NrRmHandle *>(rm);
  if (!h || !key || !value) return -1;
  const std::string k = key;
  if (k == "n")
    *value = h->c.n;
  else if (k == "k")
    *value = h->c.k;
  else if (k == "zc")
    *value = h->c.zc;
  else if (k == "base_graph")
    *value = h->c.bg;
  else if (k == "fillers")
    *value = h->c.fillers;
  else if (k == "n_cb")
    *value = h->c.ncb;
  else if (k == "buffer_len")  // L: the non-NULL bits of the circular buffer
    *value = h->c.l;
  else if (k.size() == 4 && k.compare(0, 3, "k0_") == 0 && k[3] >= '0' && k[3] <= '3')
    *value = ldpc::nrrm::k0_of(h->c, static_cast<uint32_t>(k[3] - '0'));
  else if (k == "pass_elements")  // elements per pass of a batched call
    *value = static_cast<int64_t>(ldpc::kNrRmPassElements);
  else if (k == "stage_bytes")  // bytes of its longest rows a host entry stages on the device at a time
    *value = static_cast<int64_t>(ldpc::kNrRmStageBytes);
  else if (k == "device")
    *value = h->dev ? h->dev->device() : -1;
  else
    return -1;
  return 0;
}

int32_t ldpc_toolbox_nr_rm_match(void *rm, uint8_t *output, size_t e, const uint8_t *codewords, size_t n, size_t batch, uint32_t rv,
                                 uint32_t qm) {
  return nr_rm_match(rm, output, e, codewords, n, batch, rv, qm, false, nullptr);
}

int32_t ldpc_toolbox_nr_rm_match_device(void *rm, uint8_t *output, size_t e, const uint8_t *codewords, size_t n, size_t batch,
                                        uint32_t rv, uint32_t qm, void *hip_stream) {
  return nr_rm_match(rm, output, e, codewords, n, batch, rv, qm, true, hip_stream);
}

int32_t ldpc_toolbox_nr_rm_recover_f32(void *rm, float *llrs, size_t n, const float *rx, size_t e, size_t batch, uint32_t rv,
                                       uint32_t qm, double filler_llr, int32_t combine) {
  return nr_rm_recover(rm, llrs, n, rx, e, batch, rv, qm, false, filler_llr, combine, false, nullptr);
}

int32_t ldpc_toolbox_nr_rm_recover_f64(void *rm, double *llrs, size_t n, const double *rx, size_t e, size_t batch, uint32_t rv,
                                       uint32_t qm, double filler_llr, int32_t combine) {
  return nr_rm_recover(rm, llrs, n, rx, e, batch, rv, qm, true, filler_llr, combine, false, nullptr);
}

int32_t ldpc_toolbox_nr_rm_recover_f32_device(void *rm, float *llrs, size_t n, const float *rx, size_t e, size_t batch, uint32_t rv,
                                              uint32_t qm, double filler_llr, int32_t combine, void *hip_stream) {
  return nr_rm_recover(rm, llrs, n, rx, e, batch, rv, qm, false, filler_llr, combine, true, hip_stream);
}

int32_t ldpc_toolbox_nr_rm_recover_f64_device(void *rm, double *llrs, size_t n, const double *rx, size_t e, size_t batch, uint32_t rv,
                                              uint32_t qm, double filler_llr, int32_t combine, void *hip_stream) {
  return nr_rm_recover(rm, llrs, n, rx, e, batch, rv, qm, true, filler_llr, combine, true, hip_stream);
}

int32_t ldpc_toolbox_sim_set_rate_match(void *sim, void *rm, size_t e, uint32_t rv, uint32_t qm) {
  g_last_error.clear();
  auto *s = static_cast<ldpc::Simulator *>(sim);
  if (!s) {
    set_error("null argument");
    return -1;
  }
  auto *h = static_cast<NrRmHandle *>(rm);
  if (s->set_rate_match(h ? &h->c : nullptr, e, rv, qm)) return 0;
  set_error(s->last_error());
  return -1;
}

int32_t ldpc_toolbox_sim_set_harq(void *sim, void *rm, const uint64_t *e, const uint32_t *rv, uint32_t transmissions, uint32_t qm) {
  g_last_error.clear();
  auto *s = static_cast<ldpc::Simulator *>(sim);
  auto *h = static_cast<NrRmHandle *>(rm);
  // (what needs no simulator comes first: a sequence that is none is refused as such on any machine)
  if (h != nullptr)
    if (const char *why = ldpc::nrharq::sequence_error(e, rv, transmissions, qm, 1)) {
      set_error(why);
      return -1;
    }
  if (!s) {
    set_error("null argument");
    return -1;
  }
  if (s->set_harq(h ? &h->c : nullptr, e, rv, transmissions, qm)) return 0;
  set_error(s->last_error());
  return -1;
}

int32_t ldpc_toolbox_sim_run_harq(void *sim, double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames, uint32_t max_iterations,
                                  uint64_t *counters, uint64_t *per_tx) {
  g_last_error.clear();
  auto *s = static_cast<ldpc::Simulator *>(sim);
  if (!s || !counters || !per_tx) {
    set_error("null argument");
    return -1;
  }
  const int rc = s->run_harq(ebn0_db, seed, first_frame, frames, max_iterations, counters, per_tx);
  if (rc) set_error(s->last_error());
  return rc;
}

int32_t ldpc_toolbox_sim_generate_harq(void *sim, double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames, uint32_t transmission,
                                       float *llrs, uint32_t *pool_index) {
  g_last_error.clear();
  auto *s = static_cast<ldpc::Simulator *>(sim);
  if (!s || !llrs) {
    set_error("null argument");
    return -1;
  }
  const int rc = s->generate_harq(ebn0_db, seed, first_frame, frames, transmission, llrs, pool_index);
  if (rc) set_error(s->last_error());
  return rc;
}

// ---- PART 7: batched 5G NR transport block CRC, segmentation and concatenation -----------------------

void *ldpc_toolbox_nr_tb_ctor(const char *spec, int32_t device) {
  g_last_error.clear();
  if (!spec) {
    set_error("null transport block spec");
    return nullptr;
  }
  auto h = std::make_unique<NrTbHandle>();
  std::string err;
  if (!parse_nr_tb_spec(spec, &h->c, &err)) {
    set_error(err);
    return nullptr;
  }
  h->device = device < 0 ? default_device() : device;
  return h.release();
}

void ldpc_toolbox_nr_tb_dtor(void *tb) { delete static_cast<NrTbHandle *>(tb); }

int32_t ldpc_toolbox_nr_tb_get(void *tb, const char *key, int64_t *value) {
  auto *h = static_cast<NrTbHandle *>(tb);
  if (!h || !key || !value) return -1;
  const std::string k = key;
  const ldpc::nrtb::Config &c = h->c;
  if (k == "a")
    *value = c.a;
  else if (k == "base_graph")
    *value = c.bg;
  else if (k == "tb_crc")
    *value = c.l_tb;
  else if (k == "b")
    *value = c.b;
  else if (k == "c")
    *value = c.c;
  else if (k == "cb_crc")
    *value = c.l_cb;
  else if (k == "k_prime")
    *value = c.k_prime;
  else if (k == "k_b")
    *value = c.kb;
  else if (k == "zc")
    *value = c.zc;
  else if (k == "k")
    *value = c.k;
  else if (k == "fillers")
    *value = c.fillers;
  else if (k == "n")
    *value = c.n;
  else if (k == "pass_rows")  // code block rows per pass of segment / desegment
    *value = static_cast<int64_t>(ldpc::kNrTbPassRows);
  else if (k == "pass_elements")  // elements per pass of concatenate / split
    *value = static_cast<int64_t>(ldpc::kNrTbPassElements);
  else if (k == "stage_bytes")  // bytes of its longest side a host entry stages on the device at a time
    *value = static_cast<int64_t>(ldpc::kNrTbStageBytes);
  else if (k == "device")
    *value = h->dev ? h->dev->device() : -1;
  else
    return -1;
  return 0;
}

int32_t ldpc_toolbox_nr_base_graph(uint64_t a, double rate) { return ldpc::nrtb::base_graph(a, rate); }

int32_t ldpc_toolbox_nr_tb_block_lengths(void *tb, uint64_t g, uint64_t q, uint64_t *e_lo, uint64_t *e_hi, uint64_t *c_lo) {
  g_last_error.clear();
  auto *h = static_cast<NrTbHandle *>(tb);
  if (!h || !e_lo || !e_hi || !c_lo) return nr_tb_argument_error("null argument");
  if (const char *why = ldpc::nrtb::block_lengths(h->c, g, q, e_lo, e_hi, c_lo)) return nr_tb_argument_error(why);
  return 0;
}

int32_t ldpc_toolbox_nr_tb_segment(void *tb, uint8_t *rows, size_t k, const uint8_t *payload, size_t a, size_t batch) {
  return nr_tb_segment(tb, rows, k, payload, a, batch, false, nullptr);
}

int32_t ldpc_toolbox_nr_tb_segment_device(void *tb, uint8_t *rows, size_t k, const uint8_t *payload, size_t a, size_t batch,
                                          void *hip_stream) {
  return nr_tb_segment(tb, rows, k, payload, a, batch, true, hip_stream);
}

int32_t ldpc_toolbox_nr_tb_desegment(void *tb, uint8_t *payload, size_t a, uint8_t *tb_ok, uint8_t *cb_ok, const uint8_t *rows, size_t k,
                                     size_t batch) {
  return nr_tb_desegment(tb, payload, a, tb_ok, cb_ok, rows, k, batch, false, nullptr);
}

int32_t ldpc_toolbox_nr_tb_desegment_device(void *tb, uint8_t *payload, size_t a, uint8_t *tb_ok, uint8_t *cb_ok, const uint8_t *rows,
                                            size_t k, size_t batch, void *hip_stream) {
  return nr_tb_desegment(tb, payload, a, tb_ok, cb_ok, rows, k, batch, true, hip_stream);
}

int32_t ldpc_toolbox_nr_tb_concatenate(void *tb, uint8_t *output, size_t g, const uint8_t *packed, size_t q, size_t batch) {
  return nr_tb_repack(tb, output, packed, g, q, batch, false, false, false, nullptr);
}

int32_t ldpc_toolbox_nr_tb_concatenate_device(void *tb, uint8_t *output, size_t g, const uint8_t *packed, size_t q, size_t batch,
                                              void *hip_stream) {
  return nr_tb_repack(tb, output, packed, g, q, batch, false, false, true, hip_stream);
}

int32_t ldpc_toolbox_nr_tb_split_f32(void *tb, float *packed, const float *rx, size_t g, size_t q, size_t batch) {
  return nr_tb_repack(tb, packed, rx, g, q, batch, true, false, false, nullptr);
}

int32_t ldpc_toolbox_nr_tb_split_f64(void *tb, double *packed, const double *rx, size_t g, size_t q, size_t batch) {
  return nr_tb_repack(tb, packed, rx, g, q, batch, true, true, false, nullptr);
}

int32_t ldpc_toolbox_nr_tb_split_f32_device(void *tb, float *packed, const float *rx, size_t g, size_t q, size_t batch, void *hip_stream) {
  return nr_tb_repack(tb, packed, rx, g, q, batch, true, false, true, hip_stream);
}

int32_t ldpc_toolbox_nr_tb_split_f64_device(void *tb, double *packed, const double *rx, size_t g, size_t q, size_t batch, void *hip_stream) {
  return nr_tb_repack(tb, packed, rx, g, q, batch, true, true, true, hip_stream);
}

// ---- PART 8: batched 5G NR modulation mapper, soft demapper and scrambling ----------------------------

void *ldpc_toolbox_nr_qam_ctor(const char *spec, int32_t device) {
  g_last_error.clear();
  if (!spec) {
    set_error("null NR modulation spec");
    return nullptr;
  }
  auto h = std::make_unique<NrQamHandle>();
  std::string err;
  if (!ldpc::nrqam::parse_spec(spec, &h->c, &err)) {
    set_error(err);
    return nullptr;
  }
  h->device = device < 0 ? default_device() : device;
  return h.release();
}

void ldpc_toolbox_nr_qam_dtor(void *qam) { delete static_cast<NrQamHandle *>(qam); }

int32_t ldpc_toolbox_nr_qam_get(void *qam, const char *key, int64_t *value) {
  auto *h = static_cast<NrQamHandle *>(qam);
  if (!h || !key || !value) return -1;
  const std::string k = key;
  if (k == "bits_per_symbol")
    *value = h->c.qm;
  else if (k == "points")
    *value = h->c.points();
  else if (k == "levels")
    *value = h->c.levels();
  else if (k == "device")
    *value = h->dev ? h->dev->device() : -1;
  else if (k == "sequence_launches")  // runs of the Gold kernel so far: a repeated (c_init, length) does not add one
    *value = h->dev ? static_cast<int64_t>(h->dev->sequence_launches()) : 0;
  else
    return -1;
  return 0;
}

size_t ldpc_toolbox_nr_qam_points(void *qam, double *re_im, size_t len) {
  auto *h = static_cast<NrQamHandle *>(qam);
  if (!h) return 0;
  const size_t points = h->c.points();
  if (re_im && len >= 2 * points)
    for (uint32_t v = 0; v < points; v++) {
      re_im[2 * v] = h->c.amp[ldpc::nrqam::axis_index(h->c, v, 0)];
      re_im[2 * v + 1] = h->c.amp[ldpc::nrqam::axis_index(h->c, v, 1)];
    }
  return points;
}

int32_t ldpc_toolbox_nr_qam_sequence(void *qam, uint8_t *c, size_t len, int64_t c_init) {
  g_last_error.clear();
  auto *h = static_cast<NrQamHandle *>(qam);
  if (!h) return nr_qam_refuse("null NR modulation handle");
  if (const char *why = ldpc::nrqam::sequence_argument_error(len, c_init)) return nr_qam_refuse(why);
  if (len == 0) return 0;
  if (!c) return nr_qam_refuse("null sequence buffer");
  if (int32_t rc = nr_qam_device_state(h)) return rc;
  if (h->dev->sequence_host(c, len, static_cast<uint32_t>(c_init)) == 0) return 0;
  set_error(h->dev->last_error());
  return LDPC_TOOLBOX_ERR_DEVICE;
}

int32_t ldpc_toolbox_nr_qam_mod_f32(void *qam, float *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len, size_t batch,
                                    int64_t c_init) {
  return nr_qam_mod(qam, symbols, symbols_len, bits, bits_len, batch, false, c_init, false, nullptr);
}

int32_t ldpc_toolbox_nr_qam_mod_f64(void *qam, double *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len, size_t batch,
                                    int64_t c_init) {
  return nr_qam_mod(qam, symbols, symbols_len, bits, bits_len, batch, true, c_init, false, nullptr);
}

int32_t ldpc_toolbox_nr_qam_mod_f32_device(void *qam, float *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len,
                                           size_t batch, int64_t c_init, void *hip_stream) {
  return nr_qam_mod(qam, symbols, symbols_len, bits, bits_len, batch, false, c_init, true, hip_stream);
}

int32_t ldpc_toolbox_nr_qam_mod_f64_device(void *qam, double *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len,
                                           size_t batch, int64_t c_init, void *hip_stream) {
  return nr_qam_mod(qam, symbols, symbols_len, bits, bits_len, batch, true, c_init, true, hip_stream);
}

int32_t ldpc_toolbox_nr_qam_demod_f32(void *qam, float *llrs, size_t llrs_len, const float *symbols, size_t symbols_len, size_t batch,
                                      double noise_sigma, int32_t max_log, int64_t c_init) {
  return nr_qam_demod(qam, llrs, llrs_len, symbols, symbols_len, batch, false, noise_sigma, max_log, c_init, false, nullptr);
}

int32_t ldpc_toolbox_nr_qam_demod_f64(void *qam, double *llrs, size_t llrs_len, const double *symbols, size_t symbols_len, size_t batch,
                                      double noise_sigma, int32_t max_log, int64_t c_init) {
  return nr_qam_demod(qam, llrs, llrs_len, symbols, symbols_len, batch, true, noise_sigma, max_log, c_init, false, nullptr);
}

int32_t ldpc_toolbox_nr_qam_demod_f32_device(void *qam, float *llrs, size_t llrs_len, const float *symbols, size_t symbols_len,
                                             size_t batch, double noise_sigma, int32_t max_log, int64_t c_init, void *hip_stream) {
  return nr_qam_demod(qam, llrs, llrs_len, symbols, symbols_len, batch, false, noise_sigma, max_log, c_init, true, hip_stream);
}

int32_t ldpc_toolbox_nr_qam_demod_f64_device(void *qam, double *llrs, size_t llrs_len, const double *symbols, size_t symbols_len,
                                             size_t batch, double noise_sigma, int32_t max_log, int64_t c_init, void *hip_stream) {
  return nr_qam_demod(qam, llrs, llrs_len, symbols, symbols_len, batch, true, noise_sigma, max_log, c_init, true, hip_stream);
}

int32_t ldpc_toolbox_sim_set_nr_qam(void *sim, void *qam, int32_t max_log) {
  g_last_error.clear();
  auto *s = static_cast<ldpc::Simulator *>(sim);
  if (!s) {
    set_error("null argument");
    return -1;
  }
  auto *h = static_cast<NrQamHandle *>(qam);
  if (s->set_nr_qam(h ? &h->c : nullptr, max_log != 0)) return 0;
  set_error(s->last_error());
  return -1;
}

// ---- PART 9: the 8-bit soft-bit receive path -----------------------------------------------------------

int32_t ldpc_toolbox_decoder_decode_batch_i8(void *decoder, uint8_t *output, size_t output_len, const int8_t *llrs, size_t llrs_len,
                                             size_t batch, uint32_t max_iterations, int32_t *iterations, int16_t *posterior) {
  return decode_batch<int8_t>(decoder, output, output_len, llrs, llrs_len, batch, max_iterations, iterations, posterior, false, nullptr);
}

int32_t ldpc_toolbox_decoder_decode_batch_i8_device(void *decoder, uint8_t *output, size_t output_len, const int8_t *llrs,
                                                    size_t llrs_len, size_t batch, uint32_t max_iterations, int32_t *iterations,
                                                    int16_t *posterior, void *hip_stream) {
  return decode_batch<int8_t>(decoder, output, output_len, llrs, llrs_len, batch, max_iterations, iterations, posterior, true, hip_stream);
}

int32_t ldpc_toolbox_nr_demap_i8(void *qam, int8_t *llrs, size_t llrs_len, const float *symbols, size_t symbols_len, size_t batch,
                                 double noise_sigma, int32_t max_log, int64_t c_init) {
  return nr_demap_i8(qam, llrs, llrs_len, symbols, symbols_len, batch, noise_sigma, max_log, c_init, false, nullptr);
}

int32_t ldpc_toolbox_nr_demap_i8_device(void *qam, int8_t *llrs, size_t llrs_len, const float *symbols, size_t symbols_len, size_t batch,
                                        double noise_sigma, int32_t max_log, int64_t c_init, void *hip_stream) {
  return nr_demap_i8(qam, llrs, llrs_len, symbols, symbols_len, batch, noise_sigma, max_log, c_init, true, hip_stream);
}

int32_t ldpc_toolbox_nr_rm_recover_i8(void *rm, int8_t *llrs, size_t n, const int8_t *rx, size_t e, size_t batch, uint32_t rv, uint32_t qm,
                                      int32_t filler, int32_t combine) {
  return nr_rm_recover_i8(rm, llrs, n, rx, e, batch, rv, qm, filler, combine, false, nullptr);
}

int32_t ldpc_toolbox_nr_rm_recover_i8_device(void *rm, int8_t *llrs, size_t n, const int8_t *rx, size_t e, size_t batch, uint32_t rv,
                                             uint32_t qm, int32_t filler, int32_t combine, void *hip_stream) {
  return nr_rm_recover_i8(rm, llrs, n, rx, e, batch, rv, qm, filler, combine, true, hip_stream);
}

// ---- PART 10: the NR demapper with a scale per symbol ----------------------------------------------------

int32_t ldpc_toolbox_nr_demap_csi_f32(void *qam, float *llrs, size_t llrs_len, const float *symbols, const float *scale, size_t symbols_len,
                                      size_t batch, int32_t max_log, int64_t c_init) {
  return nr_demap_csi(qam, llrs, llrs_len, symbols, scale, symbols_len, batch, 4, max_log, c_init, false, nullptr);
}

int32_t ldpc_toolbox_nr_demap_csi_f64(void *qam, double *llrs, size_t llrs_len, const double *symbols, const double *scale,
                                      size_t symbols_len, size_t batch, int32_t max_log, int64_t c_init) {
  return nr_demap_csi(qam, llrs, llrs_len, symbols, scale, symbols_len, batch, 8, max_log, c_init, false, nullptr);
}

int32_t ldpc_toolbox_nr_demap_csi_i8(void *qam, int8_t *llrs, size_t llrs_len, const float *symbols, const float *scale, size_t symbols_len,
                                     size_t batch, int32_t max_log, int64_t c_init) {
  return nr_demap_csi(qam, llrs, llrs_len, symbols, scale, symbols_len, batch, 1, max_log, c_init, false, nullptr);
}

int32_t ldpc_toolbox_nr_demap_csi_f32_device(void *qam, float *llrs, size_t llrs_len, const float *symbols, const float *scale,
                                             size_t symbols_len, size_t batch, int32_t max_log, int64_t c_init, void *hip_stream) {
  return nr_demap_csi(qam, llrs, llrs_len, symbols, scale, symbols_len, batch, 4, max_log, c_init, true, hip_stream);
}

int32_t ldpc_toolbox_nr_demap_csi_f64_device(void *qam, double *llrs, size_t llrs_len, const double *symbols, const double *scale,
                                             size_t symbols_len, size_t batch, int32_t max_log, int64_t c_init, void *hip_stream) {
  return nr_demap_csi(qam, llrs, llrs_len, symbols, scale, symbols_len, batch, 8, max_log, c_init, true, hip_stream);
}

int32_t ldpc_toolbox_nr_demap_csi_i8_device(void *qam, int8_t *llrs, size_t llrs_len, const float *symbols, const float *scale,
                                            size_t symbols_len, size_t batch, int32_t max_log, int64_t c_init, void *hip_stream) {
  return nr_demap_csi(qam, llrs, llrs_len, symbols, scale, symbols_len, batch, 1, max_log, c_init, true, hip_stream);
}

// ---- PART 11: the 5G NR link handle: one-call transport blocks with HARQ slots --------------------------

void *ldpc_toolbox_nr_link_ctor(const char *spec, const char *implementation, uint32_t slots, int32_t device) {
  g_last_error.clear();
  auto refuse = [](const std::string &why) -> void * {
    set_error(why);
    return nullptr;
  };
  if (!spec) return refuse("null link spec");
  if (!implementation) return refuse("invalid decoder implementation");
  auto h = std::make_unique<NrLinkHandle>();
  if (const char *why = ldpc::nrlink::parse_spec(spec, &h->c)) return refuse(why);
  if (slots == 0) return refuse("a link handle has at least one HARQ slot");
  if (uint64_t(slots) * h->c.tb.c > 0x7fffffffu) return refuse("slots * C above 0x7fffffff");
  std::string err;
  if (!ldpc::parse_implementation(implementation, &h->impl, &err)) return refuse(err);
  h->slots = slots;
  h->filler_llr = std::numeric_limits<double>::infinity();
  h->device = device < 0 ? default_device() : device;
  return h.release();
}

void ldpc_toolbox_nr_link_dtor(void *link) { delete static_cast<NrLinkHandle *>(link); }

int32_t ldpc_toolbox_nr_link_get(void *link, const char *key, int64_t *value) {
  auto *h = static_cast<NrLinkHandle *>(link);
  if (!h || !key || !value) return -1;
  const std::string k = key;
  const ldpc::nrtb::Config &c = h->c.tb;
  const std::pair<const char *, int64_t> table[] = {
      {"a", c.a}, {"base_graph", c.bg}, {"tb_crc", c.l_tb}, {"b", c.b}, {"c", c.c}, {"cb_crc", c.l_cb}, {"k_prime", c.k_prime},
      {"k_b", c.kb}, {"zc", c.zc}, {"k", c.k}, {"fillers", c.fillers}, {"n", c.n},
      {"g", h->c.len.g}, {"qm", h->c.qm}, {"layers", h->c.layers}, {"q", h->c.q}, {"e_lo", h->c.len.e_lo}, {"e_hi", h->c.len.e_hi},
      {"c_lo", h->c.len.c_lo}, {"symbols", h->c.symbols}, {"slots", h->slots},
      {"max_log", h->max_log ? 1 : 0},
      {"soft_bits", h->soft_bits},
      {"soft_bytes", static_cast<int64_t>(ldpc::nrlink::soft_bytes(h->c, h->slots, h->soft_bits))},  // of the slots' soft rows
      {"pass_elements", static_cast<int64_t>(h->pass_elements)},  // elements (transport block, block, column) per launch of the fused recover kernel
      {"stage_bytes", static_cast<int64_t>(ldpc::nrlink::kStageBytes)},  // codeword bytes a transmit call takes through the handle's buffers at a time
      {"device", h->dev ? h->dev->device() : -1},
      {"decoded_rows", h->dev ? static_cast<int64_t>(h->dev->decoded_rows()) : 0},
      {"skipped_rows", h->dev ? static_cast<int64_t>(h->dev->skipped_rows()) : 0},
  };
  for (const auto &entry : table)
    if (k == entry.first) {
      *value = entry.second;
      return 0;
    }
  return -1;
}

int32_t ldpc_toolbox_nr_link_set(void *link, const char *key, int64_t value) {
  g_last_error.clear();
  auto *h = static_cast<NrLinkHandle *>(link);
  if (!h || !key) return nr_link_refuse("null link handle or key");
  const std::string k = key;
  if (k == "max_log") {
    if (value != 0 && value != 1) return nr_link_refuse("max_log must be 0 or 1");
    h->max_log = value != 0;
  } else if (k == "pass_elements") {
    if (const char *why = ldpc::nrlink::pass_elements_error(value)) return nr_link_refuse(why);
    h->pass_elements = static_cast<uint64_t>(value);
  } else if (k == "soft_bits") {
    if (const char *why = ldpc::nrlink::soft_bits_error(value, h->soft_bits, h->impl.i8, h->filler_llr, h->dev != nullptr)) return nr_link_refuse(why);
    h->soft_bits = static_cast<uint32_t>(value);
  } else {
    return nr_link_refuse("unknown key");
  }
  return 0;
}

int32_t ldpc_toolbox_nr_link_set_filler_llr(void *link, double filler_llr) {
  g_last_error.clear();
  auto *h = static_cast<NrLinkHandle *>(link);
  if (!h) return nr_link_refuse("null link handle");
  if (const char *why = ldpc::nrlink::filler_llr_error(filler_llr)) return nr_link_refuse(why);
  if (h->soft_bits == 8)
    if (const char *why = ldpc::nrlink::filler_soft_bit_error(filler_llr)) return nr_link_refuse(why);
  h->filler_llr = filler_llr;
  return 0;
}

int32_t ldpc_toolbox_nr_link_transmit_f32(void *link, float *symbols, size_t symbols_len, const uint8_t *payload, size_t a, size_t batch,
                                          uint32_t rv, int64_t c_init) {
  return nr_link_transmit(link, symbols, symbols_len, payload, a, batch, rv, c_init, false, nullptr);
}

int32_t ldpc_toolbox_nr_link_transmit_f32_device(void *link, float *symbols, size_t symbols_len, const uint8_t *payload, size_t a, size_t batch,
                                                 uint32_t rv, int64_t c_init, void *hip_stream) {
  return nr_link_transmit(link, symbols, symbols_len, payload, a, batch, rv, c_init, true, hip_stream);
}

int32_t ldpc_toolbox_nr_link_receive_f32(void *link, uint8_t *payload, size_t a, uint8_t *tb_ok, uint8_t *cb_ok, int32_t *iterations,
                                         const float *symbols, const float *scale, size_t symbols_len, size_t batch, double noise_sigma,
                                         uint32_t rv, int64_t c_init, uint32_t first_slot, int32_t combine, uint32_t max_iterations) {
  return nr_link_receive(link, payload, a, tb_ok, cb_ok, iterations, symbols, scale, symbols_len, batch, noise_sigma, rv, c_init, first_slot,
                         combine, max_iterations, false, nullptr);
}

int32_t ldpc_toolbox_nr_link_receive_f32_device(void *link, uint8_t *payload, size_t a, uint8_t *tb_ok, uint8_t *cb_ok, int32_t *iterations,
                                                const float *symbols, const float *scale, size_t symbols_len, size_t batch,
                                                double noise_sigma, uint32_t rv, int64_t c_init, uint32_t first_slot, int32_t combine,
                                                uint32_t max_iterations, void *hip_stream) {
  return nr_link_receive(link, payload, a, tb_ok, cb_ok, iterations, symbols, scale, symbols_len, batch, noise_sigma, rv, c_init, first_slot,
                         combine, max_iterations, true, hip_stream);
}

int32_t ldpc_toolbox_nr_link_recover_f32_device(void *link, const float *rx, size_t g, size_t batch, uint32_t rv, uint32_t first_slot,
                                                int32_t combine, void *hip_stream) {
  g_last_error.clear();
  auto *h = static_cast<NrLinkHandle *>(link);
  if (!h) return nr_link_refuse("null link handle");
  if (h->soft_bits != 32) return nr_link_wrong_mode(h);
  return nr_link_recover(h, rx, sizeof(float), g, batch, rv, first_slot, combine, hip_stream);
}

int32_t ldpc_toolbox_nr_link_slot_state(void *link, float *soft, uint8_t *done, uint8_t *rows, uint32_t first_slot, size_t batch) {
  g_last_error.clear();
  auto *h = static_cast<NrLinkHandle *>(link);
  if (!h) return nr_link_refuse("null link handle");
  if (soft && h->soft_bits != 32) return nr_link_wrong_mode(h);
  return nr_link_slot_state(h, soft, done, rows, first_slot, batch);
}

// ---- PART 12: 8-bit HARQ soft buffers in the NR link handle ----------------------------------------------

int32_t ldpc_toolbox_nr_harq_slots_recover_i8_device(void *link, const int8_t *rx, size_t g, size_t batch, uint32_t rv, uint32_t first_slot,
                                                     int32_t combine, void *hip_stream) {
  g_last_error.clear();
  auto *h = static_cast<NrLinkHandle *>(link);
  if (!h) return nr_link_refuse("null link handle");
  if (h->soft_bits != 8) return nr_link_wrong_mode(h);
  return nr_link_recover(h, rx, 1, g, batch, rv, first_slot, combine, hip_stream);
}

int32_t ldpc_toolbox_nr_harq_slots_state_i8(void *link, int8_t *soft, uint8_t *done, uint8_t *rows, uint32_t first_slot, size_t batch) {
  g_last_error.clear();
  auto *h = static_cast<NrLinkHandle *>(link);
  if (!h) return nr_link_refuse("null link handle");
  if (soft && h->soft_bits != 8) return nr_link_wrong_mode(h);
  return nr_link_slot_state(h, soft, done, rows, first_slot, batch);
}

// ---- code tables and utilities ------------------------------------------------------------------------

size_t ldpc_toolbox_code_alist(const char *spec, char *buffer, size_t buffer_len) {
  if (!spec) return 0;
  ldpc::SparseMatrix h;
  if (!ldpc::codes::by_spec(spec, &h)) return 0;
  const std::string text = h.alist(true);
  if (buffer && buffer_len > text.size()) std::memcpy(buffer, text.c_str(), text.size() + 1);
  return text.size();
}

size_t ldpc_toolbox_alist_normalize(const char *alist, int32_t padding, char *buffer, size_t buffer_len) {
  g_last_error.clear();
  if (!alist) return 0;
  ldpc::SparseMatrix h;
  std::string err;
  if (!ldpc::SparseMatrix::from_alist(alist, &h, &err)) {
    set_error(err);
    return 0;
  }
  const std::string text = h.alist(padding != 0);
  if (buffer && buffer_len > text.size()) std::memcpy(buffer, text.c_str(), text.size() + 1);
  return text.size();
}

int32_t ldpc_toolbox_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return 0;
  return count;
}

const char *ldpc_toolbox_last_error(void) { return g_last_error.c_str(); }

}  // extern "C"
