// Host side of the batched NR mapper, demapper and scrambling (device_nr_qam.h): per-call tables, the cached Gold
// sequence and the launches.  Included by simulator.hip.
#pragma once
#include <algorithm>
#include <cstdio>
#include <memory>
#include <type_traits>
#include <vector>

#include "device_nr_qam.h"
#include "kernels_nr_qam.hip.h"

namespace ldpc {

bool DeviceNrQam::fail(const std::string &m, hipError_t e) {
  error_ = m;
  if (e != hipSuccess) error_ += std::string(": ") + hipGetErrorString(e);
  std::fprintf(stderr, "ldpc_toolbox (hip): NR modulation: %s\n", error_.c_str());
  return false;
}

#define NRQAM_TRY(expr)               \
  do {                                \
    hipError_t _e = (expr);           \
    if (_e != hipSuccess) {           \
      fail(#expr, _e);                \
      return -2;                      \
    }                                 \
  } while (0)

DeviceNrQam *DeviceNrQam::create(const nrqam::Config &c, int device, std::string *err) {
  auto bail = [&](const std::string &m) -> DeviceNrQam * {
    if (err) *err = m;
    return nullptr;
  };
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return bail("no HIP device available: the NR modulation has no CPU path");
  if (device < 0 || device >= count) return bail("HIP device index out of range");
  if (hipSetDevice(device) != hipSuccess) return bail("hipSetDevice failed");
  std::unique_ptr<DeviceNrQam> d(new DeviceNrQam());
  d->c_ = c;
  d->device_ = device;
  if (d->stream_.create() != hipSuccess || d->ev_default_.create() != hipSuccess || d->ev_gold_.create() != hipSuccess ||
      d->ev_gold_read_.create() != hipSuccess)
    return bail("creating the NR modulation's stream failed");
  return d.release();
}

// (the members free what they own, the stream last)
DeviceNrQam::~DeviceNrQam() {
  (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize(stream_);
}

namespace {
// the per-axis table of one call: the constants made in double, then each value rounded once to A
template <typename A>
nrqam::Axis<A> nr_qam_axis(const nrqam::Config &c, double scale) {
  nrqam::Axis<A> t;
  const double half_scale = 0.5 * scale;
  for (uint32_t u = 0; u < nrqam::kMaxLevels; u++) {
    t.amp[u] = static_cast<A>(c.amp[u]);
    t.k[u] = static_cast<A>(half_scale * (c.amp[u] * c.amp[u]));
  }
  return t;
}

// the table of the demappers with a scale per symbol: A_u and Q_u = A_u * A_u, made in double and rounded once to A
template <typename A>
nrqam::AxisCsi<A> nr_qam_axis_csi(const nrqam::Config &c) {
  nrqam::AxisCsi<A> t;
  for (uint32_t u = 0; u < nrqam::kMaxLevels; u++) {
    t.amp[u] = static_cast<A>(c.amp[u]);
    t.q[u] = static_cast<A>(c.amp[u] * c.amp[u]);
  }
  return t;
}

// passes of whole frames whose thread count fits a 31-bit grid: fn(first frame of the pass, its frames)
template <typename F>
void nr_qam_passes(size_t batch, size_t symbols_len, F fn) {
  const size_t pass = std::max<size_t>((uint64_t(0x7fffffffu) * nrqam::kThreads) / symbols_len, 1);
  for (size_t b0 = 0; b0 < batch; b0 += pass) fn(b0, std::min(pass, batch - b0));
}

inline uint32_t nr_qam_blocks(uint64_t total) { return static_cast<uint32_t>((total + nrqam::kThreads - 1) / nrqam::kThreads); }

template <int QM, typename T>
void nr_qam_map_pass(const uint8_t *bits, T *symbols, uint32_t symbols_len, uint64_t total, double a, const uint32_t *c, hipStream_t s) {
  nrqam::map_kernel<QM, T><<<nr_qam_blocks(total), nrqam::kThreads, 0, s>>>(bits, symbols, symbols_len, total, a, c);
}

template <typename T>
void nr_qam_map(const nrqam::Config &cfg, const uint8_t *bits, T *symbols, size_t symbols_len, size_t batch, const uint32_t *c,
                hipStream_t s) {
  const uint32_t sl = static_cast<uint32_t>(symbols_len);
  nr_qam_passes(batch, symbols_len, [&](size_t b0, size_t frames) {
    const uint64_t total = uint64_t(frames) * symbols_len;
    const uint8_t *in = bits + b0 * symbols_len * cfg.qm;
    T *out = symbols + 2 * b0 * symbols_len;
    switch (cfg.qm) {
      case 2: return nr_qam_map_pass<2, T>(in, out, sl, total, cfg.a, c, s);
      case 4: return nr_qam_map_pass<4, T>(in, out, sl, total, cfg.a, c, s);
      case 6: return nr_qam_map_pass<6, T>(in, out, sl, total, cfg.a, c, s);
      default: return nr_qam_map_pass<8, T>(in, out, sl, total, cfg.a, c, s);
    }
  });
}

template <int H, typename IO, typename A, bool MAXLOG>
void nr_qam_demap_pass(const nrqam::Config &cfg, const IO *symbols, IO *llrs, uint32_t symbols_len, uint64_t total, double scale,
                       const uint32_t *c, hipStream_t s) {
  nrqam::demap_kernel<H, IO, A, MAXLOG><<<nr_qam_blocks(total), nrqam::kThreads, 0, s>>>(symbols, llrs, symbols_len, total,
                                                                                        static_cast<A>(scale), c, nr_qam_axis<A>(cfg, scale));
}

template <typename IO, typename A, bool MAXLOG>
void nr_qam_demap_h(const nrqam::Config &cfg, const IO *symbols, IO *llrs, uint32_t symbols_len, uint64_t total, double scale,
                    const uint32_t *c, hipStream_t s) {
  switch (cfg.h()) {
    case 1: return nr_qam_demap_pass<1, IO, A, MAXLOG>(cfg, symbols, llrs, symbols_len, total, scale, c, s);
    case 2: return nr_qam_demap_pass<2, IO, A, MAXLOG>(cfg, symbols, llrs, symbols_len, total, scale, c, s);
    case 3: return nr_qam_demap_pass<3, IO, A, MAXLOG>(cfg, symbols, llrs, symbols_len, total, scale, c, s);
    default: return nr_qam_demap_pass<4, IO, A, MAXLOG>(cfg, symbols, llrs, symbols_len, total, scale, c, s);
  }
}

// exact: f64 arithmetic whatever the symbols' type; max-log: the symbols' type throughout
template <typename IO>
void nr_qam_demap(const nrqam::Config &cfg, const IO *symbols, IO *llrs, size_t symbols_len, size_t batch, double sigma, bool max_log,
                  const uint32_t *c, hipStream_t s) {
  const uint32_t sl = static_cast<uint32_t>(symbols_len);
  const double scale = 1.0 / (sigma * sigma);
  nr_qam_passes(batch, symbols_len, [&](size_t b0, size_t frames) {
    const uint64_t total = uint64_t(frames) * symbols_len;
    const IO *in = symbols + 2 * b0 * symbols_len;
    IO *out = llrs + b0 * symbols_len * cfg.qm;
    if (max_log)
      nr_qam_demap_h<IO, IO, true>(cfg, in, out, sl, total, scale, c, s);
    else
      nr_qam_demap_h<IO, double, false>(cfg, in, out, sl, total, scale, c, s);
  });
}

// the 8-bit demapper: exact = double arithmetic, max-log = float, as nr_qam_demap<float>; a pass's rows begin at a multiple
// of QM bytes from `llrs`, so the piece width follows from the address of each pass's first row
template <int H>
void nr_qam_demap_i8_pass(const nrqam::Config &cfg, const float *symbols, int8_t *llrs, uint32_t symbols_len, uint64_t total, double scale,
                          bool max_log, const uint32_t *c, hipStream_t s) {
  auto go = [&](auto wide) {
    constexpr bool kWide = decltype(wide)::value;
    if (max_log)
      nrqam::demap_i8_kernel<H, float, true, kWide><<<nr_qam_blocks(total), nrqam::kThreads, 0, s>>>(
          symbols, llrs, symbols_len, total, static_cast<float>(scale), c, nr_qam_axis<float>(cfg, scale));
    else
      nrqam::demap_i8_kernel<H, double, false, kWide><<<nr_qam_blocks(total), nrqam::kThreads, 0, s>>>(symbols, llrs, symbols_len, total, scale,
                                                                                                     c, nr_qam_axis<double>(cfg, scale));
  };
  if (reinterpret_cast<uintptr_t>(llrs) % 4 == 0)
    go(std::true_type{});
  else
    go(std::false_type{});
}

void nr_qam_demap_i8(const nrqam::Config &cfg, const float *symbols, int8_t *llrs, size_t symbols_len, size_t batch, double sigma,
                     bool max_log, const uint32_t *c, hipStream_t s) {
  const uint32_t sl = static_cast<uint32_t>(symbols_len);
  const double scale = 1.0 / (sigma * sigma);
  nr_qam_passes(batch, symbols_len, [&](size_t b0, size_t frames) {
    const uint64_t total = uint64_t(frames) * symbols_len;
    const float *in = symbols + 2 * b0 * symbols_len;
    int8_t *out = llrs + b0 * symbols_len * cfg.qm;
    switch (cfg.h()) {
      case 1: return nr_qam_demap_i8_pass<1>(cfg, in, out, sl, total, scale, max_log, c, s);
      case 2: return nr_qam_demap_i8_pass<2>(cfg, in, out, sl, total, scale, max_log, c, s);
      case 3: return nr_qam_demap_i8_pass<3>(cfg, in, out, sl, total, scale, max_log, c, s);
      default: return nr_qam_demap_i8_pass<4>(cfg, in, out, sl, total, scale, max_log, c, s);
    }
  });
}

// ---- the demappers with a scale per symbol (PART 10): scale [batch][symbols_len] beside the symbols ----

template <int H, typename IO, typename A, bool MAXLOG>
void nr_qam_demap_csi_pass(const nrqam::Config &cfg, const IO *symbols, const IO *scale, IO *llrs, uint32_t symbols_len, uint64_t total,
                           const uint32_t *c, hipStream_t s) {
  nrqam::demap_csi_kernel<H, IO, A, MAXLOG><<<nr_qam_blocks(total), nrqam::kThreads, 0, s>>>(symbols, scale, llrs, symbols_len, total, c,
                                                                                            nr_qam_axis_csi<A>(cfg));
}

template <typename IO, typename A, bool MAXLOG>
void nr_qam_demap_csi_h(const nrqam::Config &cfg, const IO *symbols, const IO *scale, IO *llrs, uint32_t symbols_len, uint64_t total,
                        const uint32_t *c, hipStream_t s) {
  switch (cfg.h()) {
    case 1: return nr_qam_demap_csi_pass<1, IO, A, MAXLOG>(cfg, symbols, scale, llrs, symbols_len, total, c, s);
    case 2: return nr_qam_demap_csi_pass<2, IO, A, MAXLOG>(cfg, symbols, scale, llrs, symbols_len, total, c, s);
    case 3: return nr_qam_demap_csi_pass<3, IO, A, MAXLOG>(cfg, symbols, scale, llrs, symbols_len, total, c, s);
    default: return nr_qam_demap_csi_pass<4, IO, A, MAXLOG>(cfg, symbols, scale, llrs, symbols_len, total, c, s);
  }
}

// the arithmetic types of nr_qam_demap
template <typename IO>
void nr_qam_demap_csi(const nrqam::Config &cfg, const IO *symbols, const IO *scale, IO *llrs, size_t symbols_len, size_t batch,
                      bool max_log, const uint32_t *c, hipStream_t s) {
  const uint32_t sl = static_cast<uint32_t>(symbols_len);
  nr_qam_passes(batch, symbols_len, [&](size_t b0, size_t frames) {
    const uint64_t total = uint64_t(frames) * symbols_len;
    const IO *in = symbols + 2 * b0 * symbols_len, *sc = scale + b0 * symbols_len;
    IO *out = llrs + b0 * symbols_len * cfg.qm;
    if (max_log)
      nr_qam_demap_csi_h<IO, IO, true>(cfg, in, sc, out, sl, total, c, s);
    else
      nr_qam_demap_csi_h<IO, double, false>(cfg, in, sc, out, sl, total, c, s);
  });
}

// the piece width from the address of each pass's first row, as in nr_qam_demap_i8_pass
template <int H>
void nr_qam_demap_csi_i8_pass(const nrqam::Config &cfg, const float *symbols, const float *scale, int8_t *llrs, uint32_t symbols_len,
                              uint64_t total, bool max_log, const uint32_t *c, hipStream_t s) {
  auto go = [&](auto wide) {
    constexpr bool kWide = decltype(wide)::value;
    if (max_log)
      nrqam::demap_csi_i8_kernel<H, float, true, kWide><<<nr_qam_blocks(total), nrqam::kThreads, 0, s>>>(symbols, scale, llrs, symbols_len, total,
                                                                                                        c, nr_qam_axis_csi<float>(cfg));
    else
      nrqam::demap_csi_i8_kernel<H, double, false, kWide><<<nr_qam_blocks(total), nrqam::kThreads, 0, s>>>(symbols, scale, llrs, symbols_len,
                                                                                                          total, c, nr_qam_axis_csi<double>(cfg));
  };
  if (reinterpret_cast<uintptr_t>(llrs) % 4 == 0)
    go(std::true_type{});
  else
    go(std::false_type{});
}

void nr_qam_demap_csi_i8(const nrqam::Config &cfg, const float *symbols, const float *scale, int8_t *llrs, size_t symbols_len, size_t batch,
                         bool max_log, const uint32_t *c, hipStream_t s) {
  const uint32_t sl = static_cast<uint32_t>(symbols_len);
  nr_qam_passes(batch, symbols_len, [&](size_t b0, size_t frames) {
    const uint64_t total = uint64_t(frames) * symbols_len;
    const float *in = symbols + 2 * b0 * symbols_len, *sc = scale + b0 * symbols_len;
    int8_t *out = llrs + b0 * symbols_len * cfg.qm;
    switch (cfg.h()) {
      case 1: return nr_qam_demap_csi_i8_pass<1>(cfg, in, sc, out, sl, total, max_log, c, s);
      case 2: return nr_qam_demap_csi_i8_pass<2>(cfg, in, sc, out, sl, total, max_log, c, s);
      case 3: return nr_qam_demap_csi_i8_pass<3>(cfg, in, sc, out, sl, total, max_log, c, s);
      default: return nr_qam_demap_csi_i8_pass<4>(cfg, in, sc, out, sl, total, max_log, c, s);
    }
  });
}

// fading_block != 0: the Rayleigh block-fading form, the table holding Q_u for the symbol's own scale
template <int H>
void nr_qam_generator_pass(const nrqam::Config &c, bool max_log, const uint8_t *tx, uint32_t pool, uint32_t n_tx, uint64_t seed,
                           uint64_t first_frame, uint64_t total, double sigma, uint32_t fading_block, float *llrs, hipStream_t s) {
  const double scale = 1.0 / (sigma * sigma);
  auto go = [&](auto ml, auto fading, const auto &t) {
    nrqam::qam_llr_kernel<H, decltype(ml)::value, decltype(fading)::value><<<nr_qam_blocks(total), nrqam::kThreads, 0, s>>>(
        tx, pool, n_tx, seed, first_frame, total, sigma, scale, c.a, t, llrs, fading_block);
  };
  if (fading_block != 0) {
    const nrqam::AxisCsi<double> t = nr_qam_axis_csi<double>(c);
    if (max_log)
      go(std::true_type{}, std::true_type{}, t);
    else
      go(std::false_type{}, std::true_type{}, t);
    return;
  }
  const nrqam::Axis<double> t = nr_qam_axis<double>(c, scale);
  if (max_log)
    go(std::true_type{}, std::false_type{}, t);
  else
    go(std::false_type{}, std::false_type{}, t);
}
}  // namespace

void nr_qam_launch_generator(const nrqam::Config &c, bool max_log, const uint8_t *tx, uint32_t pool, uint32_t n_tx, uint64_t seed,
                             uint64_t first_frame, uint32_t frames, double sigma, uint32_t fading_block, float *llrs, hipStream_t s) {
  const uint64_t total = uint64_t(frames) * (n_tx / c.qm);
  switch (c.h()) {
    case 1: return nr_qam_generator_pass<1>(c, max_log, tx, pool, n_tx, seed, first_frame, total, sigma, fading_block, llrs, s);
    case 2: return nr_qam_generator_pass<2>(c, max_log, tx, pool, n_tx, seed, first_frame, total, sigma, fading_block, llrs, s);
    case 3: return nr_qam_generator_pass<3>(c, max_log, tx, pool, n_tx, seed, first_frame, total, sigma, fading_block, llrs, s);
    default: return nr_qam_generator_pass<4>(c, max_log, tx, pool, n_tx, seed, first_frame, total, sigma, fading_block, llrs, s);
  }
}

namespace {
template <int H>
void nr_qam_harq_generator_pass(const nrqam::Config &c, bool max_log, const uint8_t *tx, uint32_t pool, uint32_t e, uint32_t first_symbol,
                                uint64_t seed, uint64_t first_frame, const uint64_t *frame_ids, uint64_t total, double sigma,
                                uint32_t fading_block, float *llrs, hipStream_t s) {
  const double scale = 1.0 / (sigma * sigma);
  auto go = [&](auto ml, auto fading, const auto &t) {
    nrqam::qam_llr_harq_kernel<H, decltype(ml)::value, decltype(fading)::value><<<nr_qam_blocks(total), nrqam::kThreads, 0, s>>>(
        tx, pool, e, first_symbol, seed, first_frame, frame_ids, total, sigma, scale, c.a, t, llrs, fading_block);
  };
  if (fading_block != 0) {
    const nrqam::AxisCsi<double> t = nr_qam_axis_csi<double>(c);
    if (max_log)
      go(std::true_type{}, std::true_type{}, t);
    else
      go(std::false_type{}, std::true_type{}, t);
    return;
  }
  const nrqam::Axis<double> t = nr_qam_axis<double>(c, scale);
  if (max_log)
    go(std::true_type{}, std::false_type{}, t);
  else
    go(std::false_type{}, std::false_type{}, t);
}
}  // namespace

void nr_qam_launch_harq_generator(const nrqam::Config &c, bool max_log, const uint8_t *tx, uint32_t pool, uint32_t e, uint32_t first_symbol,
                                  uint64_t seed, uint64_t first_frame, const uint64_t *frame_ids, uint32_t frames, double sigma,
                                  uint32_t fading_block, float *llrs, hipStream_t s) {
  const uint64_t total = uint64_t(frames) * (e / c.qm);
  switch (c.h()) {
    case 1:
      return nr_qam_harq_generator_pass<1>(c, max_log, tx, pool, e, first_symbol, seed, first_frame, frame_ids, total, sigma, fading_block, llrs, s);
    case 2:
      return nr_qam_harq_generator_pass<2>(c, max_log, tx, pool, e, first_symbol, seed, first_frame, frame_ids, total, sigma, fading_block, llrs, s);
    case 3:
      return nr_qam_harq_generator_pass<3>(c, max_log, tx, pool, e, first_symbol, seed, first_frame, frame_ids, total, sigma, fading_block, llrs, s);
    default:
      return nr_qam_harq_generator_pass<4>(c, max_log, tx, pool, e, first_symbol, seed, first_frame, frame_ids, total, sigma, fading_block, llrs, s);
  }
}

int DeviceNrQam::begin(hipStream_t stream, hipStream_t *s) {
  NRQAM_TRY(hipSetDevice(device_));
  *s = stream ? stream : static_cast<hipStream_t>(stream_);
  if (!stream) {
    // (the handle's stream is non-blocking: ordered explicitly after what the legacy default stream holds now)
    NRQAM_TRY(hipEventRecord(ev_default_, nullptr));
    NRQAM_TRY(hipStreamWaitEvent(*s, ev_default_, 0));
  }
  return 0;
}

int DeviceNrQam::end(hipStream_t stream, hipStream_t s, bool scrambled) {
  NRQAM_TRY(hipGetLastError());
  if (scrambled) {
    NRQAM_TRY(hipEventRecord(ev_gold_read_, s));
    gold_read_ = true;
    gold_read_stream_ = s;
  }
  if (!stream) NRQAM_TRY(hipStreamSynchronize(s));
  return 0;
}

int DeviceNrQam::sequence(int64_t c_init, size_t len, hipStream_t s, const uint32_t **c) {
  *c = nullptr;
  if (c_init < 0) return 0;
  if (gold_valid_ && gold_c_init_ == c_init && gold_len_ == len) {
    if (s != gold_stream_) NRQAM_TRY(hipStreamWaitEvent(s, ev_gold_, 0));
    // ev_gold_read_ moves to this reader: it goes behind the last one, so that the one event stays behind every reader
    // on whatever stream, and a later generation that waits for it overwrites words nobody reads any more
    if (gold_read_ && s != gold_read_stream_) NRQAM_TRY(hipStreamWaitEvent(s, ev_gold_read_, 0));
    *c = d_gold_.get<uint32_t>();
    return 0;
  }
  // one word beyond the last bit's: nrqam::gold_window reads two words
  const uint32_t words = static_cast<uint32_t>((len + 31) / 32 + 1);
  const uint32_t runs = (words + nrqam::kGoldRunWords - 1) / nrqam::kGoldRunWords;
  gold_valid_ = false;
  if (gold_read_) NRQAM_TRY(hipStreamWaitEvent(s, ev_gold_read_, 0));  // (launches that still read the words there now)
  NRQAM_TRY(d_gold_.ensure(size_t(words) * sizeof(uint32_t), 256));
  nrqam::gold_kernel<<<nr_qam_blocks(runs), nrqam::kThreads, 0, s>>>(static_cast<uint32_t>(c_init), words, runs, d_gold_.get<uint32_t>());
  NRQAM_TRY(hipGetLastError());
  NRQAM_TRY(hipEventRecord(ev_gold_, s));
  gold_stream_ = s;
  gold_c_init_ = c_init;
  gold_len_ = len;
  gold_valid_ = true;
  sequence_launches_++;
  *c = d_gold_.get<uint32_t>();
  return 0;
}

int DeviceNrQam::mod_device(const uint8_t *bits, void *symbols, bool f64, size_t bits_len, size_t symbols_len, size_t batch,
                            int64_t c_init, hipStream_t stream) {
  if (batch == 0 || bits_len == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const uint32_t *c;
  if (int rc = sequence(c_init, bits_len, s, &c)) return rc;
  if (f64)
    nr_qam_map(c_, bits, static_cast<double *>(symbols), symbols_len, batch, c, s);
  else
    nr_qam_map(c_, bits, static_cast<float *>(symbols), symbols_len, batch, c, s);
  return end(stream, s, c != nullptr);
}

int DeviceNrQam::demod_device(const void *symbols, void *llrs, bool f64, size_t symbols_len, size_t llrs_len, size_t batch, double sigma,
                              bool max_log, int64_t c_init, hipStream_t stream) {
  if (batch == 0 || llrs_len == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const uint32_t *c;
  if (int rc = sequence(c_init, llrs_len, s, &c)) return rc;
  if (f64)
    nr_qam_demap(c_, static_cast<const double *>(symbols), static_cast<double *>(llrs), symbols_len, batch, sigma, max_log, c, s);
  else
    nr_qam_demap(c_, static_cast<const float *>(symbols), static_cast<float *>(llrs), symbols_len, batch, sigma, max_log, c, s);
  return end(stream, s, c != nullptr);
}

int DeviceNrQam::demap_i8_device(const float *symbols, int8_t *llrs, size_t symbols_len, size_t llrs_len, size_t batch, double sigma,
                                 bool max_log, int64_t c_init, hipStream_t stream) {
  if (batch == 0 || llrs_len == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const uint32_t *c;
  if (int rc = sequence(c_init, llrs_len, s, &c)) return rc;
  nr_qam_demap_i8(c_, symbols, llrs, symbols_len, batch, sigma, max_log, c, s);
  return end(stream, s, c != nullptr);
}

int DeviceNrQam::demap_i8_host(const float *symbols, int8_t *llrs, size_t symbols_len, size_t llrs_len, size_t batch, double sigma,
                               bool max_log, int64_t c_init) {
  if (batch == 0 || llrs_len == 0) return 0;
  NRQAM_TRY(hipSetDevice(device_));
  const size_t in_bytes = batch * symbols_len * 2 * sizeof(float), out_bytes = batch * llrs_len;
  NRQAM_TRY(d_in_.ensure(in_bytes, 256));
  NRQAM_TRY(d_out_.ensure(out_bytes, 256));
  NRQAM_TRY(hipMemcpyAsync(d_in_.get(), symbols, in_bytes, hipMemcpyHostToDevice, stream_));
  if (int rc = demap_i8_device(d_in_.get<float>(), d_out_.get<int8_t>(), symbols_len, llrs_len, batch, sigma, max_log, c_init, stream_)) return rc;
  NRQAM_TRY(hipMemcpyAsync(llrs, d_out_.get(), out_bytes, hipMemcpyDeviceToHost, stream_));
  NRQAM_TRY(hipStreamSynchronize(stream_));
  return 0;
}

int DeviceNrQam::demap_csi_device(const void *symbols, const void *scale, void *llrs, bool f64, size_t symbols_len, size_t llrs_len,
                                  size_t batch, bool max_log, int64_t c_init, hipStream_t stream) {
  if (batch == 0 || llrs_len == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const uint32_t *c;
  if (int rc = sequence(c_init, llrs_len, s, &c)) return rc;
  if (f64)
    nr_qam_demap_csi(c_, static_cast<const double *>(symbols), static_cast<const double *>(scale), static_cast<double *>(llrs), symbols_len,
                     batch, max_log, c, s);
  else
    nr_qam_demap_csi(c_, static_cast<const float *>(symbols), static_cast<const float *>(scale), static_cast<float *>(llrs), symbols_len, batch,
                     max_log, c, s);
  return end(stream, s, c != nullptr);
}

int DeviceNrQam::demap_csi_i8_device(const float *symbols, const float *scale, int8_t *llrs, size_t symbols_len, size_t llrs_len, size_t batch,
                                     bool max_log, int64_t c_init, hipStream_t stream) {
  if (batch == 0 || llrs_len == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const uint32_t *c;
  if (int rc = sequence(c_init, llrs_len, s, &c)) return rc;
  nr_qam_demap_csi_i8(c_, symbols, scale, llrs, symbols_len, batch, max_log, c, s);
  return end(stream, s, c != nullptr);
}

// out_elem: the bytes of one LLR -- 8, 4, or 1 for the 8-bit form (float symbols)
int DeviceNrQam::demap_csi_host(const void *symbols, const void *scale, void *llrs, size_t out_elem, size_t symbols_len, size_t llrs_len,
                                size_t batch, bool max_log, int64_t c_init) {
  if (batch == 0 || llrs_len == 0) return 0;
  NRQAM_TRY(hipSetDevice(device_));
  const size_t elem = out_elem == 8 ? 8 : 4;
  const size_t in_bytes = batch * symbols_len * 2 * elem, scale_bytes = batch * symbols_len * elem, out_bytes = batch * llrs_len * out_elem;
  NRQAM_TRY(d_in_.ensure(in_bytes, 256));
  NRQAM_TRY(d_scale_.ensure(scale_bytes, 256));
  NRQAM_TRY(d_out_.ensure(out_bytes, 256));
  NRQAM_TRY(hipMemcpyAsync(d_in_.get(), symbols, in_bytes, hipMemcpyHostToDevice, stream_));
  NRQAM_TRY(hipMemcpyAsync(d_scale_.get(), scale, scale_bytes, hipMemcpyHostToDevice, stream_));
  const int rc = out_elem == 1 ? demap_csi_i8_device(d_in_.get<float>(), d_scale_.get<float>(), d_out_.get<int8_t>(), symbols_len, llrs_len,
                                                     batch, max_log, c_init, stream_)
                               : demap_csi_device(d_in_.get(), d_scale_.get(), d_out_.get(), out_elem == 8, symbols_len, llrs_len, batch,
                                                  max_log, c_init, stream_);
  if (rc) return rc;
  // (the only write to the caller's buffer: after an earlier failure nothing has been written)
  NRQAM_TRY(hipMemcpyAsync(llrs, d_out_.get(), out_bytes, hipMemcpyDeviceToHost, stream_));
  NRQAM_TRY(hipStreamSynchronize(stream_));
  return 0;
}

int DeviceNrQam::mod_host(const uint8_t *bits, void *symbols, bool f64, size_t bits_len, size_t symbols_len, size_t batch, int64_t c_init) {
  if (batch == 0 || bits_len == 0) return 0;
  NRQAM_TRY(hipSetDevice(device_));
  const size_t in_bytes = batch * bits_len, out_bytes = batch * symbols_len * 2 * (f64 ? 8 : 4);
  NRQAM_TRY(d_in_.ensure(in_bytes, 256));
  NRQAM_TRY(d_out_.ensure(out_bytes, 256));
  NRQAM_TRY(hipMemcpyAsync(d_in_.get(), bits, in_bytes, hipMemcpyHostToDevice, stream_));
  if (int rc = mod_device(d_in_.get<uint8_t>(), d_out_.get(), f64, bits_len, symbols_len, batch, c_init, stream_)) return rc;
  // (the only write to the caller's buffer: after an earlier failure nothing has been written)
  NRQAM_TRY(hipMemcpyAsync(symbols, d_out_.get(), out_bytes, hipMemcpyDeviceToHost, stream_));
  NRQAM_TRY(hipStreamSynchronize(stream_));
  return 0;
}

int DeviceNrQam::demod_host(const void *symbols, void *llrs, bool f64, size_t symbols_len, size_t llrs_len, size_t batch, double sigma,
                            bool max_log, int64_t c_init) {
  if (batch == 0 || llrs_len == 0) return 0;
  NRQAM_TRY(hipSetDevice(device_));
  const size_t elem = f64 ? 8 : 4;
  const size_t in_bytes = batch * symbols_len * 2 * elem, out_bytes = batch * llrs_len * elem;
  NRQAM_TRY(d_in_.ensure(in_bytes, 256));
  NRQAM_TRY(d_out_.ensure(out_bytes, 256));
  NRQAM_TRY(hipMemcpyAsync(d_in_.get(), symbols, in_bytes, hipMemcpyHostToDevice, stream_));
  if (int rc = demod_device(d_in_.get(), d_out_.get(), f64, symbols_len, llrs_len, batch, sigma, max_log, c_init, stream_)) return rc;
  NRQAM_TRY(hipMemcpyAsync(llrs, d_out_.get(), out_bytes, hipMemcpyDeviceToHost, stream_));
  NRQAM_TRY(hipStreamSynchronize(stream_));
  return 0;
}

int DeviceNrQam::sequence_host(uint8_t *out, size_t len, uint32_t c_init) {
  if (len == 0) return 0;
  NRQAM_TRY(hipSetDevice(device_));
  const uint32_t *c;
  if (int rc = sequence(c_init, len, stream_, &c)) return rc;
  std::vector<uint32_t> words((len + 31) / 32);
  NRQAM_TRY(hipMemcpyAsync(words.data(), c, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_));
  NRQAM_TRY(hipStreamSynchronize(stream_));
  for (size_t i = 0; i < len; i++) out[i] = static_cast<uint8_t>((words[i >> 5] >> (i & 31)) & 1u);
  return 0;
}

#undef NRQAM_TRY

}  // namespace ldpc
