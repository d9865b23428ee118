// Host side of the batched NR mapper, demapper and scrambling (device_nr_qam.h): per-call tables, the cached Gold
// sequence and the launches; the entries' stream protocol and staging are device_stage.h's.  Included by simulator.hip.
#pragma once
#include <algorithm>
#include <memory>
#include <type_traits>
#include <vector>

#include "device_nr_qam.h"
#include "kernels_nr_qam.hip.h"

namespace ldpc {

DeviceNrQam *DeviceNrQam::create(const nrqam::Config &c, int device, std::string *err) {
  if (!select_device(device, "the NR modulation has", err)) return nullptr;
  std::unique_ptr<DeviceNrQam> d(new DeviceNrQam(device));
  d->c_ = c;
  if (!d->create_stream("the NR modulation's", err, {&d->ev_gold_, &d->ev_gold_read_})) return nullptr;
  return d.release();
}

// (the members free what they own, the stream last)
DeviceNrQam::~DeviceNrQam() { wait_idle(); }

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

template <typename T>
void nr_qam_map(const nrqam::Config &cfg, const uint8_t *bits, T *symbols, size_t symbols_len, size_t batch, const uint32_t *c,
                hipStream_t s) {
  const uint32_t sl = static_cast<uint32_t>(symbols_len);
  nr_qam_passes(batch, symbols_len, [&](size_t b0, size_t frames) {
    const uint64_t total = uint64_t(frames) * symbols_len;
    const uint8_t *in = bits + b0 * symbols_len * cfg.qm;
    T *out = symbols + 2 * b0 * symbols_len;
    with_int<2, 4, 6, 8>(static_cast<int>(cfg.qm), [&](auto qm) {
      nrqam::map_kernel<decltype(qm)::value, T><<<nr_qam_blocks(total), nrqam::kThreads, 0, s>>>(in, out, sl, total, cfg.a, c);
    });
  });
}

// The four demappers in one.  OUT: rows in the symbols' type IO, or int8_t for 8-bit soft bits (float symbols).  CSI: a
// scale per symbol, scales [batch][symbols_len], with the AxisCsi table (PART 10); else one scale 1 / sigma^2 per call with
// the Axis table.  Arithmetic: exact = double whatever the symbols' type; max-log = the symbols' type (float for soft
// bits).  A pass's rows begin at a multiple of QM bytes from `llrs`, so the piece width of the soft bits follows from the
// address of each pass's first row.
template <bool CSI, typename IO, typename OUT>
void nr_qam_demap(const nrqam::Config &cfg, const IO *symbols, const IO *scales, double sigma, OUT *llrs, size_t symbols_len, size_t batch,
                  bool max_log, const uint32_t *c, hipStream_t s) {
  constexpr bool kSoft = std::is_same<OUT, int8_t>::value;
  const uint32_t sl = static_cast<uint32_t>(symbols_len);
  const double scale = CSI ? 0.0 : 1.0 / (sigma * sigma);
  nr_qam_passes(batch, symbols_len, [&](size_t b0, size_t frames) {
    const uint64_t total = uint64_t(frames) * symbols_len;
    const IO *in = symbols + 2 * b0 * symbols_len, *sc = CSI ? scales + b0 * symbols_len : nullptr;
    OUT *out = llrs + b0 * symbols_len * cfg.qm;
    const bool wide = kSoft && reinterpret_cast<uintptr_t>(out) % 4 == 0;
    with_int<1, 2, 3, 4>(static_cast<int>(cfg.h()), [&](auto h) {
      with_bool(max_log, [&](auto ml) {
        with_bool(wide, [&](auto w) {
          constexpr int H = decltype(h)::value;
          constexpr bool MAXLOG = decltype(ml)::value, WIDE = decltype(w)::value;
          using A = std::conditional_t<MAXLOG, IO, double>;
          const dim3 grid(nr_qam_blocks(total)), block(nrqam::kThreads);
          if constexpr (CSI && kSoft)
            nrqam::demap_csi_i8_kernel<H, A, MAXLOG, WIDE><<<grid, block, 0, s>>>(in, sc, out, sl, total, c, nr_qam_axis_csi<A>(cfg));
          else if constexpr (CSI)
            nrqam::demap_csi_kernel<H, IO, A, MAXLOG><<<grid, block, 0, s>>>(in, sc, out, sl, total, c, nr_qam_axis_csi<A>(cfg));
          else if constexpr (kSoft)
            nrqam::demap_i8_kernel<H, A, MAXLOG, WIDE><<<grid, block, 0, s>>>(in, out, sl, total, static_cast<A>(scale), c, nr_qam_axis<A>(cfg, scale));
          else
            nrqam::demap_kernel<H, IO, A, MAXLOG><<<grid, block, 0, s>>>(in, out, sl, total, static_cast<A>(scale), c, nr_qam_axis<A>(cfg, scale));
        });
      });
    });
  });
}

// One launch of a generator: qam_llr_kernel over rows of `row` = n_tx bits, or (HARQ) qam_llr_harq_kernel over one
// transmission's rows of `row` = e bits, with its first symbol and frame list.  fading_block != 0: the Rayleigh
// block-fading form, the table holding Q_u for the symbol's own scale.
template <bool HARQ>
void nr_qam_generator(const nrqam::Config &c, bool max_log, const uint8_t *tx, uint32_t pool, uint32_t row, uint32_t first_symbol,
                      uint64_t seed, uint64_t first_frame, const uint64_t *frame_ids, uint32_t frames, double sigma, uint32_t fading_block,
                      float *llrs, hipStream_t s) {
  const uint64_t total = uint64_t(frames) * (row / c.qm);
  const double scale = 1.0 / (sigma * sigma);
  with_int<1, 2, 3, 4>(static_cast<int>(c.h()), [&](auto h) {
    with_bool(max_log, [&](auto ml) {
      with_bool(fading_block != 0, [&](auto fading) {
        constexpr int H = decltype(h)::value;
        constexpr bool MAXLOG = decltype(ml)::value, FADING = decltype(fading)::value;
        typename nrqam::GeneratorAxis<FADING>::type t;
        if constexpr (FADING)
          t = nr_qam_axis_csi<double>(c);
        else
          t = nr_qam_axis<double>(c, scale);
        if constexpr (HARQ)
          nrqam::qam_llr_harq_kernel<H, MAXLOG, FADING><<<nr_qam_blocks(total), nrqam::kThreads, 0, s>>>(
              tx, pool, row, first_symbol, seed, first_frame, frame_ids, total, sigma, scale, c.a, t, llrs, fading_block);
        else
          nrqam::qam_llr_kernel<H, MAXLOG, FADING><<<nr_qam_blocks(total), nrqam::kThreads, 0, s>>>(tx, pool, row, seed, first_frame, total, sigma,
                                                                                                  scale, c.a, t, llrs, fading_block);
      });
    });
  });
}
}  // namespace

void nr_qam_launch_generator(const nrqam::Config &c, bool max_log, const uint8_t *tx, uint32_t pool, uint32_t n_tx, uint64_t seed,
                             uint64_t first_frame, uint32_t frames, double sigma, uint32_t fading_block, float *llrs, hipStream_t s) {
  nr_qam_generator<false>(c, max_log, tx, pool, n_tx, 0, seed, first_frame, nullptr, frames, sigma, fading_block, llrs, s);
}

void nr_qam_launch_harq_generator(const nrqam::Config &c, bool max_log, const uint8_t *tx, uint32_t pool, uint32_t e, uint32_t first_symbol,
                                  uint64_t seed, uint64_t first_frame, const uint64_t *frame_ids, uint32_t frames, double sigma,
                                  uint32_t fading_block, float *llrs, hipStream_t s) {
  nr_qam_generator<true>(c, max_log, tx, pool, e, first_symbol, seed, first_frame, frame_ids, frames, sigma, fading_block, llrs, s);
}

// DeviceStage::end with one step between its two: the launches that read the sequence get ev_gold_read_ behind them
int DeviceNrQam::end(hipStream_t stream, hipStream_t s, bool scrambled) {
  if (!scrambled) return DeviceStage::end(stream, s);
  STAGE_TRY(hipGetLastError());
  STAGE_TRY(hipEventRecord(ev_gold_read_, s));
  gold_read_ = true;
  gold_read_stream_ = s;
  return finish(stream, s);
}

int DeviceNrQam::sequence(int64_t c_init, size_t len, hipStream_t s, const uint32_t **c) {
  *c = nullptr;
  if (c_init < 0) return 0;
  if (gold_valid_ && gold_c_init_ == c_init && gold_len_ == len) {
    if (s != gold_stream_) STAGE_TRY(hipStreamWaitEvent(s, ev_gold_, 0));
    // ev_gold_read_ moves to this reader: it goes behind the last one, so that the one event stays behind every reader
    // on whatever stream, and a later generation that waits for it overwrites words nobody reads any more
    if (gold_read_ && s != gold_read_stream_) STAGE_TRY(hipStreamWaitEvent(s, ev_gold_read_, 0));
    *c = d_gold_.get<uint32_t>();
    return 0;
  }
  // one word beyond the last bit's: nrqam::gold_window reads two words
  const uint32_t words = static_cast<uint32_t>((len + 31) / 32 + 1);
  const uint32_t runs = (words + nrqam::kGoldRunWords - 1) / nrqam::kGoldRunWords;
  gold_valid_ = false;
  if (gold_read_) STAGE_TRY(hipStreamWaitEvent(s, ev_gold_read_, 0));  // (launches that still read the words there now)
  STAGE_TRY(d_gold_.ensure(size_t(words) * sizeof(uint32_t), 256));
  nrqam::gold_kernel<<<nr_qam_blocks(runs), nrqam::kThreads, 0, s>>>(static_cast<uint32_t>(c_init), words, runs, d_gold_.get<uint32_t>());
  STAGE_TRY(hipGetLastError());
  STAGE_TRY(hipEventRecord(ev_gold_, s));
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
    nr_qam_demap<false, double>(c_, static_cast<const double *>(symbols), nullptr, sigma, static_cast<double *>(llrs), symbols_len, batch,
                                max_log, c, s);
  else
    nr_qam_demap<false, float>(c_, static_cast<const float *>(symbols), nullptr, sigma, static_cast<float *>(llrs), symbols_len, batch, max_log,
                               c, s);
  return end(stream, s, c != nullptr);
}

int DeviceNrQam::demap_i8_device(const float *symbols, int8_t *llrs, size_t symbols_len, size_t llrs_len, size_t batch, double sigma,
                                 bool max_log, int64_t c_init, hipStream_t stream) {
  if (batch == 0 || llrs_len == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const uint32_t *c;
  if (int rc = sequence(c_init, llrs_len, s, &c)) return rc;
  nr_qam_demap<false, float>(c_, symbols, nullptr, sigma, llrs, symbols_len, batch, max_log, c, s);
  return end(stream, s, c != nullptr);
}

int DeviceNrQam::demap_csi_device(const void *symbols, const void *scale, void *llrs, bool f64, size_t symbols_len, size_t llrs_len,
                                  size_t batch, bool max_log, int64_t c_init, hipStream_t stream) {
  if (batch == 0 || llrs_len == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const uint32_t *c;
  if (int rc = sequence(c_init, llrs_len, s, &c)) return rc;
  if (f64)
    nr_qam_demap<true, double>(c_, static_cast<const double *>(symbols), static_cast<const double *>(scale), 0.0, static_cast<double *>(llrs),
                               symbols_len, batch, max_log, c, s);
  else
    nr_qam_demap<true, float>(c_, static_cast<const float *>(symbols), static_cast<const float *>(scale), 0.0, static_cast<float *>(llrs),
                              symbols_len, batch, max_log, c, s);
  return end(stream, s, c != nullptr);
}

int DeviceNrQam::demap_csi_i8_device(const float *symbols, const float *scale, int8_t *llrs, size_t symbols_len, size_t llrs_len, size_t batch,
                                     bool max_log, int64_t c_init, hipStream_t stream) {
  if (batch == 0 || llrs_len == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const uint32_t *c;
  if (int rc = sequence(c_init, llrs_len, s, &c)) return rc;
  nr_qam_demap<true, float>(c_, symbols, scale, 0.0, llrs, symbols_len, batch, max_log, c, s);
  return end(stream, s, c != nullptr);
}

// The host entries stage the whole batch at once.

int DeviceNrQam::mod_host(const uint8_t *bits, void *symbols, bool f64, size_t bits_len, size_t symbols_len, size_t batch, int64_t c_init) {
  if (batch == 0 || bits_len == 0) return 0;
  return staged_rows(bits, bits_len, symbols, symbols_len * 2 * (f64 ? 8 : 4), batch, batch, false, [&](size_t frames) {
    return mod_device(d_in_.get<uint8_t>(), d_out_.get(), f64, bits_len, symbols_len, frames, c_init, stream_);
  });
}

int DeviceNrQam::demod_host(const void *symbols, void *llrs, bool f64, size_t symbols_len, size_t llrs_len, size_t batch, double sigma,
                            bool max_log, int64_t c_init) {
  if (batch == 0 || llrs_len == 0) return 0;
  const size_t elem = f64 ? 8 : 4;
  return staged_rows(symbols, symbols_len * 2 * elem, llrs, llrs_len * elem, batch, batch, false, [&](size_t frames) {
    return demod_device(d_in_.get(), d_out_.get(), f64, symbols_len, llrs_len, frames, sigma, max_log, c_init, stream_);
  });
}

int DeviceNrQam::demap_i8_host(const float *symbols, int8_t *llrs, size_t symbols_len, size_t llrs_len, size_t batch, double sigma,
                               bool max_log, int64_t c_init) {
  if (batch == 0 || llrs_len == 0) return 0;
  return staged_rows(symbols, symbols_len * 2 * sizeof(float), llrs, llrs_len, batch, batch, false, [&](size_t frames) {
    return demap_i8_device(d_in_.get<float>(), d_out_.get<int8_t>(), symbols_len, llrs_len, frames, sigma, max_log, c_init, stream_);
  });
}

// out_elem: the bytes of one LLR -- 8, 4, or 1 for the 8-bit form (float symbols)
int DeviceNrQam::demap_csi_host(const void *symbols, const void *scale, void *llrs, size_t out_elem, size_t symbols_len, size_t llrs_len,
                                size_t batch, bool max_log, int64_t c_init) {
  if (batch == 0 || llrs_len == 0) return 0;
  const size_t elem = out_elem == 8 ? 8 : 4;
  const size_t in_row = symbols_len * 2 * elem, scale_row = symbols_len * elem, out_row = llrs_len * out_elem;
  return staged(batch, batch, {{d_in_, in_row}, {d_scale_, scale_row}, {d_out_, out_row}}, [&](size_t, size_t) {
    STAGE_TRY(hipMemcpyAsync(d_in_.get(), symbols, batch * in_row, hipMemcpyHostToDevice, stream_));
    STAGE_TRY(hipMemcpyAsync(d_scale_.get(), scale, batch * scale_row, hipMemcpyHostToDevice, stream_));
    const int rc = out_elem == 1 ? demap_csi_i8_device(d_in_.get<float>(), d_scale_.get<float>(), d_out_.get<int8_t>(), symbols_len, llrs_len,
                                                       batch, max_log, c_init, stream_)
                                 : demap_csi_device(d_in_.get(), d_scale_.get(), d_out_.get(), out_elem == 8, symbols_len, llrs_len, batch,
                                                    max_log, c_init, stream_);
    if (rc) return rc;
    // (the only write to the caller's buffer: after an earlier failure nothing has been written)
    STAGE_TRY(hipMemcpyAsync(llrs, d_out_.get(), batch * out_row, hipMemcpyDeviceToHost, stream_));
    return 0;
  });
}

int DeviceNrQam::sequence_host(uint8_t *out, size_t len, uint32_t c_init) {
  if (len == 0) return 0;
  STAGE_TRY(hipSetDevice(device_));
  const uint32_t *c;
  if (int rc = sequence(c_init, len, stream_, &c)) return rc;
  std::vector<uint32_t> words((len + 31) / 32);
  STAGE_TRY(hipMemcpyAsync(words.data(), c, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_));
  STAGE_TRY(hipStreamSynchronize(stream_));
  for (size_t i = 0; i < len; i++) out[i] = static_cast<uint8_t>((words[i >> 5] >> (i & 31)) & 1u);
  return 0;
}

}  // namespace ldpc
