// Host side of the batched soft demapper (demodulator.h): per-call tables and launches (stream protocol and staging loop:
// device_stage.h).
// Included by simulator.hip -- the demodulator shares the simulator's translation unit, as the batched encoder does.
#pragma once
#include <algorithm>
#include <memory>

#include "demodulator.h"
#include "kernels_channel.hip.h"
#include "kernels_demod.hip.h"

namespace ldpc {

DeviceDemodulator *DeviceDemodulator::create(const Constellation &c, int device, std::string *err) {
  if (!select_device(device, "the demodulator has", err)) return nullptr;
  std::unique_ptr<DeviceDemodulator> d(new DeviceDemodulator(device));
  d->c_ = c;
  if (!d->create_stream("the demodulator's", err)) return nullptr;
  return d.release();
}

// (the members free what they own, the stream last)
DeviceDemodulator::~DeviceDemodulator() { wait_idle(); }

namespace {
// one pass of a table constellation: frames * symbols_len threads
template <typename IO, typename A, bool MAXLOG>
void demod_table_pass_m(uint32_t bits, const IO *symbols, IO *llrs, uint32_t symbols_len, uint32_t llrs_len, uint64_t total,
                        double scale, int32_t interleaving, const Constellation &c, hipStream_t s) {
  demod::Table<A> t;
  const double half_scale = 0.5 * scale;
  for (uint32_t v = 0; v < 32; v++) {
    t.re[v] = static_cast<A>(c.re[v]);
    t.im[v] = static_cast<A>(c.im[v]);
    t.c[v] = static_cast<A>(half_scale * c.e[v]);
  }
  const uint32_t blocks = static_cast<uint32_t>((total + demod::kThreads - 1) / demod::kThreads);
  with_int<1, 2, 3, 4, 5>(static_cast<int>(bits), [&](auto m) {
    demod::table_kernel<decltype(m)::value, IO, A, MAXLOG><<<blocks, demod::kThreads, 0, s>>>(
        symbols, llrs, symbols_len, llrs_len, total, static_cast<A>(scale), interleaving, c.energy ? 1 : 0, t);
  });
}
}  // namespace

template <typename IO>
void DeviceDemodulator::launch(const IO *symbols, IO *llrs, size_t symbols_len, size_t llrs_len, size_t batch, double sigma,
                               int32_t interleaving, bool max_log, hipStream_t s) {
  // passes of whole frames whose thread count fits a 31-bit grid (symbols_len <= llrs_len < 2^31: at least 255 frames each)
  const size_t pass = std::max<size_t>((uint64_t(0x7fffffffu) * demod::kThreads) / symbols_len, 1);
  const size_t per_symbol = c_.bpsk ? 1 : 2;
  const uint32_t sl = static_cast<uint32_t>(symbols_len), ll = static_cast<uint32_t>(llrs_len);
  for (size_t b0 = 0; b0 < batch; b0 += pass) {
    const uint64_t total = uint64_t(std::min(pass, batch - b0)) * symbols_len;
    const IO *sym = symbols + b0 * symbols_len * per_symbol;
    IO *out = llrs + b0 * llrs_len;
    if (c_.bpsk) {
      const double scale = -2.0 / (sigma * sigma);
      const uint32_t blocks = static_cast<uint32_t>((total + demod::kThreads - 1) / demod::kThreads);
      demod::bpsk_kernel<IO><<<blocks, demod::kThreads, 0, s>>>(sym, out, ll, total, static_cast<IO>(scale), interleaving);
      continue;
    }
    const double scale = 1.0 / (sigma * sigma);
    if (!max_log)
      demod_table_pass_m<IO, double, false>(c_.bits, sym, out, sl, ll, total, scale, interleaving, c_, s);
    else
      demod_table_pass_m<IO, IO, true>(c_.bits, sym, out, sl, ll, total, scale, interleaving, c_, s);
  }
}

int DeviceDemodulator::run_device(const void *symbols, void *llrs, bool f64, size_t symbols_len, size_t llrs_len, size_t batch,
                                  double sigma, int32_t interleaving, bool max_log, hipStream_t stream) {
  if (batch == 0 || llrs_len == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  if (f64)
    launch(static_cast<const double *>(symbols), static_cast<double *>(llrs), symbols_len, llrs_len, batch, sigma, interleaving,
           max_log, s);
  else
    launch(static_cast<const float *>(symbols), static_cast<float *>(llrs), symbols_len, llrs_len, batch, sigma, interleaving,
           max_log, s);
  return end(stream, s);
}

int DeviceDemodulator::run_host(const void *symbols, void *llrs, bool f64, size_t symbols_len, size_t llrs_len, size_t batch,
                                double sigma, int32_t interleaving, bool max_log) {
  if (batch == 0 || llrs_len == 0) return 0;
  const size_t elem = f64 ? 8 : 4;
  return staged_rows(symbols, symbols_len * (c_.bpsk ? 1 : 2) * elem, llrs, llrs_len * elem, batch, batch, false, [&](size_t frames) {
    return run_device(d_in_.get(), d_out_.get(), f64, symbols_len, llrs_len, frames, sigma, interleaving, max_log, stream_);
  });
}

// ---- the transmit side: modulator and AWGN channel (kernels_channel.hip.h) ------------------------------------------

namespace {
// passes of whole frames whose thread count fits a 31-bit grid: fn(first frame of the pass, its frames)
template <typename F>
void channel_passes(size_t batch, size_t threads_per_frame, F fn) {
  const size_t pass = std::max<size_t>((uint64_t(0x7fffffffu) * chan::kThreads) / threads_per_frame, 1);
  for (size_t b0 = 0; b0 < batch; b0 += pass) fn(b0, std::min(pass, batch - b0));
}

inline uint32_t channel_blocks(uint64_t total) { return static_cast<uint32_t>((total + chan::kThreads - 1) / chan::kThreads); }

template <typename T>
void mod_launch(const Constellation &c, const uint8_t *bits, T *symbols, size_t bits_len, size_t symbols_len, size_t batch,
                int32_t interleaving, hipStream_t s) {
  const uint32_t bl = static_cast<uint32_t>(bits_len), sl = static_cast<uint32_t>(symbols_len);
  chan::Points<T> t;
  for (uint32_t v = 0; v < 32; v++) {  // (each coordinate rounded once to the symbols' type)
    t.re[v] = static_cast<T>(c.re[v]);
    t.im[v] = static_cast<T>(c.im[v]);
  }
  channel_passes(batch, symbols_len, [&](size_t b0, size_t frames) {
    const uint64_t total = uint64_t(frames) * symbols_len;
    if (c.bpsk)
      chan::bpsk_mod_kernel<T><<<channel_blocks(total), chan::kThreads, 0, s>>>(bits + b0 * bits_len, symbols + b0 * symbols_len,
                                                                               bl, total, interleaving);
    else
      chan::mod_kernel<T><<<channel_blocks(total), chan::kThreads, 0, s>>>(bits + b0 * bits_len, symbols + 2 * b0 * symbols_len,
                                                                          c.bits, sl, bl, total, interleaving, t);
  });
}

template <typename T>
void awgn_launch(const Constellation &c, T *symbols, size_t symbols_len, size_t batch, double sigma, uint64_t seed,
                 uint64_t first_frame, hipStream_t s) {
  const uint32_t sl = static_cast<uint32_t>(symbols_len), pairs = static_cast<uint32_t>((symbols_len + 1) / 2);
  const size_t per_frame = c.bpsk ? pairs : symbols_len;
  channel_passes(batch, per_frame, [&](size_t b0, size_t frames) {
    const uint64_t total = uint64_t(frames) * per_frame;
    if (c.bpsk)
      chan::awgn_real_kernel<T><<<channel_blocks(total), chan::kThreads, 0, s>>>(symbols + b0 * symbols_len, sl, pairs, total,
                                                                                static_cast<T>(sigma), seed, first_frame + b0);
    else
      chan::awgn_kernel<T><<<channel_blocks(total), chan::kThreads, 0, s>>>(symbols + 2 * b0 * symbols_len, sl, total,
                                                                           static_cast<T>(sigma), seed, first_frame + b0);
  });
}

template <typename T>
void fading_launch(T *symbols, T *scale, size_t symbols_len, size_t batch, double sigma, uint32_t block, uint64_t seed,
                   uint64_t first_frame, hipStream_t s) {
  const uint32_t sl = static_cast<uint32_t>(symbols_len);
  channel_passes(batch, symbols_len, [&](size_t b0, size_t frames) {
    const uint64_t total = uint64_t(frames) * symbols_len;
    chan::fading_kernel<T><<<channel_blocks(total), chan::kThreads, 0, s>>>(symbols + 2 * b0 * symbols_len, scale + b0 * symbols_len, sl,
                                                                           total, sigma, block, seed, first_frame + b0);
  });
}
}  // namespace

int DeviceDemodulator::mod_device(const uint8_t *bits, void *symbols, bool f64, size_t bits_len, size_t symbols_len, size_t batch,
                                  int32_t interleaving, hipStream_t stream) {
  if (batch == 0 || bits_len == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  if (f64)
    mod_launch(c_, bits, static_cast<double *>(symbols), bits_len, symbols_len, batch, interleaving, s);
  else
    mod_launch(c_, bits, static_cast<float *>(symbols), bits_len, symbols_len, batch, interleaving, s);
  return end(stream, s);
}

int DeviceDemodulator::mod_host(const uint8_t *bits, void *symbols, bool f64, size_t bits_len, size_t symbols_len, size_t batch,
                                int32_t interleaving) {
  if (batch == 0 || bits_len == 0) return 0;
  return staged_rows(bits, bits_len, symbols, symbols_len * (c_.bpsk ? 1 : 2) * (f64 ? 8 : 4), batch, batch, false, [&](size_t frames) {
    return mod_device(d_in_.get<uint8_t>(), d_out_.get(), f64, bits_len, symbols_len, frames, interleaving, stream_);
  });
}

int DeviceDemodulator::awgn_device(void *symbols, bool f64, size_t symbols_len, size_t batch, double sigma, uint64_t seed,
                                   uint64_t first_frame, hipStream_t stream) {
  if (batch == 0 || symbols_len == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  if (f64)
    awgn_launch(c_, static_cast<double *>(symbols), symbols_len, batch, sigma, seed, first_frame, s);
  else
    awgn_launch(c_, static_cast<float *>(symbols), symbols_len, batch, sigma, seed, first_frame, s);
  return end(stream, s);
}

// (in place: one buffer, copied in and out)
int DeviceDemodulator::awgn_host(void *symbols, bool f64, size_t symbols_len, size_t batch, double sigma, uint64_t seed,
                                 uint64_t first_frame) {
  if (batch == 0 || symbols_len == 0) return 0;
  const size_t row = symbols_len * (c_.bpsk ? 1 : 2) * (f64 ? 8 : 4), bytes = batch * row;
  return staged(batch, batch, {{d_in_, row}}, [&](size_t, size_t) {
    STAGE_TRY(hipMemcpyAsync(d_in_.get(), symbols, bytes, hipMemcpyHostToDevice, stream_));
    if (int rc = awgn_device(d_in_.get(), f64, symbols_len, batch, sigma, seed, first_frame, stream_)) return rc;
    STAGE_TRY(hipMemcpyAsync(symbols, d_in_.get(), bytes, hipMemcpyDeviceToHost, stream_));
    return 0;
  });
}

int DeviceDemodulator::fading_device(void *symbols, void *scale, bool f64, size_t symbols_len, size_t batch, double sigma, uint32_t block,
                                     uint64_t seed, uint64_t first_frame, hipStream_t stream) {
  if (batch == 0 || symbols_len == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  if (f64)
    fading_launch(static_cast<double *>(symbols), static_cast<double *>(scale), symbols_len, batch, sigma, block, seed, first_frame, s);
  else
    fading_launch(static_cast<float *>(symbols), static_cast<float *>(scale), symbols_len, batch, sigma, block, seed, first_frame, s);
  return end(stream, s);
}

int DeviceDemodulator::fading_host(void *symbols, void *scale, bool f64, size_t symbols_len, size_t batch, double sigma, uint32_t block,
                                   uint64_t seed, uint64_t first_frame) {
  if (batch == 0 || symbols_len == 0) return 0;
  const size_t scale_row = symbols_len * (f64 ? 8 : 4), scale_bytes = batch * scale_row, bytes = 2 * scale_bytes;
  return staged(batch, batch, {{d_in_, 2 * scale_row}, {d_out_, scale_row}}, [&](size_t, size_t) {
    STAGE_TRY(hipMemcpyAsync(d_in_.get(), symbols, bytes, hipMemcpyHostToDevice, stream_));
    if (int rc = fading_device(d_in_.get(), d_out_.get(), f64, symbols_len, batch, sigma, block, seed, first_frame, stream_)) return rc;
    STAGE_TRY(hipMemcpyAsync(symbols, d_in_.get(), bytes, hipMemcpyDeviceToHost, stream_));
    STAGE_TRY(hipMemcpyAsync(scale, d_out_.get(), scale_bytes, hipMemcpyDeviceToHost, stream_));
    return 0;
  });
}

}  // namespace ldpc
