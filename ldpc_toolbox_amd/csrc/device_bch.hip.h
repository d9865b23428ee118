// Host side of the batched BCH code (device_bch.h): tables and launches (stream protocol and staging loop: device_stage.h).
// Included by simulator.hip -- it shares the simulator's translation unit, as the batched encoder does.
#pragma once
#include <algorithm>
#include <memory>

#include "device_bch.h"
#include "kernels_bch.hip.h"

namespace ldpc {

DeviceBch *DeviceBch::create(const bch::Code &c, int device, std::string *err) {
  auto bail = [&](const std::string &m) -> DeviceBch * {
    if (err) *err = m;
    return nullptr;
  };
  if (!select_device(device, "the BCH code has", err)) return nullptr;
  std::unique_ptr<DeviceBch> d(new DeviceBch(device));
  d->c_ = c;
  d->enc_geo_ = bch::geometry(c.k);
  d->dec_geo_ = bch::geometry(c.n);
  if (d->dec_geo_.staged_words > bch::kMaxStagedWords || d->dec_geo_.lanes > bch::kThreads)
    return bail("frame too long for the BCH kernels");
  bch::generator_top(c, d->g_top_);
  if (!d->create_stream("the BCH handle's", err)) return nullptr;
  hipError_t e = hipSuccess;
  auto up = [&](DeviceBuffer &b, const auto &v) {
    if (e == hipSuccess) b = upload(v, &e);
  };
  up(d->d_antilog_, c.antilog);
  up(d->d_log_, c.log);
  up(d->d_enc_table_, bch::remainder_table(c, d->enc_geo_));
  up(d->d_dec_table_, bch::remainder_table(c, d->dec_geo_));
  if (e == hipSuccess) e = d->d_list_.ensure(kBchPassFrames * sizeof(uint32_t));
  if (e == hipSuccess) e = d->d_count_.ensure(64);
  if (e == hipSuccess) e = d->d_synd_.ensure(kBchPassFrames * bch::kMaxT * sizeof(uint16_t));
  if (e == hipSuccess) e = d->d_loc_.ensure(kBchPassFrames * bch::kLocWords * sizeof(uint16_t));
  if (e != hipSuccess) return bail(std::string("device allocation for the BCH code failed: ") + hipGetErrorString(e));
  return d.release();
}

// (the members free what they own, the stream last)
DeviceBch::~DeviceBch() { wait_idle(); }

namespace {
template <bool DECODE>
void bch_remainder_pass_nw(uint32_t nw, const uint8_t *in, uint8_t *out, uint32_t frames, uint32_t copy_len, uint32_t out_stride,
                           uint32_t parity, const bch::Geometry &geo, const uint32_t *g_top, const uint32_t *table,
                           const bch::DecodeArgs &d, hipStream_t s) {
  with_int<1, 2, 3, 4, 5, 6>(static_cast<int>(nw), [&](auto words) {
    constexpr int NW = decltype(words)::value;
    bch::GeneratorTop<NW> top;
    for (int w = 0; w < NW; w++) top.w[w] = g_top[w];
    bch::remainder_kernel<NW, DECODE><<<frames, bch::kThreads, 0, s>>>(in, out, copy_len, out_stride, parity, geo, top, table, d);
  });
}
}  // namespace

int DeviceBch::encode_device(const uint8_t *input, uint8_t *output, size_t batch, hipStream_t stream) {
  if (batch == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const bch::DecodeArgs none{};
  for (size_t b0 = 0; b0 < batch; b0 += kBchPassFrames) {
    const uint32_t frames = static_cast<uint32_t>(std::min(kBchPassFrames, batch - b0));
    bch_remainder_pass_nw<false>(c_.parity_words(), input + b0 * c_.k, output + b0 * c_.n, frames, c_.k, c_.n, c_.parity, enc_geo_,
                                 g_top_, d_enc_table_.get<uint32_t>(), none, s);
  }
  return end(stream, s);
}

int DeviceBch::decode_device(const uint8_t *input, uint8_t *output, size_t output_len, size_t batch, int32_t *errors,
                             hipStream_t stream) {
  if (batch == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const uint32_t out_len = static_cast<uint32_t>(output_len);
  for (size_t b0 = 0; b0 < batch; b0 += kBchPassFrames) {
    const uint32_t frames = static_cast<uint32_t>(std::min(kBchPassFrames, batch - b0));
    uint8_t *out = output + b0 * output_len;
    int32_t *err = errors ? errors + b0 : nullptr;
    STAGE_TRY(hipMemsetAsync(d_count_.get(), 0, sizeof(uint32_t), s));
    const bch::DecodeArgs d{c_.m, c_.t, d_antilog_.get<uint16_t>(), err, d_list_.get<uint32_t>(), d_count_.get<uint32_t>(),
                            d_synd_.get<uint16_t>()};
    bch_remainder_pass_nw<true>(c_.parity_words(), input + b0 * c_.n, out, frames, out_len, out_len, c_.parity, dec_geo_, g_top_,
                                d_dec_table_.get<uint32_t>(), d, s);
    // (the list's length stays on the device: a lane or a workgroup past it returns at once)
    bch::locator_kernel<<<(frames + 63) / 64, 64, 0, s>>>(d_synd_.get<uint16_t>(), d_count_.get<uint32_t>(), d_log_.get<uint16_t>(),
                                                          d_loc_.get<uint16_t>(), c_.t, c_.poly, c_.m);
    bch::chien_kernel<<<frames, bch::kThreads, 0, s>>>(out, out_len, c_.n, c_.t, c_.m, d_antilog_.get<uint16_t>(),
                                                      d_list_.get<uint32_t>(), d_count_.get<uint32_t>(), d_loc_.get<uint16_t>(), err);
  }
  return end(stream, s);
}

// frames of a host call that are staged on the device at a time
size_t DeviceBch::stage_frames() const { return std::max<size_t>(std::min(kBchStageFrames, kBchStageBytes / c_.n), 1); }

int DeviceBch::encode_host(const uint8_t *input, uint8_t *output, size_t batch) {
  if (batch == 0) return 0;
  return staged_rows(input, c_.k, output, c_.n, batch, std::min(batch, stage_frames()), false, [&](size_t frames) {
    return encode_device(d_in_.get<uint8_t>(), d_out_.get<uint8_t>(), frames, stream_);
  });
}

int DeviceBch::decode_host(const uint8_t *input, uint8_t *output, size_t output_len, size_t batch, int32_t *errors) {
  if (batch == 0) return 0;
  const size_t stage = std::min(batch, stage_frames());
  return staged(batch, stage, {{d_in_, c_.n}, {d_out_, output_len}, {d_err_, errors ? sizeof(int32_t) : 0}}, [&](size_t b0, size_t frames) {
    STAGE_TRY(hipMemcpyAsync(d_in_.get(), input + b0 * c_.n, frames * c_.n, hipMemcpyHostToDevice, stream_));
    if (int rc = decode_device(d_in_.get<uint8_t>(), d_out_.get<uint8_t>(), output_len, frames,
                               errors ? d_err_.get<int32_t>() : nullptr, stream_))
      return rc;
    STAGE_TRY(hipMemcpyAsync(output + b0 * output_len, d_out_.get(), frames * output_len, hipMemcpyDeviceToHost, stream_));
    if (errors) STAGE_TRY(hipMemcpyAsync(errors + b0, d_err_.get(), frames * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    return 0;
  });
}

}  // namespace ldpc
