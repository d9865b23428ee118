// Host side of the batched GPU encoder (device_encoder.h): tables, work buffers and launches (stream protocol and staging
// loop: device_stage.h).
// Included by simulator.hip -- the encoder shares the simulator's translation unit.
#pragma once
#include <algorithm>
#include <memory>

#include "device_encoder.h"
#include "kernels_encoder.hip.h"

namespace ldpc {

namespace {
// frames per pass of the staircase kernels (bounds the bit-packed work buffers: n / 8 bytes per frame)
constexpr size_t kEncPassFrames = 4096;
}  // namespace

DeviceEncoder *DeviceEncoder::create(const Encoder &enc, const std::vector<uint8_t> &pattern, int device, std::string *err) {
  auto bail = [&](const std::string &m) -> DeviceEncoder * {
    if (err) *err = m;
    return nullptr;
  };
  if (!select_device(device, "the batched encoder has", err)) return nullptr;
  const size_t n = enc.n(), k = enc.k(), m = n - k;
  if (n == 0 || n > 0x7fffffffu) return bail("codeword length out of range for the batched encoder");
  if (!pattern.empty() && n % pattern.size() != 0) return bail("the puncturing pattern does not divide the codeword length");
  std::unique_ptr<DeviceEncoder> d(new DeviceEncoder(device));
  d->k_ = k;
  d->n_ = n;
  d->m_ = m;
  d->out_len_ = n;
  d->staircase_ = enc.staircase();
  auto up = [](const auto &v, DeviceBuffer *dst) {
    hipError_t e;
    *dst = upload(v, &e, 256);
    return e == hipSuccess;
  };
  bool ok = true;
  if (d->staircase_) {
    ok = up(enc.h0_ptr(), &d->d_h0_ptr_) && up(enc.h0_idx(), &d->d_h0_idx_);
  } else {
    // G0 transposed: [word][row], rows padded with zeros to a multiple of 64
    d->words_ = enc.words();
    d->m_pad_ = (m + 63) / 64 * 64;
    std::vector<uint64_t> gt(d->words_ * d->m_pad_, 0);
    const std::vector<uint64_t> &gen = enc.gen();
    for (size_t r = 0; r < m; r++)
      for (size_t w = 0; w < d->words_; w++) gt[w * d->m_pad_ + r] = gen[r * d->words_ + w];
    ok = up(gt, &d->d_gen_t_);
  }
  if (ok && !pattern.empty()) {
    std::vector<uint32_t> keep;
    for (size_t b = 0; b < pattern.size(); b++)
      if (pattern[b]) keep.push_back(static_cast<uint32_t>(b));
    d->block_ = static_cast<uint32_t>(n / pattern.size());
    d->kept_ = static_cast<uint32_t>(keep.size());
    d->out_len_ = size_t(d->block_) * d->kept_;
    ok = up(keep, &d->d_keep_);
  }
  ok = ok && d->create_stream() == hipSuccess;
  if (!ok) return bail("device allocation / upload of the encoder tables failed");
  return d.release();
}

// (the members free what they own, the stream last)
DeviceEncoder::~DeviceEncoder() { wait_idle(); }

int DeviceEncoder::grow(DeviceBuffer &b, size_t need) {
  STAGE_TRY(b.ensure(need, 256));
  return 0;
}

// one pass (at most kEncPassFrames frames) of a staircase code: in [batch][k] -> cw [batch][n]
template <typename W, bool STAGE>
static void enc_staircase_pass(const uint8_t *in, uint8_t *cw, uint32_t batch, uint32_t k, uint32_t n, uint32_t kp, void *packed,
                               void *prefix, const uint32_t *h0_ptr, const uint32_t *h0_idx, hipStream_t s) {
  constexpr uint32_t F = 8 * sizeof(W);
  const uint32_t m = n - k, groups = (batch + F - 1) / F;
  // slices of rows: enough workgroups to fill the chip at a small batch, never less than one chunk of rows each
  uint32_t slices = std::min<uint32_t>(std::max<uint32_t>((512 + groups - 1) / groups, 1), 8);
  const uint32_t slice_rows = ((m + slices - 1) / slices + enc::kScanThreads - 1) / enc::kScanThreads * enc::kScanThreads;
  slices = (m + slice_rows - 1) / slice_rows;
  W *pk = static_cast<W *>(packed), *pre = static_cast<W *>(prefix), *tot = pre + size_t(groups) * m;
  const bool aligned = k % 8 == 0 && n % 8 == 0 && (reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(cw)) % 8 == 0;
  if (k > 0) {
    const dim3 grid((k + enc::kPackCols - 1) / enc::kPackCols, groups);
    if (aligned)
      enc::pack_frames_kernel<W, true><<<grid, 256, 0, s>>>(in, cw, pk, k, n, kp, batch);
    else
      enc::pack_frames_kernel<W, false><<<grid, 256, 0, s>>>(in, cw, pk, k, n, kp, batch);
  }
  const size_t lds = STAGE ? size_t(kp) * sizeof(W) : 0;
  auto scan = enc::stair_scan_kernel<W, STAGE>;
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(scan), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
  scan<<<dim3(slices, groups), enc::kScanThreads, lds, s>>>(pk, h0_ptr, h0_idx, pre, tot, kp, m, slice_rows);
  const dim3 ogrid((m + enc::kOutRows - 1) / enc::kOutRows, groups);
  if (aligned)
    enc::stair_out_kernel<W, true><<<ogrid, 256, 0, s>>>(pre, tot, cw, k, n, m, batch, slices, slice_rows);
  else
    enc::stair_out_kernel<W, false><<<ogrid, 256, 0, s>>>(pre, tot, cw, k, n, m, batch, slices, slice_rows);
}

int DeviceEncoder::launch_staircase(const uint8_t *in, uint8_t *cw, size_t batch, hipStream_t s) {
  const uint32_t k = static_cast<uint32_t>(k_), n = static_cast<uint32_t>(n_);
  const uint32_t kp = (k + 7) / 8 * 8;
  const int form = staircase_form(k_);
  const size_t word = form == 1 ? 2 : 4, frames_per_group = 8 * word;
  const size_t pass = std::min(batch, kEncPassFrames), groups = (pass + frames_per_group - 1) / frames_per_group;
  if (int rc = grow(d_packed_, groups * kp * word + 16)) return rc;
  if (int rc = grow(d_prefix_, groups * (m_ + 8) * word)) return rc;
  const uint32_t *const h0_ptr = d_h0_ptr_.get<uint32_t>(), *const h0_idx = d_h0_idx_.get<uint32_t>();
  for (size_t b0 = 0; b0 < batch; b0 += pass) {
    const uint32_t nb = static_cast<uint32_t>(std::min(pass, batch - b0));
    const uint8_t *pin = in + b0 * k_;
    uint8_t *pcw = cw + b0 * n_;
    if (form == 0)
      enc_staircase_pass<uint32_t, true>(pin, pcw, nb, k, n, kp, d_packed_.get(), d_prefix_.get(), h0_ptr, h0_idx, s);
    else if (form == 1)
      enc_staircase_pass<uint16_t, true>(pin, pcw, nb, k, n, kp, d_packed_.get(), d_prefix_.get(), h0_ptr, h0_idx, s);
    else
      enc_staircase_pass<uint32_t, false>(pin, pcw, nb, k, n, kp, d_packed_.get(), d_prefix_.get(), h0_ptr, h0_idx, s);
  }
  return 0;
}

int DeviceEncoder::launch_dense(const uint8_t *in, uint8_t *cw, size_t batch, hipStream_t s) {
  const uint32_t k = static_cast<uint32_t>(k_), n = static_cast<uint32_t>(n_), m = static_cast<uint32_t>(m_);
  const uint32_t words = static_cast<uint32_t>(words_), m_pad = static_cast<uint32_t>(m_pad_);
  // passes of at most 2^20 frames (the frame index is a 32-bit grid dimension)
  const size_t pass = std::min<size_t>(batch, size_t(1) << 20), bpad = (pass + 63) / 64 * 64;
  if (int rc = grow(d_packed_, std::max<size_t>(words, 1) * bpad * sizeof(uint64_t))) return rc;
  for (size_t b0 = 0; b0 < batch; b0 += pass) {
    const uint32_t nb = static_cast<uint32_t>(std::min(pass, batch - b0)), nbpad = (nb + 63) / 64 * 64;
    const uint8_t *pin = in + b0 * k_;
    uint8_t *pcw = cw + b0 * n_;
    uint64_t *pk = d_packed_.get<uint64_t>();
    if (words > 0)
      enc::pack_words_kernel<<<dim3(nbpad, (words + 3) / 4), 256, 0, s>>>(pin, pcw, pk, k, n, words, nb, nbpad);
    if (m > 0)
      enc::dense_parity_kernel<<<dim3(nbpad / 64, m_pad / 64), 256, 0, s>>>(d_gen_t_.get<uint64_t>(), pk, pcw, k, n, m, m_pad, words, nb, nbpad);
  }
  return 0;
}

int DeviceEncoder::encode_device(const uint8_t *input, uint8_t *output, size_t batch, hipStream_t stream) {
  if (batch == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  uint8_t *cw = output;
  if (d_keep_) {  // the full codewords go to a buffer of the handle, the kept blocks from there to the output
    if (int rc = grow(d_cw_, batch * n_)) return rc;
    cw = d_cw_.get<uint8_t>();
  }
  if (int rc = staircase_ ? launch_staircase(input, cw, batch, s) : launch_dense(input, cw, batch, s)) return rc;
  if (d_keep_) {
    const uint64_t total = uint64_t(batch) * out_len_;
    const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>((total + 255) / 256, 256 * 32));
    if (total > 0)
      enc::puncture_kernel<<<blocks, 256, 0, s>>>(cw, output, d_keep_.get<uint32_t>(), static_cast<uint32_t>(n_), block_, kept_, total);
  }
  return end(stream, s);
}

int DeviceEncoder::encode_host(const uint8_t *input, uint8_t *output, size_t batch) {
  if (batch == 0) return 0;
  return staged_rows(input, k_, output, out_len_, batch, batch, false,
                     [&](size_t frames) { return encode_device(d_in_.get<uint8_t>(), d_out_.get<uint8_t>(), frames, stream_); });
}

}  // namespace ldpc
