// Host side of the batched NR transport block processing (device_nr_tb.h): the launches and the strided copies of the host
// entries; their stream protocol and staging loop are device_stage.h's.
// Included by simulator.hip -- it shares the simulator's translation unit, as the rate matcher does.
#pragma once
#include <algorithm>
#include <memory>

#include "device_nr_tb.h"
#include "kernels_nr_tb.hip.h"

namespace ldpc {

DeviceNrTb *DeviceNrTb::create(const nrtb::Config &c, int device, std::string *err) {
  if (!select_device(device, "the transport block entries have", err)) return nullptr;
  std::unique_ptr<DeviceNrTb> d(new DeviceNrTb(device));
  d->c_ = c;
  if (!d->create_stream("the handle's", err)) return nullptr;
  hipError_t e;
  d->d_tables_ = upload(nrtb::device_tables(c), &e);
  if (e != hipSuccess) {
    if (err) *err = std::string("uploading the CRC tables failed: ") + hipGetErrorString(e);
    return nullptr;
  }
  return d.release();
}

// (the members free what they own, the stream last)
DeviceNrTb::~DeviceNrTb() { wait_idle(); }

namespace {
nrtb::RowArgs nr_tb_row_args(const nrtb::Config &c, const uint32_t *tables, size_t batch, size_t b0, size_t frames) {
  nrtb::RowArgs p;
  p.a = c.a;
  p.s = c.s;
  p.k_prime = c.k_prime;
  p.k = c.k;
  p.c = c.c;
  p.l_tb = c.l_tb;
  p.l_cb = c.l_cb;
  p.g_tb = nrtb::tb_poly(c);
  p.table_tb = tables;
  p.table_cb = tables + nrtb::power_entries(c);
  p.behind = tables + 2 * nrtb::power_entries(c);
  p.batch = batch;
  p.b0 = b0;
  p.frames = static_cast<uint32_t>(frames);
  return p;
}
}  // namespace

int DeviceNrTb::segment_device(const uint8_t *payload, uint8_t *rows, size_t batch, hipStream_t stream) {
  if (batch == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const size_t pass = std::max<size_t>(kNrTbPassRows / c_.c, 1);
  STAGE_TRY(d_part_.ensure((size_t(c_.c) + 1) * std::min(pass, batch) * sizeof(uint32_t), 256));
  for (size_t b0 = 0; b0 < batch; b0 += pass) {
    const size_t frames = std::min(pass, batch - b0);
    const nrtb::RowArgs p = nr_tb_row_args(c_, d_tables_.get<uint32_t>(), batch, b0, frames);
    const uint32_t grid = static_cast<uint32_t>(frames * c_.c);
    nrtb::rows_kernel<true><<<grid, nrtb::kThreads, 0, s>>>(payload, rows, d_part_.get<uint32_t>(), nullptr, p);
    nrtb::finish_kernel<true><<<static_cast<uint32_t>(frames), 64, 0, s>>>(d_part_.get<uint32_t>(), rows, nullptr, p);
  }
  return end(stream, s);
}

int DeviceNrTb::desegment_device(const uint8_t *rows, uint8_t *payload, uint8_t *tb_ok, uint8_t *cb_ok, size_t batch, hipStream_t stream) {
  if (batch == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const size_t pass = std::max<size_t>(kNrTbPassRows / c_.c, 1);
  STAGE_TRY(d_part_.ensure((size_t(c_.c) + 1) * std::min(pass, batch) * sizeof(uint32_t), 256));
  for (size_t b0 = 0; b0 < batch; b0 += pass) {
    const size_t frames = std::min(pass, batch - b0);
    const nrtb::RowArgs p = nr_tb_row_args(c_, d_tables_.get<uint32_t>(), batch, b0, frames);
    const uint32_t grid = static_cast<uint32_t>(frames * c_.c);
    nrtb::rows_kernel<false><<<grid, nrtb::kThreads, 0, s>>>(rows, payload, d_part_.get<uint32_t>(), cb_ok, p);
    nrtb::finish_kernel<false><<<static_cast<uint32_t>(frames), 64, 0, s>>>(d_part_.get<uint32_t>(), tb_ok, cb_ok, p);
  }
  return end(stream, s);
}

int DeviceNrTb::concatenate_device(const uint8_t *packed, uint8_t *output, const nrtb::Lengths &l, size_t batch, hipStream_t stream) {
  if (batch == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const size_t pass = std::max<size_t>(kNrTbPassElements / l.g, 1);
  for (size_t b0 = 0; b0 < batch; b0 += pass) {
    const size_t frames = std::min(pass, batch - b0);
    uint8_t *out = output + b0 * l.g;
    const uint32_t total = static_cast<uint32_t>(frames * l.g);
    const uint32_t shift = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(out) & 3);
    const uint32_t threads = static_cast<uint32_t>((uint64_t(total) + shift + 3) / 4);
    nrtb::concatenate_kernel<<<(threads + nrtb::kThreads - 1) / nrtb::kThreads, nrtb::kThreads, 0, s>>>(packed, out, total, shift,
                                                                                                      nrtb::make_packing(l, batch, b0));
  }
  return end(stream, s);
}

int DeviceNrTb::split_device(const void *rx, void *packed, bool f64, const nrtb::Lengths &l, size_t batch, hipStream_t stream) {
  if (batch == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const size_t pass = std::max<size_t>(kNrTbPassElements / l.g, 1);
  for (size_t b0 = 0; b0 < batch; b0 += pass) {
    const size_t frames = std::min(pass, batch - b0);
    const uint32_t total = static_cast<uint32_t>(frames * l.g);
    const uint32_t grid = (total + nrtb::kThreads - 1) / nrtb::kThreads;
    const nrtb::Packing p = nrtb::make_packing(l, batch, b0);
    if (f64)
      nrtb::split_kernel<double><<<grid, nrtb::kThreads, 0, s>>>(static_cast<const double *>(rx) + b0 * l.g, static_cast<double *>(packed), total, p);
    else
      nrtb::split_kernel<float><<<grid, nrtb::kThreads, 0, s>>>(static_cast<const float *>(rx) + b0 * l.g, static_cast<float *>(packed), total, p);
  }
  return end(stream, s);
}

int DeviceNrTb::copy_rows(char *dst, const char *src, size_t blocks, size_t row_bytes, size_t batch, size_t b0, size_t frames, bool to_device) {
  for (size_t r = 0; r < blocks; r++) {
    const size_t host_at = (r * batch + b0) * row_bytes, dev_at = r * frames * row_bytes;
    if (to_device)
      STAGE_TRY(hipMemcpyAsync(dst + dev_at, src + host_at, frames * row_bytes, hipMemcpyHostToDevice, stream_));
    else
      STAGE_TRY(hipMemcpyAsync(dst + host_at, src + dev_at, frames * row_bytes, hipMemcpyDeviceToHost, stream_));
  }
  return 0;
}

int DeviceNrTb::copy_packed(char *dev, char *host, const nrtb::Lengths &l, size_t el, size_t batch, size_t b0, size_t frames, bool to_device) {
  char *host_hi = host + size_t(l.c_lo) * batch * l.e_lo * el, *dev_hi = dev + size_t(l.c_lo) * frames * l.e_lo * el;
  if (to_device) {
    if (int rc = copy_rows(dev, host, l.c_lo, size_t(l.e_lo) * el, batch, b0, frames, true)) return rc;
    return copy_rows(dev_hi, host_hi, c_.c - l.c_lo, size_t(l.e_hi) * el, batch, b0, frames, true);
  }
  if (int rc = copy_rows(host, dev, l.c_lo, size_t(l.e_lo) * el, batch, b0, frames, false)) return rc;
  return copy_rows(host_hi, dev_hi, c_.c - l.c_lo, size_t(l.e_hi) * el, batch, b0, frames, false);
}

int DeviceNrTb::segment_host(const uint8_t *payload, uint8_t *rows, size_t batch) {
  if (batch == 0) return 0;
  const size_t per_tb = size_t(c_.c) * c_.k;
  const size_t stage = std::min(batch, std::max<size_t>(kNrTbStageBytes / per_tb, 1));
  return staged(batch, stage, {{d_in_, c_.a}, {d_out_, per_tb}}, [&](size_t b0, size_t frames) {
    STAGE_TRY(hipMemcpyAsync(d_in_.get(), payload + b0 * c_.a, frames * c_.a, hipMemcpyHostToDevice, stream_));
    if (int rc = segment_device(d_in_.get<uint8_t>(), d_out_.get<uint8_t>(), frames, stream_)) return rc;
    return copy_rows(reinterpret_cast<char *>(rows), d_out_.get<char>(), c_.c, c_.k, batch, b0, frames, false);
  });
}

int DeviceNrTb::desegment_host(const uint8_t *rows, uint8_t *payload, uint8_t *tb_ok, uint8_t *cb_ok, size_t batch) {
  if (batch == 0) return 0;
  const size_t per_tb = size_t(c_.c) * c_.k;
  const size_t stage = std::min(batch, std::max<size_t>(kNrTbStageBytes / per_tb, 1));
  return staged(batch, stage, {{d_in_, per_tb}, {d_out_, c_.a}, {d_flags_, size_t(c_.c) + 1}}, [&](size_t b0, size_t frames) {
    uint8_t *d_tb = d_flags_.get<uint8_t>(), *d_cb = d_tb + stage;
    if (int rc = copy_rows(d_in_.get<char>(), reinterpret_cast<const char *>(rows), c_.c, c_.k, batch, b0, frames, true)) return rc;
    if (int rc = desegment_device(d_in_.get<uint8_t>(), d_out_.get<uint8_t>(), d_tb, cb_ok ? d_cb : nullptr, frames, stream_)) return rc;
    STAGE_TRY(hipMemcpyAsync(payload + b0 * c_.a, d_out_.get(), frames * c_.a, hipMemcpyDeviceToHost, stream_));
    STAGE_TRY(hipMemcpyAsync(tb_ok + b0, d_tb, frames, hipMemcpyDeviceToHost, stream_));
    if (cb_ok) STAGE_TRY(hipMemcpyAsync(cb_ok + b0 * c_.c, d_cb, frames * c_.c, hipMemcpyDeviceToHost, stream_));
    return 0;
  });
}

int DeviceNrTb::concatenate_host(const uint8_t *packed, uint8_t *output, const nrtb::Lengths &l, size_t batch) {
  if (batch == 0) return 0;
  const size_t stage = std::min(batch, std::max<size_t>(kNrTbStageBytes / l.g, 1));
  return staged(batch, stage, {{d_in_, l.g}, {d_out_, l.g}}, [&](size_t b0, size_t frames) {
    if (int rc = copy_packed(d_in_.get<char>(), const_cast<char *>(reinterpret_cast<const char *>(packed)), l, 1, batch, b0, frames, true)) return rc;
    if (int rc = concatenate_device(d_in_.get<uint8_t>(), d_out_.get<uint8_t>(), l, frames, stream_)) return rc;
    STAGE_TRY(hipMemcpyAsync(output + b0 * l.g, d_out_.get(), frames * l.g, hipMemcpyDeviceToHost, stream_));
    return 0;
  });
}

int DeviceNrTb::split_host(const void *rx, void *packed, bool f64, const nrtb::Lengths &l, size_t batch) {
  if (batch == 0) return 0;
  const size_t el = f64 ? sizeof(double) : sizeof(float);
  const size_t stage = std::min(batch, std::max<size_t>(kNrTbStageBytes / (size_t(l.g) * el), 1));
  return staged(batch, stage, {{d_in_, l.g * el}, {d_out_, l.g * el}}, [&](size_t b0, size_t frames) {
    STAGE_TRY(hipMemcpyAsync(d_in_.get(), static_cast<const char *>(rx) + b0 * l.g * el, frames * l.g * el, hipMemcpyHostToDevice, stream_));
    if (int rc = split_device(d_in_.get(), d_out_.get(), f64, l, frames, stream_)) return rc;
    return copy_packed(d_out_.get<char>(), static_cast<char *>(packed), l, el, batch, b0, frames, false);
  });
}

}  // namespace ldpc
