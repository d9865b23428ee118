// Host side of the batched NR rate matcher (device_nr_rm.h): the launches and the staged host entries.
// Included by simulator.hip -- it shares the simulator's translation unit, as the BCH code does.
#pragma once
#include <algorithm>
#include <cstdio>
#include <memory>

#include "device_nr_rm.h"
#include "kernels_nr_rm.hip.h"

namespace ldpc {

namespace {
// frames of a pass over rows of `row` elements: the pass's elements stay below 2^31
inline size_t nr_rm_pass_frames(size_t row) { return std::max<size_t>(kNrRmPassElements / row, 1); }
}  // namespace

void nr_rm_launch_match(const nrrm::Plan &p, const uint8_t *codewords, uint8_t *output, size_t batch, hipStream_t s) {
  const size_t pass = nr_rm_pass_frames(p.e);
  const dev::FastDiv div_e = dev::fast_div(p.e);
  for (size_t b0 = 0; b0 < batch; b0 += pass) {
    const size_t frames = std::min(pass, batch - b0);
    uint8_t *out = output + b0 * p.e;
    const uint32_t total = static_cast<uint32_t>(frames * p.e);
    const uint32_t shift = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(out) & 3);
    const uint32_t threads = static_cast<uint32_t>((uint64_t(total) + shift + 3) / 4);
    nrrm::nr_rm_match_kernel<<<(threads + nrrm::kThreads - 1) / nrrm::kThreads, nrrm::kThreads, 0, s>>>(codewords + b0 * p.n, out, total,
                                                                                                        shift, p, div_e);
  }
}

template <typename T>
void nr_rm_launch_recover(const nrrm::Plan &p, const T *rx, T *llrs, size_t batch, T filler, bool combine, hipStream_t s) {
  const size_t pass = nr_rm_pass_frames(std::max(p.n, p.e));
  const dev::FastDiv div_n = dev::fast_div(p.n);
  for (size_t b0 = 0; b0 < batch; b0 += pass) {
    const size_t frames = std::min(pass, batch - b0);
    const uint32_t total = static_cast<uint32_t>(frames * p.n);
    nrrm::nr_rm_recover_kernel<T><<<(total + nrrm::kThreads - 1) / nrrm::kThreads, nrrm::kThreads, 0, s>>>(
        rx + b0 * p.e, llrs + b0 * p.n, total, p, div_n, filler, combine ? 1 : 0);
  }
}
template void nr_rm_launch_recover<float>(const nrrm::Plan &, const float *, float *, size_t, float, bool, hipStream_t);
template void nr_rm_launch_recover<double>(const nrrm::Plan &, const double *, double *, size_t, double, bool, hipStream_t);

void nr_rm_launch_recover_i8(const nrrm::Plan &p, const int8_t *rx, int8_t *llrs, size_t batch, int32_t filler, bool combine, hipStream_t s) {
  const size_t pass = nr_rm_pass_frames(std::max(p.n, p.e));
  const dev::FastDiv div_n = dev::fast_div(p.n);
  for (size_t b0 = 0; b0 < batch; b0 += pass) {
    const size_t frames = std::min(pass, batch - b0);
    int8_t *out = llrs + b0 * p.n;
    const uint32_t total = static_cast<uint32_t>(frames * p.n);
    const uint32_t shift = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(out) & 3);
    const uint32_t threads = static_cast<uint32_t>((uint64_t(total) + shift + 3) / 4);
    nrrm::nr_rm_recover_i8_kernel<<<(threads + nrrm::kThreads - 1) / nrrm::kThreads, nrrm::kThreads, 0, s>>>(
        rx + b0 * p.e, out, total, shift, p, div_n, filler, combine ? 1 : 0);
  }
}

bool DeviceNrRm::fail(const std::string &m, hipError_t e) {
  error_ = m;
  if (e != hipSuccess) error_ += std::string(": ") + hipGetErrorString(e);
  std::fprintf(stderr, "ldpc_toolbox (hip): nr_rm: %s\n", error_.c_str());
  return false;
}

#define NRRM_TRY(expr)                \
  do {                                \
    hipError_t _e = (expr);           \
    if (_e != hipSuccess) {           \
      fail(#expr, _e);                \
      return -2;                      \
    }                                 \
  } while (0)

DeviceNrRm *DeviceNrRm::create(const nrrm::Config &c, int device, std::string *err) {
  auto bail = [&](const std::string &m) -> DeviceNrRm * {
    if (err) *err = m;
    return nullptr;
  };
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return bail("no HIP device available: the rate matcher has no CPU path");
  if (device < 0 || device >= count) return bail("HIP device index out of range");
  if (hipSetDevice(device) != hipSuccess) return bail("hipSetDevice failed");
  std::unique_ptr<DeviceNrRm> d(new DeviceNrRm());
  d->c_ = c;
  d->device_ = device;
  if (d->stream_.create() != hipSuccess || d->ev_default_.create() != hipSuccess) return bail("creating the rate matcher's stream failed");
  return d.release();
}

// (the members free what they own, the stream last)
DeviceNrRm::~DeviceNrRm() {
  (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize(stream_);
}

int DeviceNrRm::begin(hipStream_t stream, hipStream_t *s) {
  NRRM_TRY(hipSetDevice(device_));
  *s = stream ? stream : static_cast<hipStream_t>(stream_);
  if (!stream) {
    // (the handle's stream is non-blocking: ordered explicitly after what the legacy default stream holds now)
    NRRM_TRY(hipEventRecord(ev_default_, nullptr));
    NRRM_TRY(hipStreamWaitEvent(*s, ev_default_, 0));
  }
  return 0;
}

int DeviceNrRm::end(hipStream_t stream, hipStream_t s) {
  NRRM_TRY(hipGetLastError());
  if (!stream) NRRM_TRY(hipStreamSynchronize(s));
  return 0;
}

int DeviceNrRm::match_device(const uint8_t *codewords, uint8_t *output, size_t batch, uint32_t e, uint32_t rv, uint32_t qm,
                             hipStream_t stream) {
  if (batch == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  nr_rm_launch_match(nrrm::make_plan(c_, e, rv, qm), codewords, output, batch, s);
  return end(stream, s);
}

int DeviceNrRm::recover_device(const void *rx, void *llrs, bool f64, size_t batch, uint32_t e, uint32_t rv, uint32_t qm,
                               double filler_llr, bool combine, hipStream_t stream) {
  if (batch == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const nrrm::Plan p = nrrm::make_plan(c_, e, rv, qm);
  if (f64)
    nr_rm_launch_recover<double>(p, static_cast<const double *>(rx), static_cast<double *>(llrs), batch, filler_llr, combine, s);
  else
    nr_rm_launch_recover<float>(p, static_cast<const float *>(rx), static_cast<float *>(llrs), batch, static_cast<float>(filler_llr),
                                combine, s);
  return end(stream, s);
}

int DeviceNrRm::recover_i8_device(const int8_t *rx, int8_t *llrs, size_t batch, uint32_t e, uint32_t rv, uint32_t qm, int32_t filler,
                                  bool combine, hipStream_t stream) {
  if (batch == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  nr_rm_launch_recover_i8(nrrm::make_plan(c_, e, rv, qm), rx, llrs, batch, filler, combine, s);
  return end(stream, s);
}

int DeviceNrRm::match_host(const uint8_t *codewords, uint8_t *output, size_t batch, uint32_t e, uint32_t rv, uint32_t qm) {
  if (batch == 0) return 0;
  NRRM_TRY(hipSetDevice(device_));
  const size_t stage = std::min(batch, std::max<size_t>(kNrRmStageBytes / std::max<size_t>(c_.n, e), 1));
  NRRM_TRY(d_in_.ensure(stage * c_.n, 256));
  NRRM_TRY(d_out_.ensure(stage * e, 256));
  for (size_t b0 = 0; b0 < batch; b0 += stage) {
    const size_t frames = std::min(stage, batch - b0);
    NRRM_TRY(hipMemcpyAsync(d_in_.get(), codewords + b0 * c_.n, frames * c_.n, hipMemcpyHostToDevice, stream_));
    if (int rc = match_device(d_in_.get<uint8_t>(), d_out_.get<uint8_t>(), frames, e, rv, qm, stream_)) return rc;
    NRRM_TRY(hipMemcpyAsync(output + b0 * e, d_out_.get(), frames * e, hipMemcpyDeviceToHost, stream_));
    // (the next stage overwrites the buffers this one reads)
    NRRM_TRY(hipStreamSynchronize(stream_));
  }
  return 0;
}

int DeviceNrRm::recover_host(const void *rx, void *llrs, bool f64, size_t batch, uint32_t e, uint32_t rv, uint32_t qm,
                             double filler_llr, bool combine) {
  if (batch == 0) return 0;
  NRRM_TRY(hipSetDevice(device_));
  const size_t el = f64 ? sizeof(double) : sizeof(float);
  const size_t stage = std::min(batch, std::max<size_t>(kNrRmStageBytes / (std::max<size_t>(c_.n, e) * el), 1));
  NRRM_TRY(d_in_.ensure(stage * e * el, 256));
  NRRM_TRY(d_out_.ensure(stage * c_.n * el, 256));
  const char *src = static_cast<const char *>(rx);
  char *dst = static_cast<char *>(llrs);
  for (size_t b0 = 0; b0 < batch; b0 += stage) {
    const size_t frames = std::min(stage, batch - b0);
    NRRM_TRY(hipMemcpyAsync(d_in_.get(), src + b0 * e * el, frames * e * el, hipMemcpyHostToDevice, stream_));
    if (combine) NRRM_TRY(hipMemcpyAsync(d_out_.get(), dst + b0 * c_.n * el, frames * c_.n * el, hipMemcpyHostToDevice, stream_));
    if (int rc = recover_device(d_in_.get(), d_out_.get(), f64, frames, e, rv, qm, filler_llr, combine, stream_)) return rc;
    NRRM_TRY(hipMemcpyAsync(dst + b0 * c_.n * el, d_out_.get(), frames * c_.n * el, hipMemcpyDeviceToHost, stream_));
    NRRM_TRY(hipStreamSynchronize(stream_));
  }
  return 0;
}

int DeviceNrRm::recover_i8_host(const int8_t *rx, int8_t *llrs, size_t batch, uint32_t e, uint32_t rv, uint32_t qm, int32_t filler,
                                bool combine) {
  if (batch == 0) return 0;
  NRRM_TRY(hipSetDevice(device_));
  const size_t stage = std::min(batch, std::max<size_t>(kNrRmStageBytes / std::max<size_t>(c_.n, e), 1));
  NRRM_TRY(d_in_.ensure(stage * e, 256));
  NRRM_TRY(d_out_.ensure(stage * c_.n, 256));
  for (size_t b0 = 0; b0 < batch; b0 += stage) {
    const size_t frames = std::min(stage, batch - b0);
    NRRM_TRY(hipMemcpyAsync(d_in_.get(), rx + b0 * e, frames * e, hipMemcpyHostToDevice, stream_));
    if (combine) NRRM_TRY(hipMemcpyAsync(d_out_.get(), llrs + b0 * c_.n, frames * c_.n, hipMemcpyHostToDevice, stream_));
    if (int rc = recover_i8_device(d_in_.get<int8_t>(), d_out_.get<int8_t>(), frames, e, rv, qm, filler, combine, stream_)) return rc;
    NRRM_TRY(hipMemcpyAsync(llrs + b0 * c_.n, d_out_.get(), frames * c_.n, hipMemcpyDeviceToHost, stream_));
    NRRM_TRY(hipStreamSynchronize(stream_));
  }
  return 0;
}

#undef NRRM_TRY

}  // namespace ldpc
