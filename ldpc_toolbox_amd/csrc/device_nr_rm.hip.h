// Host side of the batched NR rate matcher (device_nr_rm.h): the launches and the entries; their stream protocol and staging
// loop are device_stage.h's.
// Included by simulator.hip -- it shares the simulator's translation unit, as the BCH code does.
#pragma once
#include <algorithm>
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

DeviceNrRm *DeviceNrRm::create(const nrrm::Config &c, int device, std::string *err) {
  if (!select_device(device, "the rate matcher has", err)) return nullptr;
  std::unique_ptr<DeviceNrRm> d(new DeviceNrRm(device));
  d->c_ = c;
  if (!d->create_stream("the rate matcher's", err)) return nullptr;
  return d.release();
}

// (the members free what they own, the stream last)
DeviceNrRm::~DeviceNrRm() { wait_idle(); }

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
  const size_t stage = std::min(batch, std::max<size_t>(kNrRmStageBytes / std::max<size_t>(c_.n, e), 1));
  return staged_rows(codewords, c_.n, output, e, batch, stage, false, [&](size_t frames) {
    return match_device(d_in_.get<uint8_t>(), d_out_.get<uint8_t>(), frames, e, rv, qm, stream_);
  });
}

int DeviceNrRm::recover_host(const void *rx, void *llrs, bool f64, size_t batch, uint32_t e, uint32_t rv, uint32_t qm,
                             double filler_llr, bool combine) {
  if (batch == 0) return 0;
  const size_t el = f64 ? sizeof(double) : sizeof(float);
  const size_t stage = std::min(batch, std::max<size_t>(kNrRmStageBytes / (std::max<size_t>(c_.n, e) * el), 1));
  return staged_rows(rx, e * el, llrs, c_.n * el, batch, stage, combine, [&](size_t frames) {
    return recover_device(d_in_.get(), d_out_.get(), f64, frames, e, rv, qm, filler_llr, combine, stream_);
  });
}

int DeviceNrRm::recover_i8_host(const int8_t *rx, int8_t *llrs, size_t batch, uint32_t e, uint32_t rv, uint32_t qm, int32_t filler,
                                bool combine) {
  if (batch == 0) return 0;
  const size_t stage = std::min(batch, std::max<size_t>(kNrRmStageBytes / std::max<size_t>(c_.n, e), 1));
  return staged_rows(rx, e, llrs, c_.n, batch, stage, combine, [&](size_t frames) {
    return recover_i8_device(d_in_.get<int8_t>(), d_out_.get<int8_t>(), frames, e, rv, qm, filler, combine, stream_);
  });
}

}  // namespace ldpc
