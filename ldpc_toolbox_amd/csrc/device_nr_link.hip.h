// Host side of the NR link handle (device_nr_link.h): the stage handles it owns, the launches of its own kernels and the
// entries; their stream protocol is device_stage.h's.
// Included by simulator.hip -- it shares the simulator's translation unit, as the stages it drives do.
#pragma once
#include <algorithm>
#include <limits>
#include <memory>
#include <string>

#include "codes.h"
#include "device_decoder.h"
#include "device_encoder.h"
#include "device_nr_link.h"
#include "device_nr_qam.h"
#include "device_nr_rm.h"
#include "device_nr_tb.h"
#include "encoder.h"
#include "kernels_nr_link.hip.h"
#include "sparse.h"

namespace ldpc {

DeviceNrLink::DeviceNrLink(int device) : DeviceStage("nr_link", device) {}

// (the stages go first, each after waiting for its own work; then the buffers, the stream last)
DeviceNrLink::~DeviceNrLink() { wait_idle(); }

DeviceNrLink *DeviceNrLink::create(const nrlink::Config &c, const Implementation &impl, uint32_t slots, uint32_t soft_bits, int device,
                                   std::string *err) {
  if (err) err->clear();
  if (!select_device(device, "the link handle has", err)) return nullptr;
  std::unique_ptr<DeviceNrLink> d(new DeviceNrLink(device));
  d->c_ = c;
  d->slots_ = slots;
  d->soft_bytes_ = soft_bits / 8;
  d->filler_ = std::numeric_limits<float>::infinity();
  d->used_.assign(slots, 0);
  if (!d->create_stream("the link handle's", err)) return nullptr;
  // the code of the blocks, through its alist text: the graph a caller's own encoder and decoder handles are made of
  const std::string code = "nr5g:" + std::to_string(c.tb.bg) + ":" + std::to_string(c.tb.zc);
  SparseMatrix table, h;
  Encoder enc;
  if (!codes::by_spec(code, &table) || !SparseMatrix::from_alist(table.alist(true), &h, err) || !Encoder::from_h(h, &enc, err)) {
    if (err && err->empty()) *err = "no code " + code;
    return nullptr;
  }
  d->tb_.reset(DeviceNrTb::create(c.tb, device, err));
  if (d->tb_) d->enc_.reset(DeviceEncoder::create(enc, {}, device, err));
  if (d->enc_) d->rm_.reset(DeviceNrRm::create(c.rm, device, err));
  nrqam::Config qam;
  if (d->rm_ && nrqam::parse_spec("nr5g-qam:" + std::to_string(c.qm), &qam, err)) d->qam_.reset(DeviceNrQam::create(qam, device, err));
  if (d->qam_) d->dec_.reset(DeviceDecoder::create(h, impl, {}, device, err));
  if (!d->dec_) return nullptr;
  const size_t rows = size_t(c.tb.c) * slots;
  hipError_t e = d->d_soft_.ensure(rows * c.tb.n * d->soft_bytes_, 256);
  if (e == hipSuccess) e = d->d_hard_.ensure(rows * c.tb.k, 256);
  if (e == hipSuccess) e = d->d_its_.ensure(rows * sizeof(int32_t), 256);
  if (e == hipSuccess) e = d->d_done_.ensure(rows, 256);
  if (e == hipSuccess) e = d->d_count_.ensure(sizeof(uint32_t), 256);
  // a slot that nothing has been received into reads as zeros (ldpc_toolbox_nr_link_slot_state)
  if (e == hipSuccess) e = hipMemsetAsync(d->d_soft_.get(), 0, rows * c.tb.n * d->soft_bytes_, d->stream_);
  if (e == hipSuccess) e = hipMemsetAsync(d->d_hard_.get(), 0, rows * c.tb.k, d->stream_);
  if (e == hipSuccess) e = hipMemsetAsync(d->d_its_.get(), 0, rows * sizeof(int32_t), d->stream_);
  if (e == hipSuccess) e = hipMemsetAsync(d->d_done_.get(), 0, rows, d->stream_);
  if (e == hipSuccess) e = hipStreamSynchronize(d->stream_);
  if (e != hipSuccess) {
    if (err) *err = std::string("allocating the HARQ slots failed: ") + hipGetErrorString(e);
    return nullptr;
  }
  return d.release();
}

bool DeviceNrLink::slots_used(uint32_t first_slot, size_t batch) const {
  return std::all_of(used_.begin() + first_slot, used_.begin() + first_slot + batch, [](uint8_t u) { return u != 0; });
}

size_t DeviceNrLink::transmit_chunk() const {
  return std::max<size_t>(nrlink::kStageBytes / (size_t(c_.tb.c) * c_.tb.n), 1);
}

int DeviceNrLink::transmit_device(const uint8_t *payload, float *symbols, size_t batch, uint32_t rv, int64_t c_init, hipStream_t stream) {
  if (batch == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const nrtb::Config &t = c_.tb;
  const nrtb::Lengths &l = c_.len;
  const size_t chunk = std::min(batch, transmit_chunk());
  STAGE_TRY(d_rows_.ensure(chunk * t.c * t.k, 256));
  STAGE_TRY(d_cws_.ensure(chunk * t.c * t.n, 256));
  STAGE_TRY(d_packed_.ensure(chunk * l.g, 256));
  STAGE_TRY(d_tx_.ensure(chunk * l.g, 256));
  auto stage = [&](DeviceStage &h, int rc) {
    if (rc != 0) fail(h.last_error());
    return rc;
  };
  for (size_t b0 = 0; b0 < batch; b0 += chunk) {
    const size_t frames = std::min(chunk, batch - b0);
    const size_t lo_rows = size_t(l.c_lo) * frames, hi_rows = size_t(t.c - l.c_lo) * frames;
    uint8_t *cws = d_cws_.get<uint8_t>(), *packed = d_packed_.get<uint8_t>();
    if (int rc = stage(*tb_, tb_->segment_device(payload + b0 * t.a, d_rows_.get<uint8_t>(), frames, s))) return rc;
    if (int rc = stage(*enc_, enc_->encode_device(d_rows_.get<uint8_t>(), cws, frames * t.c, s))) return rc;
    if (int rc = stage(*rm_, rm_->match_device(cws, packed, lo_rows, l.e_lo, rv, c_.qm, s))) return rc;
    if (int rc = stage(*rm_, rm_->match_device(cws + lo_rows * t.n, packed + lo_rows * l.e_lo, hi_rows, l.e_hi, rv, c_.qm, s))) return rc;
    if (int rc = stage(*tb_, tb_->concatenate_device(packed, d_tx_.get<uint8_t>(), l, frames, s))) return rc;
    if (int rc = stage(*qam_, qam_->mod_device(d_tx_.get<uint8_t>(), symbols + b0 * c_.symbols * 2, false, l.g, c_.symbols, frames, c_init, s)))
      return rc;
  }
  return end(stream, s);
}

int DeviceNrLink::recover_into_slots(const void *rx, size_t batch, uint32_t rv, uint32_t first_slot, bool combine, hipStream_t s) {
  const nrlink::Geometry k = nrlink::make_geometry(c_);
  const nrrm::Plan p_lo = nrrm::make_plan(c_.rm, c_.len.e_lo, rv, c_.qm), p_hi = nrrm::make_plan(c_.rm, c_.len.e_hi, rv, c_.qm);
  const nrlink::SlotArgs sl{c_.tb.c, slots_, first_slot, static_cast<uint32_t>(batch)};
  // a first reception resets the slots: no block of them is done
  if (!combine) STAGE_TRY(hipMemsetAsync(d_done_.get<uint8_t>() + size_t(first_slot) * k.c, 0, batch * k.c, s));
  std::fill(used_.begin() + first_slot, used_.begin() + first_slot + batch, uint8_t(1));
  const uint64_t elements = uint64_t(batch) * k.per_tb;
  if (soft_i8()) {
    // four columns and one dword per thread: passes of whole dwords
    const uint64_t per_pass = nrlink::dword_pass_elements(pass_elements_);
    for (uint64_t first = 0; first < elements; first += per_pass) {
      const nrlink::Pass pass = nrlink::make_pass(c_, first, std::min<uint64_t>(per_pass, elements - first));
      nrlink::recover_i8_kernel<<<(pass.total / 4 + nrlink::kThreads - 1) / nrlink::kThreads, nrlink::kThreads, 0, s>>>(
          static_cast<const int8_t *>(rx), d_soft_.get<int8_t>(), d_done_.get<uint8_t>(), k, pass, sl, p_lo, p_hi, filler_soft_bit_, combine ? 1 : 0);
    }
    return 0;
  }
  for (uint64_t first = 0; first < elements; first += pass_elements_) {
    const nrlink::Pass pass = nrlink::make_pass(c_, first, std::min<uint64_t>(pass_elements_, elements - first));
    nrlink::recover_kernel<<<(pass.total + nrlink::kThreads - 1) / nrlink::kThreads, nrlink::kThreads, 0, s>>>(
        static_cast<const float *>(rx), d_soft_.get<float>(), d_done_.get<uint8_t>(), k, pass, sl, p_lo, p_hi, filler_, combine ? 1 : 0);
  }
  return 0;
}

int DeviceNrLink::recover_device(const void *rx, size_t batch, uint32_t rv, uint32_t first_slot, bool combine, hipStream_t stream) {
  if (batch == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  if (int rc = recover_into_slots(rx, batch, rv, first_slot, combine, s)) return rc;
  return end(stream, s);
}

int DeviceNrLink::receive_device(const float *symbols, const float *scale, uint8_t *payload, uint8_t *tb_ok, uint8_t *cb_ok,
                                 int32_t *iterations, size_t batch, double noise_sigma, uint32_t rv, int64_t c_init, uint32_t first_slot,
                                 bool combine, uint32_t max_iterations, hipStream_t stream) {
  if (batch == 0) return 0;
  hipStream_t s;
  if (int rc = begin(stream, &s)) return rc;
  const nrtb::Config &t = c_.tb;
  const size_t rows = size_t(t.c) * batch;
  const nrlink::SlotArgs sl{t.c, slots_, first_slot, static_cast<uint32_t>(batch)};
  uint8_t *done = d_done_.get<uint8_t>() + size_t(first_slot) * t.c;
  int32_t *its = d_its_.get<int32_t>() + size_t(first_slot) * t.c;
  STAGE_TRY(d_llrs_.ensure(batch * c_.len.g * soft_bytes_, 256));
  STAGE_TRY(d_list_.ensure(rows * sizeof(uint32_t), 256));
  STAGE_TRY(d_bits_.ensure(rows * t.k, 256));
  auto stage = [&](DeviceStage &h, int rc) {
    if (rc != 0) fail(h.last_error());
    return rc;
  };
  decoded_rows_ = skipped_rows_ = 0;
  int rc;
  if (soft_i8())
    rc = scale ? qam_->demap_csi_i8_device(symbols, scale, d_llrs_.get<int8_t>(), c_.symbols, c_.len.g, batch, max_log_, c_init, s)
               : qam_->demap_i8_device(symbols, d_llrs_.get<int8_t>(), c_.symbols, c_.len.g, batch, noise_sigma, max_log_, c_init, s);
  else
    rc = scale ? qam_->demap_csi_device(symbols, scale, d_llrs_.get(), false, c_.symbols, c_.len.g, batch, max_log_, c_init, s)
               : qam_->demod_device(symbols, d_llrs_.get(), false, c_.symbols, c_.len.g, batch, noise_sigma, max_log_, c_init, s);
  if (stage(*qam_, rc)) return rc;
  if ((rc = recover_into_slots(d_llrs_.get(), batch, rv, first_slot, combine, s)) != 0) return rc;
  nrlink::active_list_kernel<<<1, 64, 0, s>>>(d_done_.get<uint8_t>(), d_list_.get<uint32_t>(), d_count_.get<uint32_t>(), sl,
                                              dev::fast_div(sl.batch));
  // a first reception decodes every row; a retransmission the rows the list holds, and the host has to know how many
  uint32_t active = static_cast<uint32_t>(rows);
  if (combine) {
    STAGE_TRY(hipMemcpyAsync(&active, d_count_.get(), sizeof(active), hipMemcpyDeviceToHost, s));
    STAGE_TRY(hipStreamSynchronize(s));
  }
  if (active > 0) {
    STAGE_TRY(d_dec_in_.ensure(size_t(active) * t.n * soft_bytes_, 256));
    STAGE_TRY(d_dec_bits_.ensure(size_t(active) * t.k, 256));
    STAGE_TRY(d_dec_its_.ensure(size_t(active) * sizeof(int32_t), 256));
    // rows of 16-byte units, or of dwords where 8-bit rows begin on a dword only
    const uint32_t row_bytes = t.n * static_cast<uint32_t>(soft_bytes_);
    if (row_bytes % 16 == 0)
      nrlink::gather_soft_kernel<<<active, nrlink::kThreads, 0, s>>>(d_soft_.get<float4>(), d_list_.get<uint32_t>(), d_dec_in_.get<float4>(),
                                                                     row_bytes / 16);
    else
      nrlink::gather_soft_dword_kernel<<<active, nrlink::kThreads, 0, s>>>(d_soft_.get<uint32_t>(), d_list_.get<uint32_t>(),
                                                                           d_dec_in_.get<uint32_t>(), row_bytes / 4);
    rc = dec_->decode_device(d_dec_in_.get(), soft_i8() ? LlrType::I8 : LlrType::F32, active, max_iterations, d_dec_bits_.get<uint8_t>(), t.k,
                             d_dec_its_.get<int32_t>(), nullptr, s);
    if (rc != 0) {
      fail(dec_->last_error());
      return -2;
    }
    nrlink::scatter_hard_kernel<<<active, nrlink::kThreads, 0, s>>>(d_dec_bits_.get<uint8_t>(), d_dec_its_.get<int32_t>(),
                                                                    d_list_.get<uint32_t>(), d_hard_.get<uint8_t>(), d_its_.get<int32_t>(),
                                                                    t.k, sl, dev::fast_div(slots_));
  }
  decoded_rows_ = active;
  skipped_rows_ = rows - active;
  nrlink::gather_hard_kernel<<<static_cast<uint32_t>(rows), nrlink::kThreads, 0, s>>>(d_hard_.get<uint8_t>(), d_bits_.get<uint8_t>(), t.k, sl,
                                                                                    dev::fast_div(sl.batch));
  // the verdicts of the blocks are the slots' done flags: a done block's hard decisions have not changed, and it stays done
  if (stage(*tb_, rc = tb_->desegment_device(d_bits_.get<uint8_t>(), payload, tb_ok, done, batch, s))) return rc;
  if (cb_ok) STAGE_TRY(hipMemcpyAsync(cb_ok, done, rows, hipMemcpyDeviceToDevice, s));
  if (iterations) STAGE_TRY(hipMemcpyAsync(iterations, its, rows * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  return end(stream, s);
}

int DeviceNrLink::transmit_host(const uint8_t *payload, float *symbols, size_t batch, uint32_t rv, int64_t c_init) {
  if (batch == 0) return 0;
  const size_t stage = std::min(batch, transmit_chunk());
  return staged_rows(payload, c_.tb.a, symbols, size_t(c_.symbols) * 2 * sizeof(float), batch, stage, false, [&](size_t frames) {
    return transmit_device(d_in_.get<uint8_t>(), d_out_.get<float>(), frames, rv, c_init, stream_);
  });
}

int DeviceNrLink::receive_host(const float *symbols, const float *scale, uint8_t *payload, uint8_t *tb_ok, uint8_t *cb_ok,
                               int32_t *iterations, size_t batch, double noise_sigma, uint32_t rv, int64_t c_init, uint32_t first_slot,
                               bool combine, uint32_t max_iterations) {
  if (batch == 0) return 0;
  // the whole call at once: its transport blocks are at most the slots, whose soft rows are the larger arrays
  const size_t sym_row = size_t(c_.symbols) * 2 * sizeof(float), c = c_.tb.c;
  return staged(batch, batch, {{d_in_, sym_row}, {d_out_, c_.tb.a}, {d_scale_, c_.symbols * sizeof(float)}, {d_flags_, 5 * c + 5}},
                [&](size_t, size_t) {
                  uint8_t *d_tb = d_flags_.get<uint8_t>(), *d_cb = d_tb + batch;
                  // (the counts behind the flags, on a multiple of four bytes)
                  int32_t *d_it = reinterpret_cast<int32_t *>(d_flags_.get<uint8_t>() + (batch + c * batch + 3) / 4 * 4);
                  STAGE_TRY(hipMemcpyAsync(d_in_.get(), symbols, batch * sym_row, hipMemcpyHostToDevice, stream_));
                  if (scale) STAGE_TRY(hipMemcpyAsync(d_scale_.get(), scale, batch * c_.symbols * sizeof(float), hipMemcpyHostToDevice, stream_));
                  if (int rc = receive_device(d_in_.get<float>(), scale ? d_scale_.get<float>() : nullptr, d_out_.get<uint8_t>(), d_tb,
                                              cb_ok ? d_cb : nullptr, iterations ? d_it : nullptr, batch, noise_sigma, rv, c_init, first_slot,
                                              combine, max_iterations, stream_))
                    return rc;
                  STAGE_TRY(hipMemcpyAsync(payload, d_out_.get(), batch * c_.tb.a, hipMemcpyDeviceToHost, stream_));
                  STAGE_TRY(hipMemcpyAsync(tb_ok, d_tb, batch, hipMemcpyDeviceToHost, stream_));
                  if (cb_ok) STAGE_TRY(hipMemcpyAsync(cb_ok, d_cb, batch * c, hipMemcpyDeviceToHost, stream_));
                  if (iterations) STAGE_TRY(hipMemcpyAsync(iterations, d_it, batch * c * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
                  return 0;
                });
}

int DeviceNrLink::slot_state_host(void *soft, uint8_t *done, uint8_t *rows, uint32_t first_slot, size_t batch) {
  if (batch == 0) return 0;
  STAGE_TRY(hipSetDevice(device_));
  const size_t c = c_.tb.c, n = c_.tb.n, k = c_.tb.k;
  // block r of the range is one run of the slots' block-major rows
  for (size_t r = 0; r < c; r++) {
    const size_t from = r * slots_ + first_slot;
    if (soft)
      STAGE_TRY(hipMemcpyAsync(static_cast<uint8_t *>(soft) + r * batch * n * soft_bytes_, d_soft_.get<uint8_t>() + from * n * soft_bytes_,
                               batch * n * soft_bytes_, hipMemcpyDeviceToHost, stream_));
    if (rows) STAGE_TRY(hipMemcpyAsync(rows + r * batch * k, d_hard_.get<uint8_t>() + from * k, batch * k, hipMemcpyDeviceToHost, stream_));
  }
  if (done) STAGE_TRY(hipMemcpyAsync(done, d_done_.get<uint8_t>() + size_t(first_slot) * c, batch * c, hipMemcpyDeviceToHost, stream_));
  STAGE_TRY(hipStreamSynchronize(stream_));
  return 0;
}

}  // namespace ldpc
