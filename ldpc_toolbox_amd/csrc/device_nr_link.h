// The 5G NR link handle on the GPU: the device side of nrlink::Config (nr_link.h), for the ldpc_toolbox_nr_link_* entries
// of the C ABI.  It owns one handle of every stage of the shared-channel chain -- transport block, encoder, rate matcher,
// modulation, decoder -- and drives their _device entries on one stream, with kernels of its own (kernels_nr_link.hip.h)
// for the fused rate recovery into the HARQ slots and for the gated decode.  The host side (device_nr_link.hip.h) is
// part of the simulator's translation unit, as the stages' are.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "device_stage.h"
#include "implementation.h"
#include "nr_link.h"

namespace ldpc {

class DeviceDecoder;
class DeviceEncoder;
class DeviceNrQam;
class DeviceNrRm;
class DeviceNrTb;

class DeviceNrLink : public DeviceStage {
 public:
  // Makes the five stage handles and `slots` HARQ slots on GPU `device`.  nullptr (and *err) when there is no usable GPU
  // or an allocation fails: there is no CPU path.  soft_bits: 32, or 8 (include/ldpc_toolbox.h, PART 12: an 8-bit
  // implementation) -- the slots' soft rows, the demapper output and the decoder input are then one byte per soft bit.
  static DeviceNrLink *create(const nrlink::Config &c, const Implementation &impl, uint32_t slots, uint32_t soft_bits, int device,
                              std::string *err);
  ~DeviceNrLink();

  // per call, by the C ABI's setters
  void set_max_log(bool v) { max_log_ = v; }
  void set_pass_elements(uint64_t v) { pass_elements_ = v; }
  void set_filler_llr(float v) { filler_ = v; }
  void set_filler_soft_bit(int32_t v) { filler_soft_bit_ = v; }  // Q(filler LLR), what an 8-bit handle writes
  uint64_t decoded_rows() const { return decoded_rows_; }
  uint64_t skipped_rows() const { return skipped_rows_; }
  bool soft_i8() const { return soft_bytes_ == 1; }
  // whether every slot of the range has been received into
  bool slots_used(uint32_t first_slot, size_t batch) const;

  // Device pointers; 0, or -2 on a HIP failure; the arguments already checked (nrlink::*_argument_error).  stream: launch
  // stream (nullptr = the handle's own stream, ordered after everything queued on the legacy default stream at the time
  // of the call, and synchronised on return).
  // payload [batch][A] -> symbols [batch][G / QM] (re, im) floats
  int transmit_device(const uint8_t *payload, float *symbols, size_t batch, uint32_t rv, int64_t c_init, hipStream_t stream);
  // symbols (and scale [batch][G / QM], or nullptr: noise_sigma) -> payload [batch][A], tb_ok [batch], and cb_ok,
  // iterations [batch][C] (each may be null), through the slots first_slot .. first_slot + batch - 1.  With `combine` the
  // host waits once, for the number of rows to decode.
  int receive_device(const float *symbols, const float *scale, uint8_t *payload, uint8_t *tb_ok, uint8_t *cb_ok, int32_t *iterations,
                     size_t batch, double noise_sigma, uint32_t rv, int64_t c_init, uint32_t first_slot, bool combine,
                     uint32_t max_iterations, hipStream_t stream);
  // Host pointers: symbols staged in and results out through buffers of the handle, synchronous.
  int transmit_host(const uint8_t *payload, float *symbols, size_t batch, uint32_t rv, int64_t c_init);
  int receive_host(const float *symbols, const float *scale, uint8_t *payload, uint8_t *tb_ok, uint8_t *cb_ok, int32_t *iterations,
                   size_t batch, double noise_sigma, uint32_t rv, int64_t c_init, uint32_t first_slot, bool combine,
                   uint32_t max_iterations);
  // host copies of the slots' state, block-major over the range: soft [C * batch][n] (floats, or int8 on an 8-bit handle),
  // done [batch][C], rows [C * batch][K] (each may be null)
  int slot_state_host(void *soft, uint8_t *done, uint8_t *rows, uint32_t first_slot, size_t batch);

  // the rate recovery of receive_device alone: rx [batch][G] LLRs in transmitted order (floats, or int8 at any byte address
  // on an 8-bit handle) -> the slots' soft rows
  int recover_device(const void *rx, size_t batch, uint32_t rv, uint32_t first_slot, bool combine, hipStream_t stream);

 private:
  DeviceNrLink(int device);
  // transport blocks a transmit call takes through the handle's buffers at a time
  size_t transmit_chunk() const;
  // the slots' reset (no combine) and the fused recover kernel, in passes, on `s`
  int recover_into_slots(const void *rx, size_t batch, uint32_t rv, uint32_t first_slot, bool combine, hipStream_t s);

  nrlink::Config c_;
  uint32_t slots_ = 0;
  size_t soft_bytes_ = sizeof(float);  // of one soft bit: 4, or 1
  bool max_log_ = false;
  uint64_t pass_elements_ = nrlink::kPassElements;
  float filler_ = 0.0f;
  int32_t filler_soft_bit_ = soft::kSoftMax;
  uint64_t decoded_rows_ = 0, skipped_rows_ = 0;
  std::vector<uint8_t> used_;  // [slots]: received into since the handle was made
  // (beside the stream and the staging buffers of DeviceStage)
  // the slots: soft rows [C * slots][n] floats (or int8), hard decisions [C * slots][K], iteration counts and done flags [slots][C]
  DeviceBuffer d_soft_, d_hard_, d_its_, d_done_;
  // transmit: code block rows, codewords, rate-matched rows, the transport blocks' G bits
  DeviceBuffer d_rows_, d_cws_, d_packed_, d_tx_;
  // receive: demapper LLRs [batch][G]; the rows to decode and their number; the decoder's input and outputs; the range's
  // hard decisions for desegment; flags of a host call
  DeviceBuffer d_llrs_, d_list_, d_count_, d_dec_in_, d_dec_bits_, d_dec_its_, d_bits_, d_flags_, d_scale_;
  // the stages (declared last: destroyed first, while the stream above still exists)
  std::unique_ptr<DeviceNrTb> tb_;
  std::unique_ptr<DeviceEncoder> enc_;
  std::unique_ptr<DeviceNrRm> rm_;
  std::unique_ptr<DeviceNrQam> qam_;
  std::unique_ptr<DeviceDecoder> dec_;
};

}  // namespace ldpc
