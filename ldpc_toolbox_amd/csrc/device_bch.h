// Batched BCH encoder and bounded-distance decoder on the GPU: the device side of bch::Code (bch.h), for the
// ldpc_toolbox_bch_*_batch* entries of the C ABI.  The kernels are in kernels_bch.hip.h; the host side
// (device_bch.hip.h) is part of the simulator's translation unit, as the batched encoder and the demapper are.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>

#include "bch.h"
#include "device_stage.h"

namespace ldpc {

// frames per pass of a batched call: the lists of a pass are sized for it
constexpr size_t kBchPassFrames = 16384;
// what a host entry stages on the device at a time: at most this many frames and about this many bytes of input rows
constexpr size_t kBchStageFrames = size_t(1) << 20, kBchStageBytes = size_t(1) << 28;

class DeviceBch : public DeviceStage {
 public:
  // Uploads the tables of `c` to GPU `device`.  nullptr (and *err) when there is no usable GPU: there is no CPU path.
  static DeviceBch *create(const bch::Code &c, int device, std::string *err);
  ~DeviceBch();

  // input [batch][k] -> output [batch][n].  0, or -2 on a HIP failure.  Device pointers; stream: launch stream
  // (nullptr = the handle's own stream, ordered after everything queued on the legacy default stream at the time of
  // the call, and synchronised on return).
  int encode_device(const uint8_t *input, uint8_t *output, size_t batch, hipStream_t stream);
  // input [batch][n] -> output [batch][output_len] (output_len = k or n), errors [batch] or nullptr
  int decode_device(const uint8_t *input, uint8_t *output, size_t output_len, size_t batch, int32_t *errors, hipStream_t stream);
  // Host pointers: staged through device buffers of the handle, kBchStageFrames / kBchStageBytes at a time, synchronous.
  // A HIP failure in a later stage leaves the rows of the earlier ones written.
  int encode_host(const uint8_t *input, uint8_t *output, size_t batch);
  int decode_host(const uint8_t *input, uint8_t *output, size_t output_len, size_t batch, int32_t *errors);

 private:
  explicit DeviceBch(int device) : DeviceStage("bch", device) {}
  size_t stage_frames() const;

  bch::Code c_;
  bch::Geometry enc_geo_, dec_geo_;
  uint32_t g_top_[bch::kMaxParityWords] = {};
  // (beside the stream and the staging buffers of DeviceStage)
  DeviceBuffer d_antilog_, d_log_, d_enc_table_, d_dec_table_;
  // one pass's frames with a non-zero remainder, their number, their odd syndromes and their locators
  DeviceBuffer d_list_, d_count_, d_synd_, d_loc_;
  DeviceBuffer d_err_;  // the error counts of a stage of decode_host
};

}  // namespace ldpc
