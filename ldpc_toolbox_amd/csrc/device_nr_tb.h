// Batched 5G NR transport block CRC, segmentation and concatenation on the GPU: the device side of nrtb::Config
// (nr_transport_block.h), for the ldpc_toolbox_nr_tb_* entries of the C ABI.  The kernels are in kernels_nr_tb.hip.h; the
// host side (device_nr_tb.hip.h) is part of the simulator's translation unit, as the rate matcher is.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>

#include "device_stage.h"
#include "nr_transport_block.h"

namespace ldpc {

// code block rows of a pass of segment / desegment (one transport block when it has more): the grid of a launch
constexpr size_t kNrTbPassRows = size_t(1) << 22;
// elements of a pass of concatenate / split (one transport block when G is larger): the kernels index a pass below 2^31
constexpr size_t kNrTbPassElements = size_t(1) << 30;
// what a host entry stages on the device at a time: about this many bytes of its longest side
constexpr size_t kNrTbStageBytes = size_t(1) << 28;

class DeviceNrTb : public DeviceStage {
 public:
  // nullptr (and *err) when there is no usable GPU: there is no CPU path.
  static DeviceNrTb *create(const nrtb::Config &c, int device, std::string *err);
  ~DeviceNrTb();

  // Device pointers; 0, or -2 on a HIP failure.  stream: launch stream (nullptr = the handle's own stream, ordered after
  // everything queued on the legacy default stream at the time of the call, and synchronised on return).  The CRC parts
  // of a call live in a buffer of the handle: one call at a time per handle.
  // payload [batch][A] -> rows [C * batch][K]
  int segment_device(const uint8_t *payload, uint8_t *rows, size_t batch, hipStream_t stream);
  // rows [C * batch][K] -> payload [batch][A], tb_ok [batch], cb_ok [batch][C] (may be null)
  int desegment_device(const uint8_t *rows, uint8_t *payload, uint8_t *tb_ok, uint8_t *cb_ok, size_t batch, hipStream_t stream);
  // packed block-major rows -> [batch][G] bytes
  int concatenate_device(const uint8_t *packed, uint8_t *output, const nrtb::Lengths &l, size_t batch, hipStream_t stream);
  // [batch][G] floats or (f64) doubles -> packed block-major rows
  int split_device(const void *rx, void *packed, bool f64, const nrtb::Lengths &l, size_t batch, hipStream_t stream);
  // Host pointers: staged through device buffers of the handle, kNrTbStageBytes at a time, synchronous.
  int segment_host(const uint8_t *payload, uint8_t *rows, size_t batch);
  int desegment_host(const uint8_t *rows, uint8_t *payload, uint8_t *tb_ok, uint8_t *cb_ok, size_t batch);
  int concatenate_host(const uint8_t *packed, uint8_t *output, const nrtb::Lengths &l, size_t batch);
  int split_host(const void *rx, void *packed, bool f64, const nrtb::Lengths &l, size_t batch);

 private:
  explicit DeviceNrTb(int device) : DeviceStage("nr_tb", device) {}
  // block-major rows between a host array over `batch` transport blocks and a device array over `frames` of them
  int copy_rows(char *dst, const char *src, size_t blocks, size_t row_bytes, size_t batch, size_t b0, size_t frames, bool to_device);
  int copy_packed(char *dev, char *host, const nrtb::Lengths &l, size_t el, size_t batch, size_t b0, size_t frames, bool to_device);

  nrtb::Config c_;
  // (beside the stream and the staging buffers of DeviceStage)
  DeviceBuffer d_tables_;  // nrtb::device_tables
  DeviceBuffer d_part_;    // the CRC parts of a pass
  DeviceBuffer d_flags_;   // tb_ok and cb_ok of a stage
};

}  // namespace ldpc
