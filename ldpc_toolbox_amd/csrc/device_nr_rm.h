// Batched 5G NR rate matching and rate recovery on the GPU: the device side of nrrm::Config (nr_rate_match.h), for the
// ldpc_toolbox_nr_rm_* entries of the C ABI.  The kernels are in kernels_nr_rm.hip.h; the host side (device_nr_rm.hip.h)
// is part of the simulator's translation unit, as the BCH code and the demapper are.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>

#include "device_stage.h"
#include "nr_rate_match.h"

namespace ldpc {

// elements of a pass of a batched call (one frame when a row is longer): the kernels index a pass below 2^31
constexpr size_t kNrRmPassElements = size_t(1) << 30;
// what a host entry stages on the device at a time: about this many bytes of its longest rows
constexpr size_t kNrRmStageBytes = size_t(1) << 28;

// The launches of one transmission, enqueued on `s` (device pointers; any batch, in passes).  The handle's entries and
// the simulator use them.
void nr_rm_launch_match(const nrrm::Plan &p, const uint8_t *codewords, uint8_t *output, size_t batch, hipStream_t s);
template <typename T>
void nr_rm_launch_recover(const nrrm::Plan &p, const T *rx, T *llrs, size_t batch, T filler, bool combine, hipStream_t s);
// 8-bit soft bits with saturating sums (include/ldpc_toolbox.h, PART 9); filler in 1..127; any byte addresses
void nr_rm_launch_recover_i8(const nrrm::Plan &p, const int8_t *rx, int8_t *llrs, size_t batch, int32_t filler, bool combine, hipStream_t s);

class DeviceNrRm : public DeviceStage {
 public:
  // nullptr (and *err) when there is no usable GPU: there is no CPU path.
  static DeviceNrRm *create(const nrrm::Config &c, int device, std::string *err);
  ~DeviceNrRm();

  // codewords [batch][n] -> output [batch][e].  0, or -2 on a HIP failure.  Device pointers; stream: launch stream
  // (nullptr = the handle's own stream, ordered after everything queued on the legacy default stream at the time of the
  // call, and synchronised on return).  (e, rv, qm): accepted by nrrm::transmission_error.
  int match_device(const uint8_t *codewords, uint8_t *output, size_t batch, uint32_t e, uint32_t rv, uint32_t qm, hipStream_t stream);
  // rx [batch][e] -> llrs [batch][n], floats or (f64) doubles
  int recover_device(const void *rx, void *llrs, bool f64, size_t batch, uint32_t e, uint32_t rv, uint32_t qm, double filler_llr,
                     bool combine, hipStream_t stream);
  // rx [batch][e] -> llrs [batch][n], 8-bit soft bits
  int recover_i8_device(const int8_t *rx, int8_t *llrs, size_t batch, uint32_t e, uint32_t rv, uint32_t qm, int32_t filler, bool combine,
                        hipStream_t stream);
  // Host pointers: staged through device buffers of the handle, kNrRmStageBytes at a time, synchronous.  A HIP failure
  // in a later stage leaves the rows of the earlier ones written.
  int match_host(const uint8_t *codewords, uint8_t *output, size_t batch, uint32_t e, uint32_t rv, uint32_t qm);
  int recover_host(const void *rx, void *llrs, bool f64, size_t batch, uint32_t e, uint32_t rv, uint32_t qm, double filler_llr,
                   bool combine);
  int recover_i8_host(const int8_t *rx, int8_t *llrs, size_t batch, uint32_t e, uint32_t rv, uint32_t qm, int32_t filler, bool combine);

 private:
  explicit DeviceNrRm(int device) : DeviceStage("nr_rm", device) {}

  nrrm::Config c_;
};

}  // namespace ldpc
