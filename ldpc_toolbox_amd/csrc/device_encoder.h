// Batched systematic encoder on the GPU: the device side of ldpc::Encoder (encoder.h), for the
// ldpc_toolbox_encoder_encode_batch* entries of the C ABI.  Per frame it computes exactly what
// Encoder::encode computes (GF(2): there is no tolerance), for many frames per call:
//   * staircase codes: row sums of H0 over the message, then the running XOR down the rows;
//   * every other code: parity = G0 * message with G0 dense and bit-packed;
//   * an optional puncturing step (keep the blocks of n / pattern.size() bytes whose entry is 1).
// The kernels are in kernels_encoder.hip.h; both headers are part of the simulator's translation unit.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>
#include <vector>

#include "encoder.h"
#include "device_stage.h"

namespace ldpc {

// LDS a stair_scan_kernel workgroup may ask for: the 160 KiB of a gfx950 CU less its static words
constexpr size_t kEncLdsBudget = 160 * 1024 - 1024;

// How a staircase code of k message bits is encoded (launch_staircase; "staircase_form" of ldpc_toolbox_encoder_get).
// A group's message words are staged in LDS, kp = k rounded up to 8 of them:
//   0: 32 frames per word while 4 * kp bytes fit;
//   1: 16 frames per word for the longest messages (DVB-S2 normal frames from rate 2/3 up);
//   2: a message too long even for that is gathered from global memory, 32 frames per word.
constexpr int staircase_form(size_t k) {
  const size_t kp = (k + 7) / 8 * 8;
  return kp * 4 <= kEncLdsBudget ? 0 : (kp * 2 <= kEncLdsBudget ? 1 : 2);
}

class DeviceEncoder : public DeviceStage {
 public:
  // Uploads the tables of `enc` to GPU `device`.  pattern: empty, or a pattern whose length divides n.
  // nullptr (and *err) when there is no usable GPU or an allocation fails: there is no CPU path here.
  static DeviceEncoder *create(const Encoder &enc, const std::vector<uint8_t> &pattern, int device, std::string *err);
  ~DeviceEncoder();

  size_t k() const { return k_; }
  size_t n() const { return n_; }
  size_t output_len() const { return out_len_; }

  // input [batch][k] (a byte equal to 1 is a one), output [batch][output_len] bytes 0/1.  0, or -2 on a HIP failure.
  // Device pointers; stream: launch stream (nullptr = the handle's own stream, ordered after everything queued on the
  // legacy default stream at the time of the call, and synchronised on return).
  int encode_device(const uint8_t *input, uint8_t *output, size_t batch, hipStream_t stream);
  // Host pointers: staged through device buffers of the handle, synchronous.
  int encode_host(const uint8_t *input, uint8_t *output, size_t batch);

 private:
  explicit DeviceEncoder(int device) : DeviceStage("encoder", device) {}
  int grow(DeviceBuffer &b, size_t need);
  int launch_staircase(const uint8_t *in, uint8_t *cw, size_t batch, hipStream_t s);
  int launch_dense(const uint8_t *in, uint8_t *cw, size_t batch, hipStream_t s);

  size_t k_ = 0, n_ = 0, m_ = 0, out_len_ = 0;
  bool staircase_ = false;
  size_t words_ = 0, m_pad_ = 0;
  uint32_t kept_ = 0, block_ = 0;
  // (beside the stream and the staging buffers of DeviceStage)
  // staircase: H0 in CSR form
  DeviceBuffer d_h0_ptr_, d_h0_idx_;
  // dense: G0 transposed, [words][m rounded up to 64] 64-bit words (a wave reads 64 rows of one word column at once)
  DeviceBuffer d_gen_t_;
  // puncturing: kept block j of the output is block d_keep_[j] of the codeword
  DeviceBuffer d_keep_;
  // work buffers, grown on demand: bit-packed messages, row-sum prefixes + slice totals, full codewords before puncturing
  DeviceBuffer d_packed_, d_prefix_, d_cw_;
};

}  // namespace ldpc
