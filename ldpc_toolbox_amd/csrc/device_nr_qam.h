// Batched 5G NR modulation mapper, soft demapper and scrambling on the GPU: the device side of nrqam::Config (nr_qam.h),
// for the ldpc_toolbox_nr_qam_* entries of the C ABI.  The kernels are in kernels_nr_qam.hip.h; the host side
// (device_nr_qam.hip.h) is part of the simulator's translation unit, as the demapper and the rate matcher are.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>

#include "device_stage.h"
#include "nr_qam.h"

namespace ldpc {

// The simulator's fused generator (nrqam::qam_llr_kernel), enqueued on `s`: frames [first_frame, first_frame + frames) of
// pooled transmitted rows tx [pool][n_tx] -> llrs [frames][n_tx] in transmitted order.  fading_block: 0 = AWGN, else the
// Rayleigh block-fading channel with one gain per that many symbols and the demapper with a scale per symbol.
void nr_qam_launch_generator(const nrqam::Config &c, bool max_log, const uint8_t *tx, uint32_t pool, uint32_t n_tx, uint64_t seed,
                             uint64_t first_frame, uint32_t frames, double sigma, uint32_t fading_block, float *llrs, hipStream_t s);

// One transmission of a HARQ sequence (nrqam::qam_llr_harq_kernel; nr_harq.h): tx [pool][e] are that transmission's pooled
// rows, row r of llrs [frames][e] is frame frame_ids[r] (a device array), or first_frame + r when it is nullptr, and
// symbol s takes the normal pair first_symbol + s -- and, with a fading_block, the gain of block (first_symbol + s) / fading_block.
void nr_qam_launch_harq_generator(const nrqam::Config &c, bool max_log, const uint8_t *tx, uint32_t pool, uint32_t e, uint32_t first_symbol,
                                  uint64_t seed, uint64_t first_frame, const uint64_t *frame_ids, uint32_t frames, double sigma,
                                  uint32_t fading_block, float *llrs, hipStream_t s);

class DeviceNrQam : public DeviceStage {
 public:
  // nullptr (and *err) when there is no usable GPU: there is no CPU path.
  static DeviceNrQam *create(const nrqam::Config &c, int device, std::string *err);
  ~DeviceNrQam();
  // how often the Gold kernel has run: a call with the (c_init, length) of the one before it does not run it again
  uint64_t sequence_launches() const { return sequence_launches_; }

  // bits [batch][bits_len] -> symbols [batch][symbols_len] (re, im), floats or (f64) doubles; the arguments already
  // checked (nrqam::mod_argument_error, device_pointer_error).  0, or -2 on a HIP failure.  Device pointers; stream:
  // launch stream (nullptr = the handle's own stream, ordered after everything queued on the legacy default stream at
  // the time of the call, and synchronised on return).
  int mod_device(const uint8_t *bits, void *symbols, bool f64, size_t bits_len, size_t symbols_len, size_t batch, int64_t c_init,
                 hipStream_t stream);
  // symbols -> llrs [batch][llrs_len] (nrqam::demod_argument_error)
  int demod_device(const void *symbols, void *llrs, bool f64, size_t symbols_len, size_t llrs_len, size_t batch, double sigma,
                   bool max_log, int64_t c_init, hipStream_t stream);
  // float symbols -> 8-bit soft bits [batch][llrs_len] (include/ldpc_toolbox.h, PART 9); llrs: any byte address
  int demap_i8_device(const float *symbols, int8_t *llrs, size_t symbols_len, size_t llrs_len, size_t batch, double sigma, bool max_log,
                      int64_t c_init, hipStream_t stream);
  int demap_i8_host(const float *symbols, int8_t *llrs, size_t symbols_len, size_t llrs_len, size_t batch, double sigma, bool max_log,
                    int64_t c_init);
  // The demappers with a scale per symbol (include/ldpc_toolbox.h, PART 10; nrqam::demap_csi_argument_error): scale
  // [batch][symbols_len] in the symbols' type, s = 1 / sigma_s^2 of each symbol, used as given.
  int demap_csi_device(const void *symbols, const void *scale, void *llrs, bool f64, size_t symbols_len, size_t llrs_len, size_t batch,
                       bool max_log, int64_t c_init, hipStream_t stream);
  int demap_csi_i8_device(const float *symbols, const float *scale, int8_t *llrs, size_t symbols_len, size_t llrs_len, size_t batch,
                          bool max_log, int64_t c_init, hipStream_t stream);
  // out_elem: the bytes of one LLR: 8 (double symbols), 4, or 1 (the 8-bit form)
  int demap_csi_host(const void *symbols, const void *scale, void *llrs, size_t out_elem, size_t symbols_len, size_t llrs_len, size_t batch,
                     bool max_log, int64_t c_init);
  // Host pointers: staged through device buffers of the handle, synchronous.
  int mod_host(const uint8_t *bits, void *symbols, bool f64, size_t bits_len, size_t symbols_len, size_t batch, int64_t c_init);
  int demod_host(const void *symbols, void *llrs, bool f64, size_t symbols_len, size_t llrs_len, size_t batch, double sigma,
                 bool max_log, int64_t c_init);
  // c(0 .. len-1) as the Gold kernel wrote it, one byte per bit (nrqam::sequence_argument_error)
  int sequence_host(uint8_t *c, size_t len, uint32_t c_init);

 private:
  explicit DeviceNrQam(int device) : DeviceStage("NR modulation", device) {}
  // DeviceStage::end, and before its wait the record of ev_gold_read_ behind a launch that read the sequence
  int end(hipStream_t stream, hipStream_t s, bool scrambled);
  // the sequence of (c_init, len) in d_gold_, generated on `s` unless it is the one already there: *c = its words, or
  // nullptr for c_init -1.  -2 on a HIP failure.
  int sequence(int64_t c_init, size_t len, hipStream_t s, const uint32_t **c);

  nrqam::Config c_;
  // (beside the stream and the staging buffers of DeviceStage)
  // the cached sequence: ceil(len / 32) + 1 words; the stream that generated it, the event behind that launch, and the
  // event behind the last launch that read it, with that launch's stream.  A reader on another stream waits for the
  // event before it takes it over, so the event is behind every earlier reader and a later generation waits for it alone.
  Event ev_gold_, ev_gold_read_;
  hipStream_t gold_stream_ = nullptr, gold_read_stream_ = nullptr;
  bool gold_valid_ = false, gold_read_ = false;
  int64_t gold_c_init_ = -1;
  size_t gold_len_ = 0;
  uint64_t sequence_launches_ = 0;
  DeviceBuffer d_gold_;
  DeviceBuffer d_scale_;  // the scales of demap_csi_host, beside d_in_ and d_out_
};

}  // namespace ldpc
