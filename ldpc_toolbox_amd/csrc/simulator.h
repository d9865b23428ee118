// GPU-resident BER simulation step: generate frames -> decode -> count errors, all on the device.
// Host-side counterpart of the reference's BerTest / Worker (src/simulation/ber.rs:246-282, 297-368,
// 436-481) for BPSK and 8PSK (with the DVB-S2 bit interleaver) over AWGN; see frame_gen.hip.h for
// the frame definition.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "demodulator.h"
#include "device_bch.h"
#include "device_decoder.h"
#include "device_nr_qam.h"
#include "device_nr_rm.h"
#include "hip_owned.h"
#include "encoder.h"
#include "nr_harq.h"

namespace ldpc {

class Simulator {
 public:
  // pool: number of pre-encoded random messages frames draw their codeword from (the decoders are
  // symmetric, so the error statistics do not depend on which codewords are sent)
  static Simulator *create(const std::string &alist, const std::string &implementation,
                           const std::string &puncturing, int device, uint32_t pool, uint64_t pool_seed,
                           std::string *err);
  ~Simulator();

  size_t k() const { return k_; }
  size_t n() const { return n_; }
  size_t n_tx() const { return n_tx_; }
  uint32_t pool() const { return pool_; }
  double rate() const { return static_cast<double>(k_) / static_cast<double>(n_tx_); }  // ber.rs:259
  // modulation: 1 = BPSK, 3 = 8PSK (bits per symbol, factory.rs:53-73; 8PSK needs n_tx % 3 == 0).
  // interleaving: columns of the DVB-S2 bit interleaver, negative = rows read backwards, 0 = none
  // (ber.rs:250-252; needs n_tx % columns == 0).  Both return false on an unusable value.
  bool set_modulation(int bits_per_symbol);
  bool set_interleaving(int64_t columns);
  // A constellation (a copy of the one a demodulator handle holds) in place of what set_modulation selects; nullptr
  // returns to that.  BPSK: the BPSK generator.  A table: n_tx must be a multiple of its bits and its mean energy 1 within
  // 1e-6 (sim_constellation_error), else false with nothing changed.  max_log: the demapper's fold step.
  // The frames are then defined by composition: the LLRs are what the modulator, the AWGN channel (the run's seed, frame
  // numbers and sigma) and the f64 demapper of this constellation give on the pooled codewords, each rounded once to float.
  bool set_constellation(const Constellation *c, bool max_log);
  bool has_constellation() const { return use_constellation_; }
  bool max_log() const { return (use_constellation_ || use_nr_qam_) && max_log_; }
  int modulation() const {
    return use_nr_qam_ ? static_cast<int>(nr_qam_.qm) : use_constellation_ ? static_cast<int>(constellation_.bits) : bits_per_symbol_;
  }
  // An NR modulation (a copy of what an "nr5g-qam:QM" handle holds: nr_qam.h) in place of what set_modulation selects;
  // nullptr returns to that.  false with nothing changed unless n_tx is a multiple of QM and the interleaving is 0
  // (nrqam::sim_error).  It takes the place of a constellation of set_constellation, and set_constellation takes its place.
  // The frames are then defined by composition: the LLRs of a frame are what the NR mapper without scrambling, the AWGN
  // channel (the run's seed, frame number and sigma) and the f64 NR demapper give on the frame's pooled transmitted row,
  // each rounded once to float, in transmitted order.  A rate matcher's qm is not compared with QM.
  bool set_nr_qam(const nrqam::Config *c, bool max_log);
  bool has_nr_qam() const { return use_nr_qam_; }
  int64_t interleaving() const { return interleaving_; }
  // "fading_block": 0 (none, the default) or the symbols per gain of the Rayleigh block-fading channel with perfect CSI
  // (include/ldpc_toolbox.h, PART 10), up to 0x7fffffff; false with nothing changed outside that range.  While it is set the
  // channel between the NR mapper and the demapper of set_nr_qam is the fading channel, and the demapper takes each symbol's
  // own scale.  Without an NR modulation in force every run and generate call is refused (-1, counters untouched): the run,
  // not this setter.
  bool set_fading_block(int64_t symbols);
  uint32_t fading_block() const { return fading_block_; }
  // An outer BCH code (a copy of the one a BCH handle holds) in place of the genie of run_bch; nullptr returns to the
  // genie.  false with nothing changed unless the code's n is this simulator's k.
  bool set_bch(const bch::Code *c);
  bool has_bch() const { return bch_ != nullptr; }
  // 5G NR rate matching (nr_rate_match.h) between the pooled codewords and the channel; nullptr returns to none.
  // false with nothing changed unless the simulator was built with puncturing "", the configuration's n is this
  // simulator's n, it has no filler bits (the pool's messages are random in all k positions), (e, rv, qm) is a
  // transmission and e is a multiple of the modulation's bits per symbol and of |interleaving|.
  // While set, n_tx is e: the pool's transmitted rows are the rate-matched codewords, the generator's LLRs [frames][e]
  // are what it gives for those rows, and the decoder sees them recovered (combine = 0) to [frames][n].
  bool set_rate_match(const nrrm::Config *c, uint64_t e, uint32_t rv, uint32_t qm);
  bool has_rate_match() const { return rate_match_; }
  // A HARQ sequence (nr_harq.h): `transmissions` transmissions (e[t], rv[t]) of one qm.  It puts the simulator into the
  // state of set_rate_match(c, e[0], rv[0], qm) -- run, run_bch, generate and the pool are those of that call -- and keeps
  // the further transmissions for run_harq and generate_harq.  nullptr: set_rate_match(nullptr).  Every set_rate_match
  // call clears the further transmissions.  false with nothing changed when set_rate_match would refuse the first
  // transmission, when the sequence is none (nrharq::sequence_error), when the interleaving is not 0, or while 8PSK or a
  // table constellation is in force: the sequence's generators are the BPSK one and the NR modulation's.
  bool set_harq(const nrrm::Config *c, const uint64_t *e, const uint32_t *rv, uint32_t transmissions, uint32_t qm);
  const nrharq::Sequence &harq() const { return harq_; }
  DeviceDecoder *decoder() { return dec_.get(); }
  // straggler pooling (run_bch): 0 = every chunk runs the full iteration budget
  void set_pooling(bool on) {
    pooling_ = on;
    budget_valid_ = false;
  }
  uint64_t pooled_frames() const { return pooled_frames_; }
  // "soft_bits": 32 (float soft buffers, the default) or 8 -- run_harq alone then keeps its soft buffers as 8-bit soft bits
  // (include/ldpc_toolbox.h, PART 9).  false with nothing changed for any other value, and for 8 unless the decoder's
  // implementation is one of the 8-bit names.
  bool set_soft_bits(int64_t bits);
  int soft_bits() const { return soft_bits_; }
  const std::vector<uint8_t> &messages() const { return messages_; }
  const std::vector<uint8_t> &tx_bits() const { return tx_bits_; }
  const std::string &last_error() const { return error_; }

  // Frames [first_frame, first_frame + frames) at ebn0_db: returns the six counters of
  // sharding.COUNTER_FIELDS (frames, bit errors, frame errors, false decodes, total iterations,
  // iterations of the correct frames) for exactly these frames.
  int run(double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames, uint32_t max_iterations,
          uint64_t counters[6]);
  // The same with the outer-BCH accounting of ber.rs:328-337: counters[9] = the six above, then
  // BCH bit errors, BCH frame errors (frames with more than bch_max_errors bit errors) and the
  // iterations of the frames the BCH code corrects.
  // With a code set (set_bch) bch_max_errors must be its t (else -4, 0 included), and counters 6..8 come from the real
  // decoder; run() does not see the code.
  // Per frame, e = the frame's k hard decisions XOR its pooled message; the bounded-distance decoder runs on e -- by
  // linearity the outcome for EVERY transmitted BCH codeword, so the pool's messages need not be codewords --
  // residual = the weight of the first k_bch bits of its output; [6] += residual, [7] += residual > 0, [8] += the
  // frame's iterations when residual == 0.  A miscorrection adds errors, parity bits are not payload, and a frame
  // whose errors all lie in the parity is correct.
  int run_bch(double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames, uint32_t max_iterations,
              uint64_t bch_max_errors, uint64_t counters[9]);
  // The same frames' LLRs (host [frames][n_tx]) and pooled-codeword indices, for tests.
  int generate(double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames, float *llrs,
               uint32_t *pool_index);
  // The frames through the HARQ sequence of set_harq (nr_harq.h), all on the device.  Every frame is decoded after each of
  // its transmissions with the full max_iterations (the straggler budget has no part here), on the soft buffer recovered
  // from all of them so far, and stops at the first attempt that converges -- right or wrong -- or after the last one.
  // "soft_bits" 8: an attempt after transmission t is the generator's float row taken through Q, recovered on 8-bit soft
  // bits with saturating sums into the frame's int8 soft row (combine = t > 0), and decoded by the 8-bit input entry; the
  // stage pools hold [capacity][n] bytes.
  // The noise sigma is that of n_tx = E_0 for every transmission.  counters[6]: the fields of run() for each frame's
  // final attempt, the iterations summed over all its attempts (a failed one counts max_iterations).
  // per_tx[T][4], per transmission: attempts, frames that stopped because the attempt converged, of those with bit
  // errors, iterations of these attempts.  A frame's result depends on (seed, frame, configuration) alone.
  // "pooling" 1: the frames that go on wait in their next stage's pool and are decoded thousands at a time
  // (pooled_frames: the retransmission attempts); 0: every chunk's failures run through all stages before the next chunk.
  // -4 and zeroed counters without a sequence, with a BCH code set, or when the modulation no longer fits the sequence.
  int run_harq(double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames, uint32_t max_iterations, uint64_t counters[6],
               uint64_t *per_tx);
  // LLRs (host [frames][E_t]) of transmission t of the same frames, and their pooled-codeword indices, for tests.
  int generate_harq(double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames, uint32_t transmission, float *llrs,
                    uint32_t *pool_index);
  // rows per flush of stage t of the last run_harq call (a benchmark's figure)
  uint64_t harq_flushes(uint32_t t) const { return t < nrharq::kMaxTransmissions ? harq_flushes_[t] : 0; }
  uint64_t harq_flushed_rows(uint32_t t) const { return t < nrharq::kMaxTransmissions ? harq_flushed_rows_[t] : 0; }

 private:
  Simulator() = default;
  int ensure(size_t frames, size_t llr_rows);
  void noise_params(double ebn0_db, float *sigma, float *scale) const;
  double noise_sigma(double ebn0_db) const;
  void launch_generator(double ebn0_db, uint64_t seed, uint64_t first_frame, uint32_t frames, float *dst = nullptr);
  void launch_table_generator(double sigma, uint64_t seed, uint64_t first_frame, uint32_t frames, float *dst);
  bool fail(const std::string &m, hipError_t e = hipSuccess);

  std::unique_ptr<DeviceDecoder> dec_;
  Stream stream_;  // (declared before the buffers: destroyed after them)
  size_t k_ = 0, n_ = 0, n_tx_ = 0;
  uint32_t pool_ = 0;
  int device_ = 0;
  int bits_per_symbol_ = 1;
  bool use_constellation_ = false, max_log_ = false;
  Constellation constellation_;
  bool use_nr_qam_ = false;
  nrqam::Config nr_qam_;
  int64_t interleaving_ = 0;
  uint32_t fading_block_ = 0;
  const char *fading_error() const;
  std::vector<uint8_t> messages_, tx_bits_;
  DeviceBuffer d_messages_, d_tx_, d_bits_, d_llrs_, d_its_, d_counters_;
  // Straggler pooling: once a run() call has seen how many iterations its frames take, later chunks run a reduced
  // budget and the frames that have not converged by then are pooled and decoded together with the full budget --
  // instead of every chunk dragging its few slow (or failing) frames through launch-bound, nearly empty iterations
  // up to max_iterations.  Per frame the result is the one of a single full-budget decode (the decoder is
  // deterministic per frame and does not depend on the batch around it): identical counters.
  bool pooling_ = true;
  uint64_t pooled_frames_ = 0;
  bool budget_valid_ = false;  // the reduced budget the last call arrived at, and the point it belongs to
  uint32_t budget_ = 0, budget_max_it_ = 0;
  double budget_ebn0_ = 0.0;
  DeviceBuffer d_pool_llrs_, d_pool_frames_, d_pool_count_, d_pool_bits_, d_pool_its_;
  size_t pool_cap_ = 0;
  int ensure_pool(size_t capacity);
  int flush_pool(uint32_t count, uint64_t seed, uint32_t max_iterations, uint64_t bch_max_errors, bool real_bch, size_t chunk_group);
  int run_frames(double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames, uint32_t max_iterations,
                 uint64_t bch_max_errors, bool real_bch, uint64_t counters[9]);
  // the outer code of set_bch: the error patterns of a chunk (or of the pool) and what the decoder makes of them
  std::unique_ptr<DeviceBch> bch_;
  bch::Code bch_code_;
  DeviceBuffer d_bch_in_, d_bch_out_;
  // the rate matcher of set_rate_match: its plan, the generator's rows [chunk][n_tx] before recovery, and the pooled
  // codewords (what tx_bits_ holds while none is set)
  bool rate_match_ = false, punctured_ = false;
  nrrm::Plan rm_plan_{};
  DeviceBuffer d_rx_;
  std::vector<uint8_t> codewords_;
  int count_bch(const uint8_t *bits, const int32_t *its, uint64_t seed, uint64_t first_frame, uint32_t frames,
                uint32_t max_iterations, const uint64_t *frame_ids, int skip_failed);
  const char *rate_match_error(const nrrm::Config &c, uint64_t e, uint32_t rv, uint32_t qm) const;
  // the sequence of set_harq (t = 0: none), its configuration and plans, and every transmission's pooled transmitted rows
  // [pool][E_t], one after the other in d_harq_tx_ (transmission t at harq_.offset[t] * pool)
  nrharq::Sequence harq_;
  nrrm::Config harq_config_;
  nrrm::Plan harq_plans_[nrharq::kMaxTransmissions] = {};
  DeviceBuffer d_harq_tx_;
  // Stage pools: stage t = 1 .. T-1 holds the frames that wait for transmission t -- soft rows [capacity][n], frame
  // numbers and the iterations spent so far -- and the flush's own buffers are shared: the generated rows
  // [capacity][max E_t], decoded bits and iteration counts.  counts: one fill count per stage; per_tx: [T][4].
  struct HarqStage {
    DeviceBuffer soft, frames, spent;
  };
  HarqStage harq_stage_[nrharq::kMaxTransmissions];
  DeviceBuffer d_harq_rx_, d_harq_bits_, d_harq_its_, d_harq_counts_, d_harq_per_tx_;
  // "soft_bits" 8: the soft rows above are int8, and a generator's float rows (d_rx_ of stage 0, d_harq_rx_ of a flush) go
  // through Q in a pass of their own into these receive buffers, which rate recovery reads
  int soft_bits_ = 32;
  DeviceBuffer d_rx_i8_, d_harq_rx_i8_;
  void launch_quantize(const float *src, int8_t *dst, uint64_t total);
  size_t harq_cap_ = 0;
  uint64_t harq_flushes_[nrharq::kMaxTransmissions] = {}, harq_flushed_rows_[nrharq::kMaxTransmissions] = {};
  const char *harq_modulation_error() const;
  int ensure_harq(size_t capacity);
  void launch_harq_generator(double ebn0_db, uint64_t seed, uint32_t t, uint64_t first_frame, const uint64_t *frame_ids, uint32_t frames,
                             float *dst);
  int flush_harq(uint32_t t, uint32_t count, double ebn0_db, uint64_t seed, uint32_t max_iterations, size_t chunk);
  std::string error_;
};

}  // namespace ldpc
