#include "simulator.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "demodulator.hip.h"      // so does the batched soft demapper
#include "device_bch.hip.h"       // and the batched BCH code
#include "device_encoder.hip.h"  // the batched GPU encoder lives in this translation unit
#include "device_nr_qam.hip.h"    // the NR modulation mapper, demapper and scrambling
#include "device_nr_rm.hip.h"     // and the batched NR rate matcher
#include "device_nr_tb.hip.h"     // and the NR transport block CRCs, segmentation and concatenation
#include "device_nr_link.hip.h"   // and the NR link handle that drives those stages
#include "frame_gen.hip.h"
#include "implementation.h"
#include "sparse.h"

namespace ldpc {

bool Simulator::fail(const std::string &m, hipError_t e) {
  error_ = m;
  if (e != hipSuccess) error_ += std::string(": ") + hipGetErrorString(e);
  std::fprintf(stderr, "ldpc_toolbox (hip): simulator: %s\n", error_.c_str());
  return false;
}

#define SIM_TRY(expr)                 \
  do {                                \
    hipError_t _e = (expr);           \
    if (_e != hipSuccess) {           \
      fail(#expr, _e);                \
      return -2;                      \
    }                                 \
  } while (0)

Simulator *Simulator::create(const std::string &alist, const std::string &implementation,
                             const std::string &puncturing, int device, uint32_t pool, uint64_t pool_seed,
                             std::string *err) {
  auto bail = [&](const std::string &m) -> Simulator * {
    if (err) *err = m;
    return nullptr;
  };
  SparseMatrix h;
  std::string e;
  if (!SparseMatrix::from_alist(alist, &h, &e)) return bail(e);
  Implementation impl;
  if (!parse_implementation(implementation, &impl, &e)) return bail(e);
  std::vector<uint8_t> pattern;
  if (!parse_puncturing_pattern(puncturing, &pattern)) return bail("invalid puncturing pattern");
  Encoder enc;
  if (!Encoder::from_h(h, &enc, &e)) return bail(e);
  std::unique_ptr<Simulator> s(new Simulator());
  s->dec_.reset(DeviceDecoder::create(h, impl, pattern, device, &e));
  if (!s->dec_) return bail(e);
  // (run() reads the counters back right after every chunk: the decode calls may as well pace themselves on the
  // groups' progress instead of enqueuing every iteration up to max_iterations)
  (void)s->dec_->set_option("throttle", 1);
  s->device_ = device;
  s->n_ = h.num_cols();
  s->k_ = h.num_cols() - h.num_rows();
  s->n_tx_ = s->dec_->input_len();
  s->punctured_ = !pattern.empty();
  s->pool_ = std::max<uint32_t>(pool, 1);
  // the pool: random messages, systematic encode, puncture (puncturing.rs:47-75)
  std::mt19937_64 rng(pool_seed);
  s->messages_.resize(size_t(s->pool_) * s->k_);
  s->tx_bits_.resize(size_t(s->pool_) * s->n_tx_);
  std::vector<uint8_t> cw(s->n_);
  for (uint32_t p = 0; p < s->pool_; p++) {
    uint8_t *m = &s->messages_[size_t(p) * s->k_];
    for (size_t i = 0; i < s->k_; i += 64) {
      uint64_t w = rng();
      for (size_t j = i; j < std::min(i + 64, s->k_); j++, w >>= 1) m[j] = w & 1;
    }
    enc.encode(m, cw.data());
    uint8_t *tx = &s->tx_bits_[size_t(p) * s->n_tx_];
    if (pattern.empty()) {
      std::copy(cw.begin(), cw.end(), tx);
    } else {
      const size_t block = s->n_ / pattern.size();
      size_t j = 0;
      for (size_t b = 0; b < pattern.size(); b++)
        if (pattern[b]) std::copy(cw.begin() + b * block, cw.begin() + (b + 1) * block, tx + (j++) * block);
    }
  }
  if (hipSetDevice(device) != hipSuccess) return bail("hipSetDevice failed");
  bool ok = s->d_messages_.ensure(s->messages_.size()) == hipSuccess && s->d_tx_.ensure(s->tx_bits_.size()) == hipSuccess &&
            s->d_counters_.ensure(9 * sizeof(unsigned long long)) == hipSuccess &&
            hipMemcpy(s->d_messages_.get(), s->messages_.data(), s->messages_.size(), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(s->d_tx_.get(), s->tx_bits_.data(), s->tx_bits_.size(), hipMemcpyHostToDevice) == hipSuccess &&
            s->stream_.create() == hipSuccess;
  if (!ok) return bail("device allocation for the simulator failed");
  return s.release();
}

// (the members free what they own, the stream last and the decoder after it)
Simulator::~Simulator() {
  (void)hipSetDevice(device_);
  if (stream_) (void)hipStreamSynchronize(stream_);
}

// device buffers: LLR rows (one group's worth is enough for the streamed chunks), decoded bits and iteration counts
int Simulator::ensure(size_t frames, size_t llr_rows) {
  SIM_TRY(d_llrs_.ensure(llr_rows * dec_->input_len() * sizeof(float)));
  if (rate_match_) SIM_TRY(d_rx_.ensure(llr_rows * n_tx_ * sizeof(float)));
  SIM_TRY(d_bits_.ensure(frames * std::max<size_t>(k_, 1)));
  SIM_TRY(d_its_.ensure(frames * sizeof(int32_t)));
  return 0;
}

int Simulator::ensure_pool(size_t capacity) {
  if (capacity <= pool_cap_) return 0;
  pool_cap_ = 0;
  d_pool_count_ = DeviceBuffer();  // (its size is fixed: allocated anew with the others, as it always was)
  SIM_TRY(d_pool_llrs_.ensure(capacity * dec_->input_len() * sizeof(float)));
  SIM_TRY(d_pool_frames_.ensure(capacity * sizeof(uint64_t)));
  SIM_TRY(d_pool_count_.ensure(64));
  SIM_TRY(d_pool_bits_.ensure(capacity * std::max<size_t>(k_, 1)));
  SIM_TRY(d_pool_its_.ensure(capacity * sizeof(int32_t)));
  pool_cap_ = capacity;
  return 0;
}

// the pooled stragglers, with the full iteration budget (the stream is idle: the caller has just read the count)
int Simulator::flush_pool(uint32_t count, uint64_t seed, uint32_t max_iterations, uint64_t bch_max_errors, bool real_bch,
                          size_t chunk_group) {
  // (a call on the decoder's own stream: a handful of stragglers takes the single-launch small-batch path; a pool too
  // large for that is decoded in the chunks' group size, so that the decoder keeps the workspace it has -- a group
  // sized by the pool would free and re-allocate gigabytes before and after every flush)
  dec_->set_min_group(chunk_group);
  const int drc = dec_->decode_device(d_pool_llrs_.get(), LlrType::F32, count, max_iterations, d_pool_bits_.get<uint8_t>(), k_,
                                      d_pool_its_.get<int32_t>(), nullptr, nullptr);
  dec_->set_min_group(0);
  if (drc) {
    error_ = dec_->last_error();
    return drc;
  }
  gen::count_errors_kernel<<<(count * 64 + 255) / 256, 256, 0, stream_>>>(
      d_pool_bits_.get<uint8_t>(), static_cast<uint32_t>(k_), d_pool_its_.get<int32_t>(), d_messages_.get<uint8_t>(),
      static_cast<uint32_t>(k_), pool_, seed, 0, count, max_iterations, real_bch ? 0 : bch_max_errors,
      d_counters_.get<unsigned long long>(), d_pool_frames_.get<uint64_t>(), nullptr, 0);
  if (real_bch)
    if (int rc = count_bch(d_pool_bits_.get<uint8_t>(), d_pool_its_.get<int32_t>(), seed, 0, count, max_iterations,
                           d_pool_frames_.get<uint64_t>(), 0))
      return rc;
  SIM_TRY(hipMemsetAsync(d_pool_count_.get(), 0, sizeof(uint32_t), stream_));
  pooled_frames_ += count;
  return 0;
}

bool Simulator::set_modulation(int bits_per_symbol) {
  if (bits_per_symbol == 1 || (bits_per_symbol == 3 && n_tx_ % 3 == 0)) {
    bits_per_symbol_ = bits_per_symbol;
    budget_valid_ = false;  // (the iteration budget of straggler pooling belongs to one channel set-up)
    return true;
  }
  fail(bits_per_symbol == 3 ? "8PSK needs a transmitted length that is a multiple of 3 (modulation.rs:188-193)"
                            : "modulation must be 1 (BPSK) or 3 (8PSK)");
  return false;
}

bool Simulator::set_constellation(const Constellation *c, bool max_log) {
  if (c != nullptr) {
    if (const char *why = sim_constellation_error(*c, n_tx_)) {
      fail(why);
      return false;
    }
    constellation_ = *c;
  }
  use_constellation_ = c != nullptr;
  if (c != nullptr) use_nr_qam_ = false;  // (one takes the other's place)
  max_log_ = use_nr_qam_ ? max_log_ : c != nullptr && max_log;
  budget_valid_ = false;  // (as in set_modulation)
  return true;
}

bool Simulator::set_nr_qam(const nrqam::Config *c, bool max_log) {
  if (c != nullptr) {
    if (const char *why = nrqam::sim_error(*c, n_tx_, interleaving_)) {
      fail(why);
      return false;
    }
    nr_qam_ = *c;
    use_constellation_ = false;  // (one takes the other's place)
  }
  use_nr_qam_ = c != nullptr;
  max_log_ = use_constellation_ ? max_log_ : c != nullptr && max_log;
  budget_valid_ = false;  // (as in set_modulation)
  return true;
}

bool Simulator::set_bch(const bch::Code *c) {
  if (c != nullptr) {
    if (c->n != k_) {
      fail("the BCH code's n is not the LDPC code's k");
      return false;
    }
    std::string e;
    std::unique_ptr<DeviceBch> d(DeviceBch::create(*c, device_, &e));
    if (!d) {
      fail(e);
      return false;
    }
    bch_ = std::move(d);
    bch_code_ = *c;
  } else {
    bch_.reset();
    d_bch_in_ = DeviceBuffer();
    d_bch_out_ = DeviceBuffer();
  }
  budget_valid_ = false;  // (as in set_modulation)
  return true;
}

// nullptr, or why set_rate_match refuses transmission (e, rv, qm) of configuration c
const char *Simulator::rate_match_error(const nrrm::Config &c, uint64_t e, uint32_t rv, uint32_t qm) const {
  if (punctured_) return "rate matching needs a simulator built with puncturing \"\"";
  if (c.n != n_) return "the rate matcher's n is not the LDPC code's n";
  if (c.fillers != 0) return "the simulator takes no filler bits: its pooled messages are random in all k positions";
  if (const char *why = nrrm::transmission_error(e, rv, qm)) return why;
  if (e % static_cast<uint64_t>(modulation()) != 0) return "E must be a multiple of the modulation's bits per symbol";
  const uint64_t il = interleaving_ < 0 ? uint64_t(-interleaving_) : uint64_t(interleaving_);
  if (il != 0 && e % il != 0) return "E must be a multiple of the interleaver columns";
  return nullptr;
}

bool Simulator::set_rate_match(const nrrm::Config *c, uint64_t e, uint32_t rv, uint32_t qm) {
  auto refuse = [&](const char *why) {
    fail(why);
    return false;
  };
  if (c == nullptr && !rate_match_) return true;  // (no rate matcher: no HARQ sequence either)
  const std::vector<uint8_t> &cws = rate_match_ ? codewords_ : tx_bits_;
  std::vector<uint8_t> tx;
  nrrm::Plan plan{};
  if (c != nullptr) {
    if (const char *why = rate_match_error(*c, e, rv, qm)) return refuse(why);
    plan = nrrm::make_plan(*c, static_cast<uint32_t>(e), rv, qm);
    // the pool's transmitted rows: the rate-matched pooled codewords
    tx.resize(size_t(pool_) * e);
    for (uint32_t p = 0; p < pool_; p++)
      for (uint32_t pos = 0; pos < plan.e; pos++) tx[size_t(p) * e + pos] = cws[size_t(p) * n_ + nrrm::column_of_position(plan, pos)];
  } else {
    if (use_nr_qam_ && n_ % nr_qam_.qm != 0) return refuse("the codeword length is not a multiple of the NR modulation's QM: clear that first");
    tx = cws;
  }
  if (hipSetDevice(device_) != hipSuccess || hipStreamSynchronize(stream_) != hipSuccess) return refuse("the simulator's stream failed");
  DeviceBuffer d_tx;
  if (d_tx.ensure(tx.size()) != hipSuccess || hipMemcpy(d_tx.get(), tx.data(), tx.size(), hipMemcpyHostToDevice) != hipSuccess)
    return refuse("device allocation for the rate-matched pool failed");
  if (c != nullptr && !rate_match_) codewords_ = tx_bits_;
  d_tx_ = std::move(d_tx);
  tx_bits_ = std::move(tx);
  rate_match_ = c != nullptr;
  rm_plan_ = plan;
  n_tx_ = rate_match_ ? plan.e : n_;
  if (!rate_match_) {
    codewords_.clear();
    d_rx_ = DeviceBuffer();
  }
  // (a HARQ sequence belongs to the set_harq call that made it: any other rate matcher ends it)
  harq_ = nrharq::Sequence();
  d_harq_tx_ = DeviceBuffer();
  budget_valid_ = false;  // (as in set_modulation)
  return true;
}

// the sequence's generators are the BPSK one and the NR modulation's, both without an interleaver
const char *Simulator::harq_modulation_error() const {
  if (use_constellation_ && !constellation_.bpsk) return "HARQ takes BPSK or an NR modulation (set_nr_qam), not a table constellation";
  if (!use_constellation_ && !use_nr_qam_ && bits_per_symbol_ != 1) return "HARQ takes BPSK or an NR modulation (set_nr_qam), not 8PSK";
  if (interleaving_ != 0) return "HARQ takes no interleaving (NR's bit interleaver is the rate matcher's)";
  return nullptr;
}

bool Simulator::set_harq(const nrrm::Config *c, const uint64_t *e, const uint32_t *rv, uint32_t transmissions, uint32_t qm) {
  auto refuse = [&](const char *why) {
    fail(why);
    return false;
  };
  if (c == nullptr) return set_rate_match(nullptr, 0, 0, 1);
  if (const char *why = harq_modulation_error()) return refuse(why);
  if (const char *why = nrharq::sequence_error(e, rv, transmissions, qm, static_cast<uint32_t>(modulation()))) return refuse(why);
  if (const char *why = rate_match_error(*c, e[0], rv[0], qm)) return refuse(why);
  // every transmission's pooled rows, from the pooled codewords: made and uploaded before anything changes
  const nrharq::Sequence seq = nrharq::make_sequence(e, rv, transmissions, qm);
  const std::vector<uint8_t> &cws = rate_match_ ? codewords_ : tx_bits_;
  std::vector<uint8_t> tx(size_t(pool_) * seq.offset[seq.t]);
  nrrm::Plan plans[nrharq::kMaxTransmissions] = {};
  for (uint32_t t = 0; t < seq.t; t++) {
    plans[t] = nrharq::plan_of(*c, seq, t);
    uint8_t *rows = &tx[size_t(pool_) * seq.offset[t]];
    for (uint32_t p = 0; p < pool_; p++)
      for (uint32_t pos = 0; pos < seq.e[t]; pos++)
        rows[size_t(p) * seq.e[t] + pos] = cws[size_t(p) * n_ + nrrm::column_of_position(plans[t], pos)];
  }
  if (hipSetDevice(device_) != hipSuccess || hipStreamSynchronize(stream_) != hipSuccess) return refuse("the simulator's stream failed");
  DeviceBuffer d_tx;
  if (d_tx.ensure(tx.size()) != hipSuccess || hipMemcpy(d_tx.get(), tx.data(), tx.size(), hipMemcpyHostToDevice) != hipSuccess)
    return refuse("device allocation for the HARQ sequence's pooled rows failed");
  if (!set_rate_match(c, e[0], rv[0], qm)) return false;  // (it clears the sequence; what it refuses has been asked above)
  harq_ = seq;
  harq_config_ = *c;
  for (uint32_t t = 0; t < seq.t; t++) harq_plans_[t] = plans[t];
  d_harq_tx_ = std::move(d_tx);
  harq_cap_ = 0;  // (the stage pools are sized for a sequence: run_harq makes them anew)
  return true;
}

// counters 6..8 of `frames` decoded frames (bits [frames][k]) from the real outer decoder, on the simulator's stream
int Simulator::count_bch(const uint8_t *bits, const int32_t *its, uint64_t seed, uint64_t first_frame, uint32_t frames,
                         uint32_t max_iterations, const uint64_t *frame_ids, int skip_failed) {
  const uint32_t k = static_cast<uint32_t>(k_);
  // (run_frames has sized both for a chunk and for a full pool; a count beyond them is refused, never written)
  if (d_bch_in_.capacity() < size_t(frames) * k_ || d_bch_out_.capacity() < size_t(frames) * bch_code_.k) {
    fail("the BCH buffers are smaller than the frames to count");
    return -3;
  }
  gen::bch_pattern_kernel<<<(frames * 64 + 255) / 256, 256, 0, stream_>>>(bits, d_messages_.get<uint8_t>(), k, pool_, seed, first_frame,
                                                                         frames, d_bch_in_.get<uint8_t>(), frame_ids);
  if (bch_->decode_device(d_bch_in_.get<uint8_t>(), d_bch_out_.get<uint8_t>(), bch_code_.k, frames, nullptr, stream_)) {
    error_ = bch_->last_error();
    return -2;
  }
  gen::count_bch_kernel<<<(frames * 64 + 255) / 256, 256, 0, stream_>>>(d_bch_out_.get<uint8_t>(), bch_code_.k, its, frames, max_iterations,
                                                                       d_counters_.get<unsigned long long>(), skip_failed);
  return 0;
}

bool Simulator::set_interleaving(int64_t columns) {
  const uint64_t c = columns < 0 ? uint64_t(-columns) : uint64_t(columns);
  if (c > 0x7FFFFFFFull || (c != 0 && n_tx_ % c != 0)) {
    fail("interleaver columns must divide the transmitted length (interleaving.rs:44)");
    return false;
  }
  if (use_nr_qam_ && columns != 0) {
    fail("the NR mapper takes no interleaving (NR's bit interleaver is the rate matcher's)");
    return false;
  }
  interleaving_ = columns;
  budget_valid_ = false;
  return true;
}

bool Simulator::set_fading_block(int64_t symbols) {
  if (symbols < 0 || symbols > 0x7fffffffll) {
    fail("fading_block must be 0 (none) or 1 .. 2^31 - 1 symbols");
    return false;
  }
  fading_block_ = static_cast<uint32_t>(symbols);
  budget_valid_ = false;  // (as in set_modulation)
  return true;
}

// the fading channel lies between the NR mapper and its demapper: nullptr, or why a run is refused
const char *Simulator::fading_error() const {
  if (fading_block_ != 0 && !use_nr_qam_) return "fading_block needs an NR modulation in force (ldpc_toolbox_sim_set_nr_qam)";
  return nullptr;
}

// ber.rs:299-302: EsN0 = rate * bits_per_symbol * EbN0, sigma = sqrt(0.5 / EsN0)
double Simulator::noise_sigma(double ebn0_db) const {
  const double ebn0 = std::pow(10.0, 0.1 * ebn0_db);
  return std::sqrt(0.5 / (rate() * static_cast<double>(modulation()) * ebn0));
}

// BPSK: the f32 values the generator uses are the roundings of these doubles
void Simulator::noise_params(double ebn0_db, float *sigma, float *scale) const {
  const double s = noise_sigma(ebn0_db);
  *sigma = static_cast<float>(s);
  *scale = static_cast<float>(-2.0 / (s * s));
}

namespace {
template <int M>
void table_generator_pass(bool max_log, uint32_t blocks, hipStream_t s, const uint8_t *tx, uint32_t pool, uint32_t n_tx,
                          int32_t interleaving, uint64_t seed, uint64_t first_frame, uint64_t total, double sigma, double scale,
                          int32_t energy, const demod::Table<double> &t, float *dst) {
  if (max_log)
    chan::table_llr_kernel<M, true><<<blocks, chan::kThreads, 0, s>>>(tx, pool, n_tx, interleaving, seed, first_frame, total, sigma,
                                                                     scale, energy, t, dst);
  else
    chan::table_llr_kernel<M, false><<<blocks, chan::kThreads, 0, s>>>(tx, pool, n_tx, interleaving, seed, first_frame, total, sigma,
                                                                      scale, energy, t, dst);
}
}  // namespace

// the fused generator of a table constellation (kernels_channel.hip.h): scale and the energy terms as the demapper's
// host side makes them (demodulator.hip.h, demod_table_pass)
void Simulator::launch_table_generator(double sigma, uint64_t seed, uint64_t first_frame, uint32_t frames, float *dst) {
  const Constellation &c = constellation_;
  const uint32_t n_tx = static_cast<uint32_t>(n_tx_);
  const double scale = 1.0 / (sigma * sigma), half_scale = 0.5 * scale;
  demod::Table<double> t;
  for (uint32_t v = 0; v < 32; v++) {
    t.re[v] = c.re[v];
    t.im[v] = c.im[v];
    t.c[v] = half_scale * c.e[v];
  }
  const uint64_t total = uint64_t(frames) * (n_tx / c.bits);
  const uint32_t blocks = static_cast<uint32_t>((total + chan::kThreads - 1) / chan::kThreads);
  const uint8_t *tx = d_tx_.get<uint8_t>();
  const int32_t il = static_cast<int32_t>(interleaving_), energy = c.energy ? 1 : 0;
  switch (c.bits) {
    case 1: return table_generator_pass<1>(max_log_, blocks, stream_, tx, pool_, n_tx, il, seed, first_frame, total, sigma, scale, energy, t, dst);
    case 2: return table_generator_pass<2>(max_log_, blocks, stream_, tx, pool_, n_tx, il, seed, first_frame, total, sigma, scale, energy, t, dst);
    case 3: return table_generator_pass<3>(max_log_, blocks, stream_, tx, pool_, n_tx, il, seed, first_frame, total, sigma, scale, energy, t, dst);
    case 4: return table_generator_pass<4>(max_log_, blocks, stream_, tx, pool_, n_tx, il, seed, first_frame, total, sigma, scale, energy, t, dst);
    default: return table_generator_pass<5>(max_log_, blocks, stream_, tx, pool_, n_tx, il, seed, first_frame, total, sigma, scale, energy, t, dst);
  }
}

// frames [first_frame, first_frame + frames) -> d_llrs_ (codeword order, ready for the decoder), or with a rate matcher
// -> d_rx_ (transmitted order, to be recovered)
void Simulator::launch_generator(double ebn0_db, uint64_t seed, uint64_t first_frame, uint32_t frames, float *dst) {
  const uint32_t n_tx = static_cast<uint32_t>(n_tx_);
  if (dst == nullptr) dst = rate_match_ ? d_rx_.get<float>() : d_llrs_.get<float>();
  if (use_nr_qam_) {
    nr_qam_launch_generator(nr_qam_, max_log_, d_tx_.get<uint8_t>(), pool_, n_tx, seed, first_frame, frames, noise_sigma(ebn0_db), fading_block_,
                            dst, stream_);
    return;
  }
  if (use_constellation_ && !constellation_.bpsk) {
    launch_table_generator(noise_sigma(ebn0_db), seed, first_frame, frames, dst);
    return;
  }
  if (!use_constellation_ && bits_per_symbol_ == 3) {
    const double s = noise_sigma(ebn0_db);
    const uint64_t threads = uint64_t(frames) * (n_tx / 3);
    gen::psk8_llr_kernel<<<static_cast<uint32_t>((threads + 255) / 256), 256, 0, stream_>>>(
        d_tx_.get<uint8_t>(), pool_, n_tx, static_cast<int32_t>(interleaving_), seed, first_frame, frames, s, 1.0 / (s * s), dst);
    return;
  }
  // BPSK: one LLR per bit, so interleaving followed by deinterleaving changes nothing but which
  // noise sample a position gets; the generator keys the noise by codeword position
  float sigma, scale;
  noise_params(ebn0_db, &sigma, &scale);
  const uint64_t threads = uint64_t(frames) * ((n_tx + 1) / 2);
  gen::awgn_llr_kernel<<<static_cast<uint32_t>((threads + 255) / 256), 256, 0, stream_>>>(
      d_tx_.get<uint8_t>(), pool_, n_tx, seed, first_frame, frames, sigma, scale, dst);
}

int Simulator::run(double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames, uint32_t max_iterations,
                   uint64_t counters[6]) {
  if (const char *why = fading_error()) return fail(why), -1;
  uint64_t all[9];
  const int rc = run_frames(ebn0_db, seed, first_frame, frames, max_iterations, 0, false, all);
  for (int i = 0; i < 6; i++) counters[i] = all[i];
  return rc;
}

int Simulator::run_bch(double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames, uint32_t max_iterations,
                       uint64_t bch_max_errors, uint64_t counters[9]) {
  if (const char *why = fading_error()) return fail(why), -1;
  if (bch_ && bch_max_errors != bch_code_.t) {
    for (int i = 0; i < 9; i++) counters[i] = 0;
    fail("bch_max_errors is not the t of the BCH code in force");
    return -4;
  }
  return run_frames(ebn0_db, seed, first_frame, frames, max_iterations, bch_max_errors, bch_ != nullptr, counters);
}

// real_bch: counters 6..8 from the decoder of set_bch; else from the genie when bch_max_errors > 0
int Simulator::run_frames(double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames, uint32_t max_iterations,
                          uint64_t bch_max_errors, bool real_bch, uint64_t counters[9]) {
  for (int i = 0; i < 9; i++) counters[i] = 0;
  if (frames == 0) return 0;
  SIM_TRY(hipSetDevice(device_));
  // a chunk is one group of the decoder -- 4096 frames, more for small graphs
  const size_t chunk = std::min<size_t>(frames, std::max<size_t>(dec_->preferred_group(frames), 4096));
  if (int rc = ensure(chunk, chunk)) return rc;
  SIM_TRY(hipMemsetAsync(d_counters_.get(), 0, 9 * sizeof(unsigned long long), stream_));
  // straggler pooling (simulator.h): from the second chunk on, when the frames seen so far converge well within the budget
  const bool track = pooling_ && max_iterations >= 24;
  const bool can_pool = track && (frames > chunk || (budget_valid_ && budget_ebn0_ == ebn0_db && budget_max_it_ == max_iterations));
  pooled_frames_ = 0;
  if (can_pool) {
    if (int rc = ensure_pool(2 * chunk)) return rc;
    SIM_TRY(hipMemsetAsync(d_pool_count_.get(), 0, sizeof(uint32_t), stream_));
  }
  if (real_bch) {  // the patterns of a chunk, or of a full pool -- whose capacity an earlier call with larger chunks may have left
    const size_t rows = can_pool ? std::max(pool_cap_, chunk) : chunk;
    SIM_TRY(d_bch_in_.ensure(rows * k_));
    SIM_TRY(d_bch_out_.ensure(rows * bch_code_.k));
  }
  // (a sweep calls run() again and again at one Eb/N0: the budget the previous call arrived at carries over)
  const bool same_point = can_pool && budget_valid_ && budget_ebn0_ == ebn0_db && budget_max_it_ == max_iterations;
  uint32_t budget = same_point ? std::min(budget_, max_iterations) : max_iterations;
  uint32_t next_call_budget = budget;
  const size_t chunk_group = dec_->preferred_group(chunk);
  // The next chunk's budget from the counters so far: twice the average iteration count of the frames that converge,
  // plus 8 -- where a frame still waiting in the pool counts with the budget it has exhausted (a lower bound; left out,
  // the average would cover only the frames that beat the budget and ratchet it down) -- and the full budget again when
  // more than a quarter of the call's frames have needed the second pass (pooled now, flushed earlier, or failed
  // outright in a full-budget chunk): then pooling decodes too much twice.
  auto next_budget = [&](const unsigned long long c[9], uint32_t pooled, uint32_t used_budget, uint32_t max_it) -> uint32_t {
    const double counted = static_cast<double>(c[0]), clean = counted - static_cast<double>(c[2]);
    const double total_its_failed = static_cast<double>(c[4]) - static_cast<double>(c[5]);
    const double failed_full = std::min(static_cast<double>(c[2]), total_its_failed / std::max<double>(max_it, 1));
    const double second_pass = static_cast<double>(pooled) + static_cast<double>(pooled_frames_) + failed_full;
    const double ok_frames = clean + pooled, ok_its = static_cast<double>(c[5]) + static_cast<double>(pooled) * used_budget;
    const double avg_ok = ok_frames > 0 ? ok_its / ok_frames : static_cast<double>(max_it);
    uint32_t next = static_cast<uint32_t>(std::min<double>(max_it, std::ceil(2.0 * avg_ok) + 8.0));
    next = std::max<uint32_t>(next, 16);
    if (second_pass > 0.25 * (counted + pooled) || next * 10 >= max_it * 7) next = max_it;  // nothing to gain
    return next;
  };
  for (size_t f0 = 0; f0 < frames; f0 += chunk) {
    const uint32_t nf = static_cast<uint32_t>(std::min(chunk, frames - f0));
    launch_generator(ebn0_db, seed, first_frame + f0, nf);
    if (rate_match_) nr_rm_launch_recover<float>(rm_plan_, d_rx_.get<float>(), d_llrs_.get<float>(), nf, 0.0f, false, stream_);
    if (int rc = dec_->decode_device(d_llrs_.get(), LlrType::F32, nf, budget, d_bits_.get<uint8_t>(), k_, d_its_.get<int32_t>(), nullptr, stream_)) {
      error_ = dec_->last_error();
      return rc;
    }
    const bool reduced = budget < max_iterations;
    if (reduced)
      gen::straggler_collect_kernel<<<(nf * 64 + 255) / 256, 256, 0, stream_>>>(
          d_its_.get<int32_t>(), nf, first_frame + f0, d_llrs_.get<float>(), static_cast<uint32_t>(dec_->input_len()), d_pool_llrs_.get<float>(),
          d_pool_frames_.get<uint64_t>(), d_pool_count_.get<uint32_t>(),
          static_cast<uint32_t>(pool_cap_));
    gen::count_errors_kernel<<<(nf * 64 + 255) / 256, 256, 0, stream_>>>(
        d_bits_.get<uint8_t>(), static_cast<uint32_t>(k_), d_its_.get<int32_t>(), d_messages_.get<uint8_t>(), static_cast<uint32_t>(k_),
        pool_, seed, first_frame + f0, nf, max_iterations, real_bch ? 0 : bch_max_errors, d_counters_.get<unsigned long long>(),
        nullptr, nullptr, reduced ? 1 : 0);
    if (real_bch)
      if (int rc = count_bch(d_bits_.get<uint8_t>(), d_its_.get<int32_t>(), seed, first_frame + f0, nf, max_iterations, nullptr,
                             reduced ? 1 : 0))
        return rc;
    if (can_pool) {
      // what the frames of this call have needed so far decides the next chunk's budget (a call that cannot pool -- a
      // single chunk at a new point -- reads the counters once, at the end: no synchronisation between its launches)
      unsigned long long c[9];
      uint32_t pooled = 0;
      SIM_TRY(hipMemcpyAsync(c, d_counters_.get(), sizeof(c), hipMemcpyDeviceToHost, stream_));
      SIM_TRY(hipMemcpyAsync(&pooled, d_pool_count_.get(), sizeof(pooled), hipMemcpyDeviceToHost, stream_));
      SIM_TRY(hipStreamSynchronize(stream_));
      if (pooled > pool_cap_) {
        fail("straggler pool overflow");
        return -3;
      }
      const uint32_t next = next_budget(c, pooled, budget, max_iterations);
      budget = next;
      next_call_budget = next;
      if (f0 + chunk < frames && pooled + chunk > pool_cap_) {
        if (int rc = flush_pool(pooled, seed, max_iterations, bch_max_errors, real_bch, chunk_group)) return rc;
      }
    }
  }
  if (can_pool) {
    budget_valid_ = true;
    budget_ = next_call_budget;
    budget_ebn0_ = ebn0_db;
    budget_max_it_ = max_iterations;
  }
  if (can_pool) {
    uint32_t pooled = 0;
    SIM_TRY(hipMemcpyAsync(&pooled, d_pool_count_.get(), sizeof(pooled), hipMemcpyDeviceToHost, stream_));
    SIM_TRY(hipStreamSynchronize(stream_));
    if (pooled > pool_cap_) {
      fail("straggler pool overflow");
      return -3;
    }
    if (pooled)
      if (int rc = flush_pool(pooled, seed, max_iterations, bch_max_errors, real_bch, chunk_group)) return rc;
  }
  unsigned long long host[9];
  SIM_TRY(hipMemcpyAsync(host, d_counters_.get(), sizeof(host), hipMemcpyDeviceToHost, stream_));
  SIM_TRY(hipStreamSynchronize(stream_));
  SIM_TRY(hipGetLastError());
  if (track && !can_pool) {  // every frame of this call ran the full budget: what they needed is the next call's estimate
    budget_valid_ = true;
    budget_ = next_budget(host, 0, max_iterations, max_iterations);
    budget_ebn0_ = ebn0_db;
    budget_max_it_ = max_iterations;
  }
  for (int i = 0; i < 9; i++) counters[i] = host[i];
  return 0;
}

int Simulator::generate(double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames, float *llrs,
                        uint32_t *pool_index) {
  if (const char *why = fading_error()) return fail(why), -1;
  if (frames == 0) return 0;
  SIM_TRY(hipSetDevice(device_));
  // `llrs` in this GPU's memory: the frames are generated in place (a multi-rank benchmark fills its gigabyte of frames
  // without a round trip through pageable host memory); anywhere else: generated here and copied out
  hipPointerAttribute_t attr{};
  const bool on_device = hipPointerGetAttributes(&attr, llrs) == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device == device_;
  (void)hipGetLastError();  // (an ordinary host pointer is "invalid value" to the query on some runtimes)
  if (on_device) {
    launch_generator(ebn0_db, seed, first_frame, static_cast<uint32_t>(frames), llrs);
  } else {
    if (int rc = ensure(0, frames)) return rc;
    launch_generator(ebn0_db, seed, first_frame, static_cast<uint32_t>(frames));
    SIM_TRY(hipMemcpyAsync(llrs, rate_match_ ? d_rx_.get() : d_llrs_.get(), frames * n_tx_ * sizeof(float), hipMemcpyDefault, stream_));
  }
  SIM_TRY(hipStreamSynchronize(stream_));
  SIM_TRY(hipGetLastError());
  if (pool_index)
    for (size_t f = 0; f < frames; f++) pool_index[f] = gen::pool_index(seed, first_frame + f, pool_);
  return 0;
}

// ---- HARQ (nr_harq.h) ------------------------------------------------------------------------------------------------

// transmission t of `frames` frames -- frame_ids (device), or first_frame on -- into dst [frames][E_t], transmitted order
void Simulator::launch_harq_generator(double ebn0_db, uint64_t seed, uint32_t t, uint64_t first_frame, const uint64_t *frame_ids,
                                      uint32_t frames, float *dst) {
  const uint32_t e = harq_.e[t];
  const uint8_t *tx = d_harq_tx_.get<uint8_t>() + size_t(pool_) * harq_.offset[t];
  if (use_nr_qam_) {
    nr_qam_launch_harq_generator(nr_qam_, max_log_, tx, pool_, e, nrharq::first_symbol(harq_, t, nr_qam_.qm), seed, first_frame, frame_ids,
                                 frames, noise_sigma(ebn0_db), fading_block_, dst, stream_);
    return;
  }
  float sigma, scale;
  noise_params(ebn0_db, &sigma, &scale);
  const uint32_t pairs = nrharq::pairs(harq_, t);
  const uint64_t threads = uint64_t(frames) * pairs;
  gen::awgn_llr_harq_kernel<<<static_cast<uint32_t>((threads + 255) / 256), 256, 0, stream_>>>(tx, pool_, e, harq_.offset[t], pairs, seed,
                                                                                              first_frame, frame_ids, frames, sigma, scale, dst);
}

bool Simulator::set_soft_bits(int64_t bits) {
  if (bits != 8 && bits != 32) return fail("soft_bits must be 8 or 32");
  if (bits == 8 && !dec_->implementation().i8) return fail("soft_bits 8 needs one of the 8-bit implementations");
  if (soft_bits_ != bits) harq_cap_ = 0;  // (the stage pools are laid out anew by the next run_harq call)
  soft_bits_ = static_cast<int>(bits);
  return true;
}

void Simulator::launch_quantize(const float *src, int8_t *dst, uint64_t total) {
  gen::quantize_i8_kernel<<<static_cast<uint32_t>(((total + 3) / 4 + 255) / 256), 256, 0, stream_>>>(src, dst, total);
}

int Simulator::ensure_harq(size_t capacity) {
  const uint32_t T = harq_.t;
  const size_t soft_elem = soft_bits_ == 8 ? sizeof(int8_t) : sizeof(float);
  uint32_t max_e = 1;
  for (uint32_t t = 1; t < T; t++) max_e = std::max(max_e, harq_.e[t]);
  SIM_TRY(d_harq_counts_.ensure(nrharq::kMaxTransmissions * sizeof(uint32_t)));
  SIM_TRY(d_harq_per_tx_.ensure(nrharq::kMaxTransmissions * 4 * sizeof(unsigned long long)));
  harq_cap_ = 0;
  for (uint32_t t = 1; t < T; t++) {
    SIM_TRY(harq_stage_[t].soft.ensure(capacity * n_ * soft_elem));
    SIM_TRY(harq_stage_[t].frames.ensure(capacity * sizeof(uint64_t)));
    SIM_TRY(harq_stage_[t].spent.ensure(capacity * sizeof(uint32_t)));
  }
  if (T > 1) {
    SIM_TRY(d_harq_rx_.ensure(capacity * max_e * sizeof(float)));
    if (soft_bits_ == 8) SIM_TRY(d_harq_rx_i8_.ensure(capacity * max_e));
    SIM_TRY(d_harq_bits_.ensure(capacity * std::max<size_t>(k_, 1)));
    SIM_TRY(d_harq_its_.ensure(capacity * sizeof(int32_t)));
  }
  harq_cap_ = capacity;
  return 0;
}

// Stage t's pool: transmission t of its `count` frames, combined into their soft rows in place, decoded with the full
// budget, counted, and the ones that still fail appended to stage t + 1.  Stage t's count returns to zero.
// The decode calls are the chunks' own: `chunk` rows each, the rows behind the last pooled one set to the LLRs of the
// all-zero codeword, which converge at once.  A call of another size makes the decoder lay out its workspace anew --
// gigabytes freed and allocated before and after every flush, which on a busy device takes longer than the flush.
int Simulator::flush_harq(uint32_t t, uint32_t count, double ebn0_db, uint64_t seed, uint32_t max_iterations, size_t chunk) {
  HarqStage &st = harq_stage_[t];
  const bool last = t + 1 == harq_.t;
  uint32_t *counts = d_harq_counts_.get<uint32_t>();
  const bool soft8 = soft_bits_ == 8;
  const size_t soft_elem = soft8 ? sizeof(int8_t) : sizeof(float);
  launch_harq_generator(ebn0_db, seed, t, 0, st.frames.get<uint64_t>(), count, d_harq_rx_.get<float>());
  if (soft8) {
    launch_quantize(d_harq_rx_.get<float>(), d_harq_rx_i8_.get<int8_t>(), uint64_t(count) * harq_.e[t]);
    nr_rm_launch_recover_i8(harq_plans_[t], d_harq_rx_i8_.get<int8_t>(), st.soft.get<int8_t>(), count, soft::kSoftMax, true, stream_);
  } else {
    nr_rm_launch_recover<float>(harq_plans_[t], d_harq_rx_.get<float>(), st.soft.get<float>(), count, 0.0f, true, stream_);
  }
  const size_t padded = (count + chunk - 1) / chunk * chunk;  // (at most the two chunks every pool has room for)
  if (padded > count)
    SIM_TRY(hipMemsetAsync(st.soft.get<char>() + size_t(count) * n_ * soft_elem,
                           0x41 /* every float 0x41414141 = +12.08, every soft bit +65 steps */, (padded - count) * n_ * soft_elem, stream_));
  for (size_t p0 = 0; p0 < padded; p0 += chunk)
    if (int rc = dec_->decode_device(st.soft.get<char>() + p0 * n_ * soft_elem, soft8 ? LlrType::I8 : LlrType::F32, chunk, max_iterations,
                                     d_harq_bits_.get<uint8_t>() + p0 * k_, k_, d_harq_its_.get<int32_t>() + p0, nullptr, stream_)) {
      error_ = dec_->last_error();
      return rc;
    }
  if (!last && soft8) {
    HarqStage &next = harq_stage_[t + 1];
    gen::harq_collect_i8_kernel<<<(count * 64 + 255) / 256, 256, 0, stream_>>>(
        d_harq_its_.get<int32_t>(), count, 0, st.frames.get<uint64_t>(), st.spent.get<uint32_t>(), max_iterations, st.soft.get<uint32_t>(),
        static_cast<uint32_t>(n_ / 4), next.soft.get<uint32_t>(), next.frames.get<uint64_t>(), next.spent.get<uint32_t>(), counts + t + 1,
        static_cast<uint32_t>(2 * chunk));
  } else if (!last) {
    HarqStage &next = harq_stage_[t + 1];
    gen::harq_collect_kernel<<<(count * 64 + 255) / 256, 256, 0, stream_>>>(
        d_harq_its_.get<int32_t>(), count, 0, st.frames.get<uint64_t>(), st.spent.get<uint32_t>(), max_iterations, st.soft.get<float>(),
        static_cast<uint32_t>(n_), next.soft.get<float>(), next.frames.get<uint64_t>(), next.spent.get<uint32_t>(), counts + t + 1,
        static_cast<uint32_t>(2 * chunk));
  }
  gen::harq_count_kernel<<<(count * 64 + 255) / 256, 256, 0, stream_>>>(
      d_harq_bits_.get<uint8_t>(), d_harq_its_.get<int32_t>(), d_messages_.get<uint8_t>(), static_cast<uint32_t>(k_), pool_, seed, 0,
      st.frames.get<uint64_t>(), st.spent.get<uint32_t>(), count, max_iterations, last ? 1 : 0, d_counters_.get<unsigned long long>(),
      d_harq_per_tx_.get<unsigned long long>() + 4 * t);
  SIM_TRY(hipMemsetAsync(counts + t, 0, sizeof(uint32_t), stream_));
  harq_flushes_[t]++;
  harq_flushed_rows_[t] += count;
  pooled_frames_ += pooling_ ? count : 0;
  return 0;
}

int Simulator::run_harq(double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames, uint32_t max_iterations, uint64_t counters[6],
                        uint64_t *per_tx) {
  if (const char *why = fading_error()) return fail(why), -1;
  const uint32_t T = harq_.t;
  for (int i = 0; i < 6; i++) counters[i] = 0;
  for (uint32_t i = 0; i < 4 * T; i++) per_tx[i] = 0;
  auto refuse = [&](const char *why) {
    fail(why);
    return -4;
  };
  if (T == 0) return refuse("no HARQ sequence is set (ldpc_toolbox_sim_set_harq)");
  if (bch_) return refuse("a HARQ run takes no outer BCH code: clear it first");
  // (the modulation may have changed since set_harq)
  if (const char *why = harq_modulation_error()) return refuse(why);
  for (uint32_t t = 0; t < T; t++)
    if (harq_.e[t] % static_cast<uint32_t>(modulation()) != 0) return refuse("every E must be a multiple of the modulation's bits per symbol");
  pooled_frames_ = 0;
  for (uint32_t t = 0; t < nrharq::kMaxTransmissions; t++) harq_flushes_[t] = harq_flushed_rows_[t] = 0;
  if (frames == 0) return 0;
  SIM_TRY(hipSetDevice(device_));
  const size_t chunk = std::min<size_t>(frames, std::max<size_t>(dec_->preferred_group(frames), 4096));  // (as in run_frames)
  if (int rc = ensure(chunk, chunk)) return rc;
  const bool soft8 = soft_bits_ == 8;
  if (soft8 && n_ % 4 != 0) return refuse("soft_bits 8 needs a codeword length that is a multiple of 4");  // (every NR code's is)
  if (soft8) SIM_TRY(d_rx_i8_.ensure(chunk * n_tx_));
  if (harq_cap_ < 2 * chunk)
    if (int rc = ensure_harq(2 * chunk)) return rc;
  const size_t cap = 2 * chunk;  // (of this call: an earlier one with larger chunks may have left larger buffers)
  unsigned long long *d_counters = d_counters_.get<unsigned long long>(), *d_per_tx = d_harq_per_tx_.get<unsigned long long>();
  uint32_t *d_counts = d_harq_counts_.get<uint32_t>();
  SIM_TRY(hipMemsetAsync(d_counters, 0, 9 * sizeof(unsigned long long), stream_));
  SIM_TRY(hipMemsetAsync(d_per_tx, 0, nrharq::kMaxTransmissions * 4 * sizeof(unsigned long long), stream_));
  SIM_TRY(hipMemsetAsync(d_counts, 0, nrharq::kMaxTransmissions * sizeof(uint32_t), stream_));
  // what every stage holds, read back (the stream is idle afterwards)
  uint32_t held[nrharq::kMaxTransmissions] = {};
  auto read_held = [&]() -> int {
    SIM_TRY(hipMemcpyAsync(held, d_counts, sizeof(held), hipMemcpyDeviceToHost, stream_));
    SIM_TRY(hipStreamSynchronize(stream_));
    for (uint32_t s = 1; s < T; s++)
      if (held[s] > cap) {
        fail("HARQ stage pool overflow");
        return -3;
      }
    return 0;
  };
  // Stage t flushed.  It may pass on every row it holds, so the stage behind it is flushed first when that many might
  // not fit there, and so on down the stages: the deepest of them first, each into the room just made.
  auto drain = [&](uint32_t t) -> int {
    uint32_t deepest = t;
    while (deepest + 1 < T && size_t(held[deepest + 1]) + held[deepest] > cap) deepest++;
    for (uint32_t s = deepest;; s--) {
      if (held[s])
        if (int rc = flush_harq(s, held[s], ebn0_db, seed, max_iterations, chunk)) return rc;
      if (int rc = read_held()) return rc;
      if (s == t) return 0;
    }
  };
  // between chunks with pooling: stage 1 alone is filled by a chunk, and is flushed when another chunk's failures might
  // not fit; else, and at the end of the call: every stage in order
  auto flush_stages = [&](bool all) -> int {
    if (int rc = read_held()) return rc;
    if (!all) return held[1] + chunk > cap ? drain(1) : 0;
    for (uint32_t t = 1; t < T; t++)
      if (held[t])
        if (int rc = drain(t)) return rc;
    return 0;
  };
  for (size_t f0 = 0; f0 < frames; f0 += chunk) {
    const uint32_t nf = static_cast<uint32_t>(std::min(chunk, frames - f0));
    // stage 0: the first transmission is the frame of run() -- its generator, recovered with combine = 0
    launch_generator(ebn0_db, seed, first_frame + f0, nf);
    if (soft8) {
      launch_quantize(d_rx_.get<float>(), d_rx_i8_.get<int8_t>(), uint64_t(nf) * n_tx_);
      nr_rm_launch_recover_i8(rm_plan_, d_rx_i8_.get<int8_t>(), d_llrs_.get<int8_t>(), nf, soft::kSoftMax, false, stream_);
    } else {
      nr_rm_launch_recover<float>(rm_plan_, d_rx_.get<float>(), d_llrs_.get<float>(), nf, 0.0f, false, stream_);
    }
    if (int rc = dec_->decode_device(d_llrs_.get(), soft8 ? LlrType::I8 : LlrType::F32, nf, max_iterations, d_bits_.get<uint8_t>(), k_,
                                     d_its_.get<int32_t>(), nullptr, stream_)) {
      error_ = dec_->last_error();
      return rc;
    }
    if (T > 1 && soft8)
      gen::harq_collect_i8_kernel<<<(nf * 64 + 255) / 256, 256, 0, stream_>>>(
          d_its_.get<int32_t>(), nf, first_frame + f0, nullptr, nullptr, max_iterations, d_llrs_.get<uint32_t>(), static_cast<uint32_t>(n_ / 4),
          harq_stage_[1].soft.get<uint32_t>(), harq_stage_[1].frames.get<uint64_t>(), harq_stage_[1].spent.get<uint32_t>(), d_counts + 1,
          static_cast<uint32_t>(cap));
    else if (T > 1)
      gen::harq_collect_kernel<<<(nf * 64 + 255) / 256, 256, 0, stream_>>>(
          d_its_.get<int32_t>(), nf, first_frame + f0, nullptr, nullptr, max_iterations, d_llrs_.get<float>(), static_cast<uint32_t>(n_),
          harq_stage_[1].soft.get<float>(), harq_stage_[1].frames.get<uint64_t>(), harq_stage_[1].spent.get<uint32_t>(), d_counts + 1,
          static_cast<uint32_t>(cap));
    gen::harq_count_kernel<<<(nf * 64 + 255) / 256, 256, 0, stream_>>>(d_bits_.get<uint8_t>(), d_its_.get<int32_t>(), d_messages_.get<uint8_t>(),
                                                                       static_cast<uint32_t>(k_), pool_, seed, first_frame + f0, nullptr, nullptr,
                                                                       nf, max_iterations, T == 1 ? 1 : 0, d_counters, d_per_tx);
    if (T > 1 && f0 + chunk < frames)
      if (int rc = flush_stages(!pooling_)) return rc;
  }
  if (T > 1)
    if (int rc = flush_stages(true)) return rc;
  unsigned long long host[6], host_tx[nrharq::kMaxTransmissions * 4];
  SIM_TRY(hipMemcpyAsync(host, d_counters, sizeof(host), hipMemcpyDeviceToHost, stream_));
  SIM_TRY(hipMemcpyAsync(host_tx, d_per_tx, sizeof(host_tx), hipMemcpyDeviceToHost, stream_));
  SIM_TRY(hipStreamSynchronize(stream_));
  SIM_TRY(hipGetLastError());
  for (int i = 0; i < 6; i++) counters[i] = host[i];
  for (uint32_t i = 0; i < 4 * T; i++) per_tx[i] = host_tx[i];
  return 0;
}

int Simulator::generate_harq(double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames, uint32_t transmission, float *llrs,
                             uint32_t *pool_index) {
  if (const char *why = fading_error()) return fail(why), -1;
  auto refuse = [&](const char *why) {
    fail(why);
    return -4;
  };
  if (harq_.t == 0) return refuse("no HARQ sequence is set (ldpc_toolbox_sim_set_harq)");
  if (transmission >= harq_.t) return refuse("the HARQ sequence has no such transmission");
  if (const char *why = harq_modulation_error()) return refuse(why);
  for (uint32_t t = 0; t < harq_.t; t++)
    if (harq_.e[t] % static_cast<uint32_t>(modulation()) != 0) return refuse("every E must be a multiple of the modulation's bits per symbol");
  if (frames == 0) return 0;
  SIM_TRY(hipSetDevice(device_));
  const size_t bytes = frames * harq_.e[transmission] * sizeof(float);
  DeviceBuffer d_out;
  SIM_TRY(d_out.ensure(bytes));
  launch_harq_generator(ebn0_db, seed, transmission, first_frame, nullptr, static_cast<uint32_t>(frames), d_out.get<float>());
  SIM_TRY(hipMemcpyAsync(llrs, d_out.get(), bytes, hipMemcpyDeviceToHost, stream_));
  SIM_TRY(hipStreamSynchronize(stream_));
  SIM_TRY(hipGetLastError());
  if (pool_index)
    for (size_t f = 0; f < frames; f++) pool_index[f] = gen::pool_index(seed, first_frame + f, pool_);
  return 0;
}

}  // namespace ldpc
