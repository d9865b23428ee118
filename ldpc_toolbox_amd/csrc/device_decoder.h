// Batched belief-propagation decoder on one MI355X (gfx950) -- host-side handle.
//
// This is the device replacement for the reference's per-codeword decoder objects
// (flooding::Decoder<A>, /root/reference/src/decoder/flooding.rs:13-125, and
// horizontal_layered::Decoder<A>, /root/reference/src/decoder/horizontal_layered.rs:17-110)
// generic over the float DecoderArithmetic rules (arithmetic.rs:140-580, 899-1072).
// One handle = one Tanner graph + one rule + one schedule on one device, decoding
// batches of codewords with per-codeword semantics identical to the scalar decode:
// pre-check on the raw input (iterations 0), freeze at the first zero syndrome,
// failure after max_iterations.
//
// HBM layout: every per-codeword array is [row][G] with the
// codeword index fastest, G = codewords per group; a wavefront therefore reads a
// contiguous 256 B..1 KiB row segment for every graph edge it touches.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "hip_owned.h"
#include "implementation.h"
#include "sparse.h"

namespace ldpc {

struct GroupCall;

// Element type of a decode call's LLR rows.  The posterior it asks for is in the same precision, except that 8-bit soft bits
// (include/ldpc_toolbox.h, PART 9; the 8-bit implementations only) get the decoder's int16_t posterior word.
enum class LlrType : uint8_t { F32, F64, I8 };
constexpr size_t llr_bytes(LlrType t) { return t == LlrType::F64 ? 8 : (t == LlrType::F32 ? 4 : 1); }
constexpr size_t posterior_bytes(LlrType t) { return t == LlrType::F64 ? 8 : (t == LlrType::F32 ? 4 : 2); }

struct KernelStat {
  uint64_t launches = 0;
  double total_ms = 0.0;
};

// which launches are bracketed with hipEvents when profiling is on
enum KernelKind { kKernelCheck = 0, kKernelVar = 1, kKernelLayer = 2, kKernelOther = 3, kKernelKinds = 4 };

class DeviceDecoder {
 public:
  // puncturing: empty = none, else the reference's block pattern (puncturing.rs:27-40).
  static DeviceDecoder *create(const SparseMatrix &h, const Implementation &impl,
                               const std::vector<uint8_t> &puncturing, int device, std::string *err);
  ~DeviceDecoder();

  size_t n() const { return n_; }
  size_t m() const { return m_; }
  size_t edges() const { return e_; }
  // length of the LLR vector a caller must supply (punctured length if puncturing is set)
  size_t input_len() const { return input_len_; }
  const Implementation &implementation() const { return impl_; }
  int device() const { return device_; }
  uint32_t max_check_degree() const { return max_row_weight_; }
  uint32_t max_variable_degree() const { return max_col_weight_; }
  size_t layers() const { return level_ptr_.empty() ? 0 : level_ptr_.size() - 1; }
  // how the last decode_device / decode_host call was laid out: execution lanes used, codewords per group
  uint32_t last_lanes() const { return last_lanes_; }
  uint64_t last_pooled() const { return last_pooled_; }   // frames of the last call that went through the straggler pool
  size_t last_group() const { return last_group_; }
  // words per check-row record when the flooding min-sum path keeps row records (kernels.hip.h,
  // cn_minsum_rec_kernel), 0 when it keeps per-edge messages
  uint32_t row_records() const { return (rec_ready_ && records_wanted() && opt_lfree_ && !opt_staged_minsum_) ? rec_w_ : 0; }
  uint32_t record_flag_bits() const { return row_records() ? rec_flag_bits_ : 0; }
  // whether the last decode call's variable-node launches read the row records ("vn_records")
  uint32_t last_vn_records() const { return last_vn_records_.load(std::memory_order_relaxed) ? 1 : 0; }
  // "flags8" as set, and the bytes of a record's flags word in the last decode call: 1 (the byte form), 2, 4 or 8; 0: the call
  // kept no flooding row records
  uint32_t flags8() const { return opt_flags8_ ? 1 : 0; }
  uint32_t last_record_flag_bytes() const { return last_record_flag_bytes_.load(std::memory_order_relaxed); }
  // whether the last decode call's variable-node launches walked the kept list in bundles ("vn_bundles"), and the record
  // fetches the bundles spare when every coincident request of a workgroup is served once, in thousandths of the list's
  // fetches, at that call's bundle width (graph_tables.h, count_vn_bundle_fetches); 0 when off
  uint32_t last_vn_bundles() const { return last_vn_bundles_.load(std::memory_order_relaxed) ? 1 : 0; }
  uint32_t vn_bundle_saved_permille() const { return last_vn_bundle_saved_.load(std::memory_order_relaxed); }
  // whether they walked it in chains ("vn_chains": the bundled walk with a record carried from entry to entry), and the
  // loads of records the chains spare, carried ones and coincident ones, in thousandths of the list's fetches
  // (graph_tables.h, count_vn_chain_fetches); 0 when off
  uint32_t last_vn_chains() const { return last_vn_chains_.load(std::memory_order_relaxed) ? 1 : 0; }
  uint32_t vn_chain_saved_permille() const { return last_vn_chain_saved_.load(std::memory_order_relaxed); }
  // "cn_row_shape" as set; whether the last decode call's check-node launches behind the first iteration took the row-shape
  // form; and the runs of the walk that conformed at that call's run length, and the rows in them (graph_tables.h,
  // count_row_shape_runs); 0 when the form did not run
  uint32_t cn_row_shape() const { return opt_cn_row_shape_ ? 1 : 0; }
  uint32_t last_cn_row_shape() const { return last_cn_row_shape_.load(std::memory_order_relaxed) ? 1 : 0; }
  uint32_t cn_row_shape_runs() const { return last_cn_row_shape() ? last_cn_shape_runs_.load(std::memory_order_relaxed) : 0; }
  uint32_t cn_row_shape_rows() const { return last_cn_row_shape() ? last_cn_shape_rows_.load(std::memory_order_relaxed) : 0; }
  // "call_edges" as set, and which of its shortcuts the groups of the last decode call took (kCallEdge* below, OR-ed)
  uint32_t call_edges() const { return opt_call_edges_ ? 1 : 0; }
  uint32_t last_call_edges() const { return last_call_edges_.load(std::memory_order_relaxed); }
  static constexpr uint32_t kCallEdgeIngest = 1;      // the ingest launch stored no copy of the input in the posterior array
  static constexpr uint32_t kCallEdgeClose = 2;       // the last pack covered the kept rows only; the closing launch packed the L-free ones
  static constexpr uint32_t kCallEdgeEmit = 4;        // the final emit launch was given the packed decisions
  static constexpr uint32_t kCallEdgeCheckpoint = 8;  // a checkpoint ran as two launches behind its plan (set when one was enqueued)

  // codewords per group (rounded up to the wave tile).  0 = automatic.
  void set_group_size(size_t g) { group_pref_ = g; }
  size_t group_size() const { return group_pref_; }
  // a call of fewer codewords still runs in groups of at least this many (0 = off): a caller that alternates between
  // large and small calls keeps one workspace instead of re-allocating it every time (the simulator's straggler pool)
  void set_min_group(size_t g) { min_group_ = g; }
  // codewords per group a call of `batch` codewords is cut into (the set value, else a default that grows for small graphs)
  size_t preferred_group(size_t batch) const { return pick_group(batch); }
  // The 33 options of set_option (26 in round 6; there were 54: the tuning knobs whose alternatives had all been measured within a
  // percent are constants now, see kStreamBlock ... below).  Results never depend on any of them; each selects between
  // forms that tests/ compare bit for bit.  returns false for an unknown key.
  //   which kernels run   "lfree" (0: plain flooding min-sum kernels), "records" (0 / 1 / 2: per-edge messages / row records
  //                       where the graph suits them / wherever possible), "rec_quiet" (0: L-free posteriors stored every
  //                       iteration), "vn_event" (0: the first convergences' rebuild as a launch of its own), "vn_records" (0 / 1:
  //                       the variable nodes summed from per-edge messages / from the row records, 16-bit flags only), "vn_bundles" (0 / 1: that
  //                       form's kept list in variable order / in bundles of the variables a workgroup sums together), "vn_chains" (0 / 1: the
  //                       bundled list walked entry by entry / in chains whose shared record stays in registers; "vn_chain_len":
  //                       4, 8 or 16 entries per chain), "flags8" (0 / 1: the
  //                       16-bit flags of rows of at most 7 edges stored as half-words / as bytes), "cn_row_shape" (0 / 1: with
  //                       "vn_records" and "flags8" in f32, the generic row step in every run of the check-node walk / a
  //                       straight-line one in the runs whose rows all have the graph's dominant shape), "rec_long"
  //                       (1: the record kernel's long-row variant whatever the graph), "call_edges" (0: the launches around a
  //                       call's iterations as they were: opt_call_edges_ below), "staged_minsum" (1: Minsum through
  //                       the generic LDS-staged kernel), "cn_reg" / "hl_reg" / "hl_records" (0: the LDS-staged / two-pass /
  //                       per-edge forms instead of register-resident rows and layered row records), "serial_levels"
  //                       (layered: more dependency levels than this -> row-serial mode), "latency" / "latency_edge"
  //                       (largest batch the single-launch small-batch paths take; 0 = never)
  //   launch geometry     "waves" (target wavefronts per launch), "vec" (codewords per lane: 1, 2, 4), "tile" (codewords per
  //                       layout tile), "rec_run" (consecutive rows per wavefront step of the record kernel)
  //   early termination   "compact" (0: no batch compaction), "compact_first", "compact_every" (checkpoint schedule)
  //   host side           "lanes" (1 or 2 execution lanes; 0 = automatic), "lane_threads", "lane_pace", "lead", "poll" (0: the
  //                       host ignores the progress word), "throttle" (a call on the caller's stream may pace itself),
  //                       "pooling" (straggler pooling inside the batch entries: below)
  // plus "group_size" and "profiling" at the C ABI.  LDPC_TOOLBOX_{GROUP, WAVES, VEC, STAGED_MINSUM} set four of them at
  // construction.
  bool set_option(const std::string &key, int64_t value);
  void set_profiling(bool on);
  KernelStat kernel_stat(int kind);
  void reset_kernel_stats();

  // Device-resident batch decode.  All pointers are device pointers on device();
  // llrs: [batch][input_len()] f32, f64 or int8_t soft bits (llrs_type), one row per codeword;
  // bits: [batch][out_len] u8, first out_len hard decisions of every codeword;
  // iterations: [batch] i32, -1 = failed (may be null);
  // posterior: [batch][n] in the precision of `llrs`, int16_t for 8-bit soft bits (may be null).
  // stream: launch stream (nullptr = the handle's own stream, ordered after everything queued on the
  // legacy default stream at the time of the call, and synchronised on return).
  // returns 0, or a negative error code (message via last_error()).
  int decode_device(const void *llrs, LlrType llrs_type, size_t batch, uint32_t max_iterations,
                    uint8_t *bits, size_t out_len, int32_t *iterations, void *posterior,
                    hipStream_t stream);

  // Same contract with host pointers: staged through device buffers group by group.
  int decode_host(const void *llrs, LlrType llrs_type, size_t batch, uint32_t max_iterations,
                  uint8_t *bits, size_t out_len, int32_t *iterations, void *posterior);

  // Syndrome of hard decisions (the reference's check_llrs, decoder.rs:157-164, with the parities
  // returned): bits [batch][n] one byte per bit; syndrome [batch][m] (1 = unsatisfied; may be
  // null); weight [batch] (may be null).  Device pointers / host pointers.
  int syndrome_device(const uint8_t *bits, size_t batch, uint8_t *syndrome, uint32_t *weight, hipStream_t stream);
  int syndrome_host(const uint8_t *bits, size_t batch, uint8_t *syndrome, uint32_t *weight);

  const std::string &last_error() const { return error_; }

 private:
  DeviceDecoder() = default;
  struct Workspace;
  struct GroupFrame;
  // one group of codewords (device_decoder_internal.h, GroupCall): run_any resolves the host's pacing and hands the group
  // to the 8-bit rules or to the float rules in the decoder's precision
  int run_group_i8(Workspace &w, const GroupCall &call);
  template <typename T>
  int run_group(Workspace &w, const GroupCall &call);
  int run_any(Workspace &w, const GroupCall &call);
  int ensure_workspace(Workspace &w, size_t group, void *place = nullptr, size_t *need = nullptr);
  int ensure_lanes(uint32_t lanes, size_t group);
  void release_joint();
  int ensure_host_staging(Workspace &w, size_t G, size_t in_elem);
  int ensure_row_scratch(Workspace &w, size_t bytes);
  // host-pointer entry: pinned staging rings, copy streams, batch-wide device output buffers
  struct HostPipe;
  int ensure_pipe(size_t group, size_t out_len, size_t post_elem, bool posterior);
  int stage_in(const char *src, char *dst, size_t bytes);
  int drain_out(char *dst, const char *src, size_t bytes);
  // recorded by run_group right after the ingest launch (the group's input buffer is free again)
  // small-batch (latency) path: lanes across the rows / variables of one codeword, one persistent launch
  // per call (latency.hip.h).  Flooding Minsumf32 only; the other implementations take the batch kernels.
  struct LatencyPath;
  struct SmallBatchCall;  // what both small-batch paths stage alike (latency_paths.hip)
  // the lane-per-edge small-batch path (latency_edge.hip.h): the layered schedule and, for every rule but Minsumf32,
  // the flooding schedule; f32 and f64 arithmetic
  struct EdgeLatencyPath;
  // largest batch that takes it: up to 8 codewords decode one per XCD, larger calls in bundles of up to 8 per XCD that
  // share every phase and barrier; measured against the batched kernels (tools/scalar_probe_layered.py,
  // profiles/r03_latency.txt); the A-Min* rule's serial fold is repeated by every lane of a row: a lower limit
  size_t edge_latency_limit() const;
  uint32_t opt_latency_edge_ = 256;  // "latency_edge": cap on that limit
  size_t edge_lanes_ = 0;           // lane slots of the edge path's message array
  int decode_latency_edge(const void *llrs, LlrType llrs_type, bool host_pointers, size_t batch, uint32_t max_iterations,
                             uint8_t *bits, size_t out_len, int32_t *iterations, void *posterior, hipStream_t stream);
  // "latency": largest batch that takes this path (0 = never).  8 codewords decode at once (one per XCD), more
  // take turns; measured against the batched kernels (tools/scalar_probe.py): ahead up to 32 (DVB-S2 1/2 at 2 dB:
  // 16 frames 0.57 vs 2.05 ms, 32 frames 1.11 vs 2.37 ms), level at 64
  uint32_t opt_latency_ = 32;
  static constexpr int kLatencyRetry = -100;  // decode_latency: redo the call with the batched kernels
  static constexpr uint32_t opt_serial_levels_default() { return 512; }
  int decode_latency(const void *llrs, LlrType llrs_type, bool host_pointers, size_t batch, uint32_t max_iterations,
                     uint8_t *bits, size_t out_len, int32_t *iterations, void *posterior, hipStream_t stream);
  uint32_t lane_count() const;
  bool split_pays(size_t batch) const;
  size_t pick_group(size_t batch) const;
  bool fail(const std::string &msg, hipError_t e = hipSuccess);
  void timed_begin(int kind, hipStream_t s);
  void timed_end(int kind, hipStream_t s);
  void drain_events();

  Implementation impl_;
  int device_ = 0;
  size_t n_ = 0, m_ = 0, e_ = 0, input_len_ = 0;
  uint32_t max_row_weight_ = 0, max_col_weight_ = 0;
  size_t group_pref_ = 0, min_group_ = 0;
  uint32_t opt_tile_ = 0;
  uint32_t opt_waves_ = 0, opt_vec_ = 4;
  bool opt_staged_minsum_ = false;
  // Launch constants that were run-time options up to round 5.  Every one of them had been measured within a percent of its
  // alternatives ("What did not pay"; profiles/r0N_*), each alternative was a set of template variants or
  // a branch nobody took: fixed in round 6 (54 keys in set_option -> 30 with the new "pooling", 641 kernels -> 450 with its three).
  static constexpr uint32_t kStreamBlock = 256;      // threads per workgroup of the streaming kernels (64 / 128: within 1 %)
  static constexpr uint32_t kVnWaves = 128 * 1024;   // wavefronts of a variable-node launch
  static constexpr uint32_t kPackWaves = 16 * 1024;  // ... of the hard-decision packing launch (256 K: -0.7 % on config 3)
  static constexpr uint32_t kSyndThreads = 512 * 1024, kMoveWaves = 64 * 1024, kRetireBlocks = 256;
  // workgroups of a "call_edges" checkpoint launch's two roles: they walk the blocks / waves of the launches they stand for
  static constexpr uint32_t kEdgeRetireBlocks = 1024, kEdgeMoveBlocks = 2048;
  // decision rule of the compaction checkpoints (kernels_group.hip.h, CompactRule): waiting until half of the slots are
  // free beats re-packing at a quarter, the cost constants hardly matter (round 2's sweep over Eb/N0)
  static constexpr uint32_t kCompactHorizon = 8, kCompactCostLive = 9, kCompactCostSlots = 0, kCompactMinFreedQ = 2;
  std::string error_;

  // L-free variables (degree <= 2) of the flooding min-sum path (graph_tables.h, LfreeTables)
  uint32_t n_keep_ = 0, n_free_ = 0;
  uint32_t post_rows_keep_ = 0;  // 1 + index of the last variable of degree != 1, 2 (a compaction moves only those posterior rows)
  // row records of the flooding min-sum path (graph_tables.h, RowRecordTables)
  bool opt_rec_long_ = false;  // "rec_long": take the record kernel's long-row variant whatever the graph (A/B)
  bool opt_rec_quiet_ = true;  // "rec_quiet": L-free posteriors are stored only once a slice has a converged codeword
  bool opt_vn_event_ = true;  // "vn_event": the first convergences' L-free posteriors rebuilt inside the variable-node launch (0: a launch of their own)
  // "vn_records": the variable-node launch reads this iteration's row records instead of per-edge messages, which the
  // check-node launch then does not store (run_group.hip.h; 16-bit flags only)
  // (default: on for plain Minsumf32 on DVB-S2 normal frames at rate 1/2, the one configuration measured to pay by the
  // project's bar, profiles/vn_records.txt; off for every other code, rule and precision)
  bool opt_vn_records_ = false;
  // "flags8": where record_flag_bytes (graph_tables.h) says 1 -- 16-bit flags, rows of at most 7 edges -- the flags are stored
  // as bytes and two argmin bits in the magnitudes' sign bits (record_flags8.h), in the first half of the same arrays: the
  // key may change between calls.  (default: on where "vn_records" is -- plain Minsumf32 on DVB-S2 normal frames at rate 1/2,
  // the one configuration timed: +2.9 .. +3.5 % codewords/s, profiles/record_flags8.txt; off for every other code, rule
  // and precision, where the key selects it)
  bool opt_flags8_ = false;
  // "vn_bundles": the record form of the variable-node launch walks the kept list in the order of build_vn_bundles
  // (graph_tables.h): the list entries the waves of a workgroup sum in the same step share rows, so a row's record crosses
  // the path from the Infinity Cache once for them.  The tables are built for kVnBundleW entries per bundle -- a workgroup's
  // waves when a slice is a whole tile -- and a launch with more slices per tile finds its narrower bundles inside them.
  // Another order of independent sums: results do not depend on it.  (default: on where "vn_records" is -- plain Minsumf32 on
  // DVB-S2 normal frames at rate 1/2, the one configuration timed: +5.0 % codewords/s, profiles/vn_bundles.txt; off for every
  // other code, rule and precision, where the key selects it)
  bool opt_vn_bundles_ = false;
  static constexpr uint32_t kVnBundleW = kStreamBlock / 64;
  uint32_t vn_bundle_saved_[kVnBundleW + 1] = {};  // [w]: thousandths of the record fetches spared at bundle width w
  std::atomic<bool> last_vn_bundles_{false};
  std::atomic<uint32_t> last_vn_bundle_saved_{0};
  // "vn_chains": with "vn_bundles", the launch walks the kept list in the order of build_vn_chains (graph_tables.h): a wave
  // sums kVnChainLens[...] = "vn_chain_len" entries one after the other, and where two of them share a row the second takes
  // the row's record from the wave's registers.  Another order of independent sums: results do not depend on it.
  // (default: on where "vn_bundles" is -- plain Minsumf32 on DVB-S2 normal frames at rate 1/2, the one configuration timed,
  // with chains of 8: profiles/vn_chains.txt; off for every other code, rule and precision, where the key selects it)
  // (The tables of all three lengths are built and uploaded at create, for every graph that gets bundled tables: the keys may
  // change between calls and a call allocates nothing -- the chained lists lie behind the bundled ones in d_keep_rs_.  On
  // DVB-S2 1/2, the largest built-in graph: 27 ms of create and 0.9 MB per length.)
  bool opt_vn_chains_ = false;
  uint32_t opt_vn_chain_len_ = 8;
  static constexpr uint32_t kVnChainLens[3] = {4, 8, 16};
  struct VnChainAt {
    uint32_t rs_at = 0, var_at = 0, ptr_at = 0, n_blocks = 0;  // word offsets in d_keep_rs_ (rs_at 0: no such tables)
    uint32_t saved = 0, saved_alone = 0;  // thousandths of the fetches spared: with kVnBundleW step-mates; by the carries alone
  } vn_chain_at_[3];
  std::atomic<bool> last_vn_chains_{false};
  std::atomic<uint32_t> last_vn_chain_saved_{0};
  // "cn_row_shape": with "vn_records" and "flags8" in f32, the check-node launches behind the first iteration take the record
  // kernel's row-shape form (kernels_flooding.hip.h, SHAPE): runs of the walk whose rows all have the graph's dominant shape
  // (graph_tables.h, build_row_shapes) run a straight-line row step, every other run the generic one, in the same launch.  The
  // same operations in the same order: results do not depend on it.  A call whose run length ("rec_run") leaves no
  // conforming run launches the generic form.  (default: on where "flags8" is -- plain Minsumf32 on DVB-S2 normal frames at
  // rate 1/2, the one configuration timed: +2.1 % codewords/s, profiles/cn_row_shape.txt; off for every other code, rule and
  // precision, where the key selects it: f32 only)
  bool opt_cn_row_shape_ = false;
  std::vector<uint32_t> row_shape_span_;  // RowShapeTables::span, as uploaded behind the peer words (empty: no such tables)
  uint32_t row_shape_kind_ = 0;           // RowShapeTables::kind: the order of the two parity slots the counts are about
  std::atomic<bool> last_cn_row_shape_{false};
  std::atomic<uint32_t> last_cn_shape_runs_{0}, last_cn_shape_rows_{0};
  // "call_edges": what a call does around its iterations, trimmed to what its result needs (profiles/call_edges.txt).  On the
  // flooding record path of a call that asks for no posterior: the ingest launch stores the input once, not twice (the first
  // check-node launch reads `chan` in the posterior's place); the last pack covers the rows the variable-node launch writes and
  // the closing launch packs the L-free variables' decisions without storing their posteriors (vn_free_hard_kernel); the
  // final emit launch reads those packed words, not posterior rows.  And wherever a compaction checkpoint is due, it is two
  // launches behind its plan, not four (kernels_group.hip.h, compact_retire_move_kernel).  0: every launch as before.
  // Results do not depend on it.
  bool opt_call_edges_ = true;
  std::atomic<uint32_t> last_call_edges_{0};  // (OR-ed by every group's run_group, cleared by the decode entries)
  std::atomic<uint32_t> last_record_flag_bytes_{0};
  std::atomic<bool> last_vn_records_{false};  // (written by every group's run_group: with "lane_threads" from two host threads)
  uint32_t rec_w_ = 0;
  uint32_t rec_flag_bits_ = 0;  // 16: the records' flags are half-words in an array of their own (graph_tables.h)
  bool rec_ready_ = false, rec_prefers_ = false;
  // "records": 0 = never, 1 = where the graph suits them (rec_prefers_: the default), 2 = wherever they are possible
  uint32_t opt_records_ = 1;
  bool records_wanted() const { return opt_records_ >= 2 || (opt_records_ == 1 && rec_prefers_); }
  uint32_t opt_rec_run_ = 8;
  bool opt_compact_ = true;
  // schedule of the compaction checkpoints ("compact_first", "compact_every": 0 = 6 and 2 for flooding, 3 and 1 for the
  // layered schedule)
  uint32_t opt_compact_first_ = 0, opt_compact_every_ = 0;
  uint32_t opt_serial_levels_ = 512;  // layered: more dependency levels than this -> row-serial mode
  uint32_t opt_cn_reg_ = 1;  // flooding LDS-staged rules: register-resident rows with row records (0 = cn_staged_kernel)
  uint32_t opt_hl_reg_ = 1;  // layered min-sum: register-resident rows (0 = two-pass form)
  // "lane_threads": the layered schedule's two execution lanes are enqueued by two host threads;
  // "throttle": a call on the CALLER's stream may also wait on the group's progress word between iterations (it then
  // returns when the group is within two iterations of its end instead of at once; the simulator sets it)
  bool opt_lane_threads_ = true, opt_throttle_ = false;
  uint32_t opt_lead_ = 0;  // iterations a paced host may run ahead of its group (0: 1 for a lane's own thread, else 2 layered, 8 flooding)
  bool opt_lane_pace_ = true;  // a lane's own enqueuing thread paces itself on the group's progress word
  bool opt_hl_records_ = true;  // "hl_records": layered min-sum keeps a row's messages as one record (0 = per-edge R)
  std::vector<uint32_t> level_maxdeg_;
  std::vector<uint32_t> level_rec_ptr_;  // [n_levels] first word of a level's records in d_level_recs_
  bool lfree_ready_ = false, opt_lfree_ = true;
  std::vector<uint32_t> level_ptr_;
  uint32_t pattern_len_ = 0;  // blocks of the puncturing pattern (0: none)

  size_t joint_stride_ = 0, joint_second_ = 0;  // nominal distance of the lanes; the one the placement probe chose
  int order_after_default_stream(hipStream_t s);
  uint32_t last_lanes_ = 0;
  size_t last_group_ = 0;
  // "pooling" (0 / 1, default 0): STRAGGLER POOLING inside the batch entries (the simulation driver has had it since round 3,
  // csrc/simulator.h).  A call of several chunks learns from its first chunk how many iterations its frames take; later chunks
  // run a reduced budget (2 x average + 8), the frames that have not converged by then are decoded again, together, with the
  // full budget, and their results replace the first pass's.  Per frame the outcome is that of ONE full-budget decode (the
  // decoder starts from the channel LLRs and is deterministic), so outputs do not depend on the option; what it spares is
  // every chunk's nearly empty iterations up to max_iterations behind its few slow or failing frames (the waterfall with
  // the reference's default of 100 iterations, src/cli/ber.rs:64-66).  The host reads each chunk's iteration counts before
  // it starts the next: the call synchronises between chunks (device entry: the library's own stream, or "throttle").
  bool opt_pooling_ = false;
  uint64_t last_pooled_ = 0;
  uint32_t pool_budget_ = 0, pool_budget_max_it_ = 0;  // the budget the last pooled call ended with carries over to the next one at the same limit
  struct StragglerPool;
  int ensure_pool(size_t batch, size_t rows, size_t out_len, size_t in_elem, size_t post_elem, bool posterior, bool own_iterations);
  static uint32_t next_pool_budget(double ok, double sum_its_ok, double stragglers, double straggler_its, double failed_full,
                                   uint32_t max_it);
  int decode_device_plain(const void *llrs, LlrType llrs_type, size_t batch, uint32_t max_iterations, uint8_t *bits, size_t out_len,
                          int32_t *iterations, void *posterior, hipStream_t stream);
  int decode_device_pooled(const void *llrs, LlrType llrs_type, size_t batch, uint32_t max_iterations, uint8_t *bits, size_t out_len,
                           int32_t *iterations, void *posterior, hipStream_t stream);
  int decode_host_plain(const void *llrs, LlrType llrs_type, size_t batch, uint32_t max_iterations, uint8_t *bits, size_t out_len,
                        int32_t *iterations, void *posterior);
  int decode_host_pooled(const void *llrs, LlrType llrs_type, size_t batch, uint32_t max_iterations, uint8_t *bits, size_t out_len,
                         int32_t *iterations, void *posterior);
  size_t pool_chunk(size_t batch) const;
  uint32_t opt_lanes_ = 0;  // 0 = automatic (2 for the layered schedule, 1 for flooding)
  bool opt_poll_ = true;    // host follows the device's progress word and stops enqueuing a finished group

  bool profiling_ = false;
  struct PendingEvent {
    int kind;
    Event a, b;
  };
  KernelStat stats_[kKernelKinds];

  // What the handle owns (hip_owned.h).  Members are destroyed last to first: the streams go after every buffer and
  // event, and ~DeviceDecoder has made them idle before anything goes.
  Stream stream_, stream2_;
  Event ev_fork_, ev_join_, ev_default_;
  // graph tables in HBM
  DeviceBuffer d_row_ptr_, d_edge_col_, d_col_ptr_, d_col_edge_;
  // layered schedule: rows grouped into dependency levels (hard part 5)
  DeviceBuffer d_level_rows_;
  DeviceBuffer d_level_recs_;   // row records of the register-resident level kernels (slice_tasks.h, build_level_recs)
  DeviceBuffer d_row_recs_;     // flooding: every row's record in row order (cn_reg_kernel)
  DeviceBuffer d_serial_recs_;  // the same for the row-serial launch: all rows as one level, one record size
  DeviceBuffer d_src_block_;    // depuncture map: source block of every pattern block, -1 = punctured
  DeviceBuffer d_edge_aux_, d_keep_var_, d_keep_ptr_, d_keep_edge_, d_free_var_, d_free_ptr_, d_free_edge_;  // LfreeTables
  DeviceBuffer d_edge_peer_, d_free_rs_, d_keep_pos_;                                                         // RowRecordTables
  // KeepRsTable, and behind it in the same allocation the VnBundleTables: keep_rs, list_var, list_ptr at these word offsets
  // (and behind those the VnChainTables of every chain length: vn_chain_at_)
  DeviceBuffer d_keep_rs_;
  uint32_t bundle_rs_at_ = 0, bundle_var_at_ = 0, bundle_ptr_at_ = 0;  // (bundle_rs_at_ 0: no bundled tables)
  // Two execution lanes (workspace + stream): groups alternate between them, so the idle gaps
  // between one lane's short launches (layered schedule: one per dependency level) are filled by
  // the other's, and the host entry's PCIe copies overlap the other lane's decode.
  DeviceBuffer joint_slab_;  // both lanes' workspaces (ensure_lanes); a workspace inside it is a view, not an owner
  std::unique_ptr<Workspace> ws_[2];
  std::unique_ptr<StragglerPool> pool_;
  std::unique_ptr<EdgeLatencyPath> lat_edge_;
  std::unique_ptr<LatencyPath> lat_;
  std::unique_ptr<HostPipe> pipe_;
  std::vector<Event> event_pool_;
  std::vector<PendingEvent> pending_;
};

}  // namespace ldpc
