// Internal to the library's translation units (device_decoder.hip, run_group_f32.hip, run_group_f64.hip,
// run_group_i8.hip, latency_paths.hip): the per-handle state behind DeviceDecoder's opaque members, launch geometry,
// the per-call knobs and the host's view of a group's progress word.  Round 6 cut the one 3 200-line translation unit
// (6 minutes of compile time) by what instantiates kernels: the f32 and f64 float rules, the 8-bit rules and the small-batch
// kernels each compile on their own, in parallel; every kernel is still instantiated in exactly one of them.
#pragma once
#include "device_decoder.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <type_traits>

#include "graph_tables.h"
#include "hip_owned.h"
#include "kernels.hip.h"
#include "slice_tasks.h"
#include "latency.hip.h"
#include "latency_edge.hip.h"

namespace ldpc {

inline uint32_t env_u32(const char *name, uint32_t dflt) {
  const char *s = std::getenv(name);
  if (!s || !*s) return dflt;
  return static_cast<uint32_t>(std::strtoul(s, nullptr, 10));
}

inline size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

struct DeviceDecoder::Workspace {
  size_t G = 0;  // codewords per group this workspace is sized for
  size_t elem = 4;
  void *slab = nullptr;  // one allocation; the arrays below are carved from it
  DeviceBuffer own_slab;  // ... this one, unless
  bool borrowed = false;  // the slab is a part of the decoder's joint allocation for both lanes (ensure_lanes): a view
  size_t slab_bytes = 0;
  void *chan = nullptr, *post = nullptr, *msg = nullptr, *msg2 = nullptr;
  void *rec[2] = {nullptr, nullptr};  // row records, double-buffered (instead of msg2)
  uint16_t *rec_flags[2] = {nullptr, nullptr};  // their 16-bit flags (rec then holds the magnitudes alone), or null
  bool records = false;
  uint64_t *rawbits = nullptr, *hardbits = nullptr;
  // compaction: perm = the movers' slots, slot_tmp = the holes they fill, fill_cw = codeword landing in a slot
  uint32_t *perm = nullptr, *slot_cw = nullptr, *slot_tmp = nullptr, *fill_cw = nullptr, *n_slots = nullptr;
  dev::CompactPlan *plan = nullptr;
  uint32_t *hard_ok = nullptr;  // "call_edges": whether the last pack of the group wrote hardbits (pack_hard_kernel, `ran`)
  uint32_t *done = nullptr, *unsat0 = nullptr, *unsat1 = nullptr, *n_active = nullptr, *scratch_flags = nullptr,
           *slice_state = nullptr;
  int32_t *iters = nullptr;
  // progress word (pinned host memory, mapped into the device): kernels.hip.h, State::publish
  PinnedBuffer flag;
  uint64_t *h_flag = nullptr, *d_flag = nullptr;
  uint32_t epoch = 0;
  // device-side input staging of decode_host (one group's rows as the caller laid them out)
  DeviceBuffer in;
  // decode_host: recorded right after the ingest kernel of the group being enqueued (the lane's input buffer is free
  // again), and counted, so that the staging thread knows the record has been made
  hipEvent_t after_ingest = nullptr;
  std::atomic<uint32_t> *ingest_seq = nullptr;
  // check rows too long for the LDS-staged kernels' columns (more than 160 KB per 64 threads): per-wavefront columns in
  // HBM, allocated at the first call that needs them (kernels.hip.h, cn_staged_kernel SCRATCH)
  DeviceBuffer row_scratch;
};

// pinned staging of the host-pointer entry (decode_host, further down)
struct DeviceDecoder::HostPipe {
  static constexpr size_t kChunk = size_t(32) << 20;
  static constexpr size_t kGranule = size_t(64) << 10;
  static constexpr int kSlots = 4;
  static constexpr int kOutRing = 4;  // group-sized device output buffers (two per execution lane)
  Stream h2d, d2h;
  // pinned chunks (<= kChunk), allocated at first use and only as large as the calls need (a reference-style scalar call
  // pins a few hundred KB, not 8 x 32 MiB)
  PinnedBuffer in_slot[kSlots], out_slot[kSlots];
  Event in_done[kSlots], out_done[kSlots];
  int next_in = 0;
  Event in_ready[2], ingested[2];
  std::vector<Event> group_done;
  DeviceBuffer d_bits[kOutRing], d_iters[kOutRing], d_post[kOutRing];
  unsigned copy_threads = 1;
};

// What the two single-launch small-batch paths stage alike (latency_paths.hip, stage_small_batch): pinned memory the
// kernel reads and writes itself, sized by the largest call so far -- the caller's input; [error word | bits |
// iterations | posterior] -- and the size of the persistent launch.
struct SmallBatchStaging {
  PinnedBuffer h_in, h_out;
  uint32_t grid = 0;  // workgroups of the persistent launch (0 = not yet sized from the device's occupancy)
};

// small-batch path (latency.hip.h): graph tables in the order that path wants, per-XCD codeword state
struct DeviceDecoder::LatencyPath {
  SlicedTables tables;  // built in create(), uploaded at first use
  bool uploaded = false;
  DeviceBuffer d_rslice_ptr, d_rdeg, d_col, d_vslice_ptr, d_vdeg, d_vedge, d_perm, d_inv;
  DeviceBuffer slot_mem, sync;
  dev::LatencyState slots{};  // 8 slots of {chan, post, msg, rawhard} in slot_mem
  SmallBatchStaging staging;
  static constexpr size_t kPinnedGranule = size_t(1) << 20;
};

// small-batch path with the lanes across a codeword's edges (latency_edge.hip.h): the rows packed into wavefront
// chunks, level after level (layered) or all at once (flooding, plus the variables' edge lists)
struct DeviceDecoder::EdgeLatencyPath {
  EdgeLaneTables tables;
  bool uploaded = false;
  DeviceBuffer d_level_chunk, d_lane_var, d_lane_info, d_var_ptr, d_var_lane;
  DeviceBuffer slot_mem, flag_mem, sync;
  dev::EdgeLatState slots{};  // base in slot_mem, flags in flag_mem
  SmallBatchStaging staging;
  static constexpr size_t kPinnedGranule = size_t(1) << 16;
};

#define HIP_TRY(expr)                                  \
  do {                                                 \
    hipError_t _e = (expr);                            \
    if (_e != hipSuccess) {                            \
      fail(#expr, _e);                                 \
      return -2;                                       \
    }                                                  \
  } while (0)

// the batch entries' straggler pool (device_decoder.h, "pooling"): device buffers of decode_device_pooled
struct DeviceDecoder::StragglerPool {
  // stats: [converged, failed at the full budget, stragglers] + u64 iterations of the converged
  DeviceBuffer d_idx, d_stats, d_llrs, d_post, d_bits, d_its, d_its_all;
};

// ---- launch helpers ----------------------------------------------------------------------

struct Tiling {
  uint32_t blocks, threads;
  dev::Sched sched;
};

// Waves are tile-major: wave w works on codeword slice w / wpc and starts at node w % wpc
// (stride wpc).  wpc is rounded so that a slice's waves fill whole workgroups.
inline Tiling make_tiling(uint32_t G, uint32_t tile, uint32_t slice, uint32_t nodes, uint32_t threads,
                   uint32_t target_waves) {
  Tiling t;
  t.threads = threads;
  t.sched.tile = tile;
  t.sched.nchunks = G / slice;
  const uint32_t wpb = threads / 64;
  uint32_t wpc = std::max<uint32_t>(1, target_waves / t.sched.nchunks);
  wpc = std::min<uint32_t>(wpc, std::max<uint32_t>(nodes, 1));
  t.sched.slices_per_tile = std::max<uint32_t>(1, tile / slice);
  // a tile's waves (wpc * slices_per_tile) fill whole workgroups
  while ((uint64_t(wpc) * t.sched.slices_per_tile) % wpb != 0) wpc++;
  t.sched.waves_per_chunk = wpc;
  t.sched.reverse = 0;
  t.sched.per_tile_div = dev::fast_div(wpc * t.sched.slices_per_tile);
  t.sched.spt_div = dev::fast_div(t.sched.slices_per_tile);
  t.sched.tile_div = dev::fast_div(tile);
  t.sched.n_tiles = (t.sched.nchunks + t.sched.slices_per_tile - 1) / t.sched.slices_per_tile;
  t.blocks = static_cast<uint32_t>(uint64_t(wpc) * t.sched.nchunks / wpb);
  return t;
}

// One group's call, from the batch entries through run_any to run_group<T> / run_group_i8.
struct GroupCall {
  const void *llrs;  // the group's input rows (device memory): f32, f64, or 8-bit soft bits (the 8-bit rules only)
  LlrType llrs_type;
  size_t nb;  // codewords of this group
  uint32_t max_iterations;
  uint8_t *bits;
  size_t out_len;
  int32_t *iterations;
  void *posterior;
  hipStream_t stream;
  bool may_block;   // the entry's call may wait on the device; run_any hands on whether this group's host is paced
  bool own_thread;  // the calling thread enqueues this lane's groups only
  bool flood_pace;  // a one-lane call of the device-resident entry: a flooding group's host may follow its progress
  uint32_t pace_lead = 0;  // resolved by run_any: iterations a paced host runs ahead (0: by schedule)
};

// Run-time values as template arguments, each ladder written once: f gets the value as a std::integral_constant.
template <int V>
using int_c = std::integral_constant<int, V>;
template <typename F>
auto with_bool(bool b, F &&f) {
  if (b) return f(std::true_type{});
  return f(std::false_type{});
}
// codewords per lane of the streaming kernels: 4 for f32 only (T = double never instantiates VEC = 4: it lands on 2), 2 or 1
template <typename T, typename F>
auto with_vec(uint32_t vec, F &&f) {
  if constexpr (sizeof(T) == 4)
    if (vec == 4) return f(int_c<4>{});
  if (vec >= 2) return f(int_c<2>{});
  return f(int_c<1>{});
}

// LDS-staged kernels: largest block whose [arrays][dmax][threads] columns fit the CU's LDS
inline bool staged_block(uint32_t arrays, uint32_t dmax, size_t elem, uint32_t *threads, size_t *lds) {
  for (uint32_t t : {256u, 128u, 64u}) {
    const size_t bytes = size_t(arrays) * std::max<uint32_t>(dmax, 1) * t * elem;
    if (bytes <= 64 * 1024 || (t == 64 && bytes <= 160 * 1024)) {
      *threads = t;
      *lds = bytes;
      return true;
    }
  }
  return false;
}


// Rows beyond that: the launch keeps its two columns per wavefront in HBM.  A launch of at most kScratchWaves wavefronts
// (make_tiling rounds a slice's waves up to whole workgroups: the allocation follows the tiling actually used).
constexpr uint32_t kScratchWaves = 2048, kScratchThreads = 256;
inline size_t scratch_bytes_for(const Tiling &t, uint32_t dmax, size_t elem) {
  return size_t(t.blocks) * (t.threads / 64) * 2 * dmax * 64 * elem;
}


// Host view of a group's progress word (kernels.hip.h, State::publish).  finished(it) is asked
// before iteration `it` is enqueued: true when every codeword of the group has finished, so that
// all further launches would return at once.  With `throttle` the host also waits until the device
// is within `lead` iterations -- for small groups the launches are so short that an un-throttled
// host would have enqueued most of max_iterations before the first result is known.
struct ProgressPoll {
  const uint64_t *flag;
  uint32_t epoch;
  bool throttle;
  uint32_t lead;
  hipStream_t stream;
  // a paced call that sees no progress at all for this long stops pacing itself (the rest of the group is enqueued at
  // once, as an unpaced call's is): a caller's stream may be gated behind something the calling thread only releases
  // after the call returns (hipStreamWaitValue, a host callback), and then nothing would ever be published
  static constexpr int64_t kStallNs = 200 * 1000 * 1000;
  mutable bool gave_up = false;

  static uint64_t load(const uint64_t *p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
  // codewords of this group still running, as last published (`all` while nothing of this group has been published)
  uint32_t running(uint32_t all) const {
    if (!flag) return all;
    const uint64_t f = load(flag);
    return (f >> 40) == uint64_t(epoch & 0xFFFFFFu) ? static_cast<uint32_t>(f & 0xFFFFFu) : all;
  }
  bool finished(uint32_t it) const {
    if (!flag) return false;
    const uint64_t mine = uint64_t(epoch & 0xFFFFFFu);
    uint64_t f = load(flag);
    if (throttle && !gave_up && it > lead) {
      uint64_t last = f;
      auto since = std::chrono::steady_clock::now();
      for (uint32_t spins = 1;; spins++) {
        if ((f >> 40) == mine && ((f & 0xFFFFFu) == 0 || ((f >> 20) & 0xFFFFFu) + lead >= it)) break;
        if ((spins & 0x3FFu) == 0) {
          if (hipStreamQuery(stream) != hipErrorNotReady) {
            f = load(flag);  // the stream has drained (or failed): nothing more will be published
            break;
          }
          const auto now = std::chrono::steady_clock::now();
          if (f != last) {
            last = f;
            since = now;
          } else if (std::chrono::duration_cast<std::chrono::nanoseconds>(now - since).count() > kStallNs) {
            gave_up = true;
            break;
          }
        }
        f = load(flag);
      }
    }
    return (f >> 40) == mine && (f & 0xFFFFFu) == 0;
  }
};


// Codewords per lane (1, 2 or 4) of the streaming kernels: a wave covers 64 * vec codewords, and
// those slices must tile the layout tile exactly (a 192-codeword tile takes vec = 1: with 128-wide
// slices its last 64 codewords would belong to no wave).
inline uint32_t pick_vec_for(uint32_t tile, uint32_t max_vec, uint32_t wanted) {
  uint32_t vec = std::min<uint32_t>(std::min(max_vec, std::max<uint32_t>(wanted, 1)), 4);
  if (vec == 3) vec = 2;
  while (vec > 1 && tile % (64 * vec) != 0) vec /= 2;
  return vec;
}

// Launchers of the group kernels that are not templates (kernels_group.hip.h): each is defined -- and its kernel compiled --
// once, in device_decoder.hip; the translation units of the schedules call these.
namespace grp {
void init_group(hipStream_t s, uint32_t *done, int32_t *iters, uint32_t *unsat0, uint32_t *unsat1, uint32_t *n_active,
                uint32_t *n_slots, uint32_t *slot_cw, uint32_t nb, uint32_t G);
void latch(hipStream_t s, uint32_t *done, int32_t *iters, uint32_t *unsat, uint32_t *n_active, int32_t iteration, uint32_t G);
void syndrome_bits(hipStream_t s, uint32_t threads, const uint32_t *row_ptr, const uint32_t *edge_col, uint32_t n_rows,
                   const uint64_t *bits, uint32_t *unsat, const uint32_t *n_active, const uint32_t *n_slots, uint32_t W,
                   uint32_t rows_per_thread);
void compact_plan(hipStream_t s, dev::State st, dev::CompactPlan *plan, uint32_t *movers, uint32_t *holes, uint32_t *fill_cw,
                  uint32_t remaining_iterations, dev::CompactRule rule);
void compact_commit(hipStream_t s, dev::State st, const dev::CompactPlan *plan, uint32_t *unsat0, uint32_t *unsat1,
                    uint32_t *n_slots, const uint32_t *fill_cw, uint32_t G);
}  // namespace grp

// What one group's run has in common under the float and the 8-bit rules (run_group<T>, run_group_i8): the codeword state
// with its progress word, the launches up to the pre-check on the raw input, the syndrome / latch pair that ends an
// iteration, and the emit launch.  The schedule loops between them are each rule family's own.
struct DeviceDecoder::GroupFrame {
  DeviceDecoder &d;
  Workspace &w;
  const GroupCall &c;
  const hipStream_t s;
  const uint32_t G, W, n, m, tile;  // tile: codewords per self-contained sub-batch (kernels.hip.h, tile_base)
  const uint32_t *const row_ptr = d.d_row_ptr_.get<uint32_t>(), *const edge_col = d.d_edge_col_.get<uint32_t>();
  dev::State st;
  const ProgressPoll poll;
  // syndrome launch: a wavefront takes 64 packed words of a few checks; enough wavefronts to fill the chip
  const uint32_t synd_chunks = (W + 63) / 64;
  const uint32_t synd_rows =
      std::max<uint32_t>(1, std::min<uint32_t>(64, uint32_t(uint64_t(m) * synd_chunks * 64 / kSyndThreads)));
  const uint32_t synd_threads = 64 * synd_chunks * ((m + synd_rows - 1) / synd_rows);

  GroupFrame(DeviceDecoder &dec, Workspace &ws, const GroupCall &call, uint32_t tile_)
      : d(dec), w(ws), c(call), s(call.stream), G(static_cast<uint32_t>(ws.G)), W(G / 64), n(static_cast<uint32_t>(dec.n_)),
        m(static_cast<uint32_t>(dec.m_)), tile(tile_),
        st{ws.done, ws.iters, ws.n_active, ws.n_slots, ws.slot_cw, nullptr, 0, 0, nullptr, nullptr, 0},
        poll{(dec.opt_poll_ && ws.d_flag) ? ws.h_flag : nullptr, ws.epoch = (ws.epoch % 0xFFFFFFu) + 1, call.may_block,
             call.pace_lead ? call.pace_lead : (dec.impl_.schedule == Schedule::Layered ? 2u : 8u), call.stream} {}

  dev::Graph graph(const uint32_t *edge_aux, const uint32_t *edge_peer) const {
    return dev::Graph{row_ptr, edge_col, d.d_col_ptr_.get<uint32_t>(), d.d_col_edge_.get<uint32_t>(), m, n, static_cast<uint32_t>(d.e_),
                      nullptr, nullptr,  nullptr,                      0,                              edge_aux, edge_peer};
  }
  // progress word: the first check-node launch of iteration `it` runs with ticked(it)
  dev::State ticked(uint32_t it) const {
    dev::State t = st;
    t.publish = d.opt_poll_ ? w.d_flag : nullptr;
    t.epoch = w.epoch;
    t.tick = it;
    return t;
  }
  void syndrome_of(const uint64_t *hard, uint32_t *unsat) const {
    if (m == 0) return;
    grp::syndrome_bits(s, synd_threads, row_ptr, edge_col, m, hard, unsat, w.n_active, w.n_slots, W, synd_rows);
  }
  void latch(uint32_t *unsat, int32_t it) const { grp::latch(s, w.done, w.iters, unsat, w.n_active, it, G); }
  // the group's first launches: state, ingest (the rule family's kernel for f32 and for f64 input; the 8-bit rules have a
  // third, for rows of 8-bit soft bits), and the pre-check on the raw input: iterations = 0 (flooding.rs:57-64)
  template <typename K32, typename K64, typename C, typename P, typename K8 = std::nullptr_t>
  int begin(K32 ingest_f32, K64 ingest_f64, C *chan, P *post, K8 ingest_i8 = nullptr) const {
    grp::init_group(s, w.done, w.iters, w.unsat0, w.unsat1, w.n_active, w.n_slots, w.slot_cw, static_cast<uint32_t>(c.nb), G);
    const dim3 grid((n + 63) / 64, W);
    const uint32_t block_size = d.pattern_len_ ? n / d.pattern_len_ : 0;
    auto ingest = [&](auto kernel, auto *src) {
      kernel<<<grid, 256, 0, s>>>(src, d.input_len_, static_cast<uint32_t>(c.nb), n, G, tile, chan, post, w.rawbits,
                                  d.d_src_block_.get<int32_t>(), block_size);
    };
    if (c.llrs_type == LlrType::I8) {
      if constexpr (std::is_same<K8, std::nullptr_t>::value) {
        d.fail("internal error: 8-bit soft bits handed to a float rule");
        return -3;
      } else {
        ingest(ingest_i8, static_cast<const int8_t *>(c.llrs));
      }
    } else if (c.llrs_type == LlrType::F64)
      ingest(ingest_f64, static_cast<const double *>(c.llrs));
    else
      ingest(ingest_f32, static_cast<const float *>(c.llrs));
    if (w.after_ingest) {
      if (const hipError_t e = hipEventRecord(w.after_ingest, s); e != hipSuccess) {
        d.fail("hipEventRecord(w.after_ingest, s)", e);
        return -2;
      }
      if (w.ingest_seq) w.ingest_seq->fetch_add(1, std::memory_order_release);
    }
    syndrome_of(w.rawbits, w.unsat0);
    latch(w.unsat0, 0);
    return 0;
  }
  // results to the caller's rows, in the precision of its input (retire_only: a compaction checkpoint's, do_compact its plan)
  // hard, hard_ok ("call_edges"): the last posterior's packed decisions, by slot, and the word that says whether they are
  // valid -- a launch that writes no posterior takes the decisions from them (kernels_group.hip.h, emit_kernel): a block then
  // covers 256 variables of its 64 slots per step, not 64
  template <typename P>
  void emit(const P *post, const uint32_t *do_compact, int zero_fill, int retire_only, const uint64_t *hard = nullptr,
            const uint32_t *hard_ok = nullptr) const {
    const bool from_hard = hard != nullptr && c.posterior == nullptr && !zero_fill && !retire_only;
    const uint32_t blocks_x = from_hard ? (std::min<uint32_t>(n, static_cast<uint32_t>(c.out_len)) + 3) / 4 / 64 + 1 : (n + 63) / 64;
    const dim3 grid(std::min<uint32_t>(blocks_x, retire_only ? kRetireBlocks : 4096), W);
    auto go = [&](auto kernel, auto *out) {
      kernel<<<grid, 256, 0, s>>>(post, w.rawbits, st, do_compact, n, G, tile, static_cast<uint32_t>(c.out_len), c.bits,
                                  c.iterations, out, zero_fill, retire_only, from_hard ? hard : nullptr, hard_ok);
    };
    if constexpr (sizeof(P) == 2) {  // the 8-bit rules: soft-bit input gets the posterior word itself
      if (c.llrs_type == LlrType::I8) return go(dev::emit_kernel<P, int16_t>, static_cast<int16_t *>(c.posterior));
    }
    if (c.llrs_type == LlrType::F64)
      go(dev::emit_kernel<P, double>, static_cast<double *>(c.posterior));
    else
      go(dev::emit_kernel<P, float>, static_cast<float *>(c.posterior));
  }
};

}  // namespace ldpc
