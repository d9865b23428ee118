// One group of codewords through the float rules, both schedules: DeviceDecoder::run_group<T>.  Instantiated for float in
// run_group_f32.hip and for double in run_group_f64.hip (each compiles its own kernels).
#pragma once
#include "launch.hip.h"

namespace ldpc {

// ---- one group of codewords ----------------------------------------------------------------

template <typename T>
int DeviceDecoder::run_group(Workspace &w, const GroupCall &call) {
  const uint32_t max_iterations = call.max_iterations;
  const size_t nb = call.nb;
  // layout tile: codewords per self-contained sub-batch (kernels.hip.h, tile_base)
  uint32_t tile = opt_tile_ ? opt_tile_ : (sizeof(T) == 4 ? 256 : 128);
  tile = std::max<uint32_t>(64, tile / 64 * 64);
  while (w.G % tile != 0) tile -= 64;
  GroupFrame f(*this, w, call, tile);
  const uint32_t G = f.G, W = f.W, n = f.n, m = f.m;
  const hipStream_t s = f.s;
  const ProgressPoll &poll = f.poll;
  dev::State &st = f.st;
  auto ticked = [&](uint32_t it) { return f.ticked(it); };
  T *chan = static_cast<T *>(w.chan), *post = static_cast<T *>(w.post), *msg = static_cast<T *>(w.msg);
  // default: enough waves that each handles ~4 nodes (oversubscription evens out the tail)
  const uint32_t target_waves = opt_waves_ ? opt_waves_ : 256 * 1024;
  // LDS columns per thread of the staged kernels: the Tanh rule works in one (rule_check_node), the others need
  // the inputs beside the outputs
  const uint32_t lds_columns = impl_.rule == Rule::Tanh ? 1u : 2u;
  const Launch<T> launch{s, max_row_weight_ > 8 || opt_rec_long_, impl_.fast, impl_.correction != Correction::None,
                         dev::MinsumCorr<T>{static_cast<T>(impl_.alpha()), static_cast<T>(impl_.beta())}};
  const dev::Graph g = f.graph(d_edge_aux_.get<uint32_t>(), d_edge_peer_.get<uint32_t>());

  // Whether the call takes the flooding record path, decided before its first launch: "call_edges" trims the launches around
  // that path's iterations when no posterior was asked for (device_decoder.h, opt_call_edges_).
  // (the streaming min-sum kernels keep a row's signs in a 64-bit mask: longer rows take the LDS-staged kernel; the record
  // kernel's buffer addressing carries 32-bit byte offsets inside a tile slice)
  const bool fl_streaming = impl_.schedule == Schedule::Flooding && impl_.rule == Rule::Minsum && !opt_staged_minsum_ &&
                            max_row_weight_ <= 64;
  const bool fl_records = fl_streaming && w.records && w.rec[0] != nullptr &&
                          uint64_t(std::max<size_t>(std::max(e_, n_), m_ * rec_w_)) * tile * sizeof(T) < (1ull << 32);
  const bool edges = opt_call_edges_, edges_no_post = edges && fl_records && call.posterior == nullptr;
  uint32_t edges_ran = 0;
  // (1) nothing reads the posterior array before it is rewritten: the first check-node launch reads the kept variables' rows,
  // which equal the channel's, and stores none; the first variable-node launch writes every kept row of every running
  // codeword; the L-free rows are stored before they are read (State::slice_state); a frame that passes the pre-check is
  // emitted from rawbits.  So the ingest launch stores the input once, and the first check-node launch reads `chan` twice.
  const bool ingest_no_post = edges_no_post;
  if (ingest_no_post) edges_ran |= kCallEdgeIngest;
  if (int rc = f.begin(dev::ingest_kernel<float, T>, dev::ingest_kernel<double, T>, chan, ingest_no_post ? static_cast<T *>(nullptr) : post))
    return rc;
  // (one codeword per lane: the paired-load form of the 16-bit posterior, pack_hard_pair_kernel, is slower here --
  // 210 vs 191 us for 8192 x BG1 Zc=384: 256-byte requests already stream, the exchange only adds work)
  // (16 K waves by default: the launch runs once per layered iteration and its waves are short -- at the 256 K of the other
  // launches a wave packs six rows and is gone; 5G NR BG1 Zc=384 HLTanhf32 +0.7 % over three alternating pairs, round 5)
  const Tiling pack_t = make_tiling(G, tile, 64, n, 256, std::min<uint32_t>(target_waves, kPackWaves));
  // (rows: the leading rows packed; ran: where the launch says whether it packed -- "call_edges", pack_hard_kernel)
  auto pack = [&](const T *soft, uint32_t rows, uint32_t *ran) {
    dev::pack_hard_kernel<T><<<pack_t.blocks, pack_t.threads, 0, s>>>(soft, w.hardbits, w.n_active, w.n_slots, n, tile,
                                                                      W, pack_t.sched.waves_per_chunk, rows, ran);
  };

  const uint64_t *emit_hard = nullptr;  // set where the last pack's words serve the final emit launch ("call_edges")
  auto emit = [&](int zero_fill, int retire_only) {
    f.emit(post, &w.plan->do_compact, zero_fill, retire_only, retire_only ? nullptr : emit_hard, w.hard_ok);
  };
  // batch compaction checkpoint (kernels.hip.h): everything decided on the device
  const Tiling mv_t = make_tiling(G, tile, 64, n, 256, kMoveWaves);
  uint32_t post_move_rows = 0;  // 0 = all rows; set by the flooding L-free paths below
  // (flags, flag_rows: the 16-bit flags of flooding row records, which travel with their magnitudes in msg_cur; flags8: the
  // same array holds bytes)
  auto compact = [&](uint32_t remaining, T *msg_cur, bool with_chan, uint32_t msg_rows, uint16_t *flags = nullptr,
                     uint32_t flag_rows = 0, bool flags8 = false) {
    grp::compact_plan(s, ticked(max_iterations - remaining), w.plan, w.perm, w.slot_tmp, w.fill_cw, remaining,
        dev::CompactRule{kCompactHorizon, kCompactCostLive, kCompactCostSlots, kCompactMinFreedQ});
    if (edges) {
      // "call_edges": two launches behind the plan (kernels_group.hip.h, compact_retire_move_kernel): the retire-emit with the
      // movers of everything but the posterior, then the posterior's mover with the commit
      edges_ran |= kCallEdgeCheckpoint;
      dev::MoveList<T> rest{}, pm{};
      auto add_to = [](dev::MoveList<T> &l, T *arr, uint32_t rows, uint32_t moved) {
        l.arr[l.count] = arr;
        l.rows[l.count] = rows;
        l.moved[l.count++] = moved;
      };
      if (with_chan) add_to(rest, chan, n, n);
      if (msg_rows) add_to(rest, msg_cur, msg_rows, msg_rows);
      add_to(pm, post, n, post_move_rows ? post_move_rows : n);
      const uint32_t emit_nbx = std::min<uint32_t>((n + 63) / 64, kRetireBlocks);
      const uint32_t emit_blocks = std::min<uint32_t>(emit_nbx * W, kEdgeRetireBlocks);
      const uint32_t commit_blocks = (G + 255) / 256;
      auto retire_move = [&](auto fw, auto *out) {
        using FW = decltype(fw);
        dev::MoveList<FW> fl{};
        if (flags) fl = dev::MoveList<FW>{{reinterpret_cast<FW *>(flags)}, {flag_rows}, {flag_rows}, 1};
        using OutT = std::remove_pointer_t<decltype(out)>;
        dev::compact_retire_move_kernel<T, OutT, FW><<<emit_blocks + kEdgeMoveBlocks, 256, 0, s>>>(
            w.plan, post, w.rawbits, st, n, G, tile, static_cast<uint32_t>(call.out_len), call.bits, call.iterations, out,
            emit_blocks, emit_nbx, w.perm, w.slot_tmp, rest, fl, mv_t.sched.nchunks, mv_t.sched.waves_per_chunk);
      };
      auto with_out = [&](auto fw) {
        if (call.llrs_type == LlrType::F64)
          retire_move(fw, static_cast<double *>(call.posterior));
        else
          retire_move(fw, static_cast<float *>(call.posterior));
      };
      if (flags && flags8)
        with_out(uint8_t{});
      else
        with_out(uint16_t{});
      dev::compact_post_commit_kernel<T><<<commit_blocks + kEdgeMoveBlocks, 256, 0, s>>>(
          st, w.plan, w.unsat0, w.unsat1, w.n_slots, w.fill_cw, G, commit_blocks, w.perm, w.slot_tmp, pm, tile,
          mv_t.sched.nchunks, mv_t.sched.waves_per_chunk);
      return;
    }
    emit(0, 1);
    dev::MoveList<T> ml{};
    auto add = [&](T *arr, uint32_t rows, uint32_t moved) {
      ml.arr[ml.count] = arr;
      ml.rows[ml.count] = rows;
      ml.moved[ml.count++] = moved;
    };
    if (with_chan) add(chan, n, n);
    // (flooding min-sum with L-free variables: the posterior of a degree <= 2 variable is rebuilt by the next check-node pass
    // from the channel LLR and the records / messages before anything reads it -- every slice stores them after a commit --
    // so the rows beyond the last variable the variable-node kernel writes need not travel: DVB-S2's staircase, 5G NR's
    // extension parity: half of the posterior rows, 14 % of what a mover carries)
    add(post, n, post_move_rows ? post_move_rows : n);
    if (msg_rows) add(msg_cur, msg_rows, msg_rows);
    dev::compact_move_kernel<T><<<mv_t.blocks, mv_t.threads, 0, s>>>(w.plan, w.perm, w.slot_tmp, ml, tile,
                                                                     mv_t.sched.nchunks, mv_t.sched.waves_per_chunk);
    if (flags && flags8) {
      const dev::MoveList<uint8_t> fl{{reinterpret_cast<uint8_t *>(flags)}, {flag_rows}, {flag_rows}, 1};
      dev::compact_move_kernel<uint8_t><<<mv_t.blocks, mv_t.threads, 0, s>>>(w.plan, w.perm, w.slot_tmp, fl, tile,
                                                                           mv_t.sched.nchunks, mv_t.sched.waves_per_chunk);
    } else if (flags) {
      const dev::MoveList<uint16_t> fl{{flags}, {flag_rows}, {flag_rows}, 1};
      dev::compact_move_kernel<uint16_t><<<mv_t.blocks, mv_t.threads, 0, s>>>(w.plan, w.perm, w.slot_tmp, fl, tile,
                                                                            mv_t.sched.nchunks, mv_t.sched.waves_per_chunk);
    }
    grp::compact_commit(s, st, w.plan, w.unsat0, w.unsat1, w.n_slots, w.fill_cw, G);
  };
  auto checkpoint_due = [&](uint32_t it) {
    if (!opt_compact_ || max_iterations < 12 || it + 4 > max_iterations) return false;
    // (0 = by schedule.  The layered schedule converges in a third of the iterations flooding needs, and a frame is
    // latched in the iteration it converges in: checkpoints from iteration 3 on, every iteration -- BASELINE config 3 at
    // +2 dB, where no frame runs more than 6 iterations: 323 k -> 331 k codewords/s, tools/c3_p2_sweep.py)
    const bool layered = impl_.schedule == Schedule::Layered;
    const uint32_t first = opt_compact_first_ ? opt_compact_first_ : (layered ? 3u : 6u);
    const uint32_t every = opt_compact_every_ ? opt_compact_every_ : (layered ? 1u : 2u);
    if (it < first) return false;
    return it <= 26 ? (it - first) % every == 0 : it % 4 == 0;
  };

  uint32_t *unsat[2] = {w.unsat0, w.unsat1};
  int zero_fill = 0;
  last_record_flag_bytes_.store(0, std::memory_order_relaxed);  // (the flooding record path says what it ran)
  last_cn_row_shape_.store(false, std::memory_order_relaxed);

  if (impl_.schedule == Schedule::Flooding) {
    const bool streaming = fl_streaming;  // (decided above)
    const uint32_t vec = pick_vec_for(tile, sizeof(T) == 4 ? 4 : 2, opt_vec_);
    const uint32_t stream_block = kStreamBlock;
    const Tiling vn_t = make_tiling(G, tile, 64 * vec, n, stream_block, opt_waves_ ? opt_waves_ : kVnWaves);
    Tiling cn_t = make_tiling(G, tile, 64 * vec, m, stream_block, target_waves);
    uint32_t st_threads = 256;
    size_t st_lds = 0;
    T *cn_scratch = nullptr;  // non-null: the LDS-staged kernel keeps its columns there
    if (!streaming) {
      if (staged_block(lds_columns, max_row_weight_, sizeof(T), &st_threads, &st_lds)) {
        cn_t = make_tiling(G, tile, 64, m, st_threads, target_waves);
      } else {
        // rows beyond the LDS: the columns live in HBM, one region per wavefront of a small launch
        st_threads = kScratchThreads;
        st_lds = 0;
        cn_t = make_tiling(G, tile, 64, m, st_threads, std::min(target_waves, kScratchWaves));
        if (int rc = ensure_row_scratch(w, scratch_bytes_for(cn_t, max_row_weight_, sizeof(T)))) return rc;
        cn_scratch = w.row_scratch.get<T>();
      }
    }
    // the Tanh rule on graphs with rows of at most 12 edges: rows in registers (cn_reg_kernel: 32-bit byte offsets inside
    // a tile slice).  Measured (round 4, 0.xxx of the roofline, cn_staged_kernel -> cn_reg_kernel): DVB-S2 1/2 Tanhf32
    // 0.455 -> 0.469, Tanhf64 0.410 -> 0.417, CCSDS AR4JA 1/2 Tanhf32 0.478 -> 0.479; the other rules lose 0-2 % and 5G NR
    // BG1's mixed 3..19-edge rows in one 24-edge bucket 15 %, so they keep cn_staged_kernel.
    const uint32_t cn_reg = (streaming || !opt_cn_reg_ || !d_row_recs_ || impl_.rule != Rule::Tanh || impl_.fast ||
                             uint64_t(std::max(e_, n_)) * tile * sizeof(T) >= (1ull << 32))
                                ? 0u
                                : (max_row_weight_ <= 10 ? 10u : (max_row_weight_ <= 12 ? 12u : 0u));
    const bool wide_mask = max_row_weight_ > 32;
    // row records instead of per-edge messages on the check-node side (kernels.hip.h, cn_minsum_rec_kernel)
    // (its buffer addressing carries 32-bit byte offsets inside a tile slice)
    const bool records = fl_records;  // (decided above)
    const bool lfree = streaming && lfree_ready_ && opt_lfree_ && (w.msg2 != nullptr || records);
    T *mbuf[2] = {msg, (lfree && !records) ? static_cast<T *>(w.msg2) : msg};
    // (16-bit flags, rows of at most 12 edges: w.rec_flags holds them, w.rec the magnitudes alone)
    // "flags8": rows of at most 7 edges store those flags as bytes, in the first half of the same arrays (record_flags8.h); one
    // decision for every launch of the call -- the long-row variant of the record kernel ("rec_long") has no byte form
    const bool flags8 = records && w.rec_flags[0] != nullptr && opt_flags8_ && !launch.rec_long &&
                        record_flag_bytes(max_row_weight_, sizeof(T) == 8) == 1;
    if (records) last_record_flag_bytes_.store((flags8 ? 1u : (w.rec_flags[0] ? 2u : uint32_t(sizeof(T)))),
                                  std::memory_order_relaxed);
    const typename Launch<T>::Records rbuf[2] = {{static_cast<T *>(w.rec[0]), w.rec_flags[0], rec_w_, flags8},
                                                 {static_cast<T *>(w.rec[1]), w.rec_flags[1], rec_w_, flags8}};
    const uint32_t rec_rows = w.rec_flags[0] ? 2 * m : m * rec_w_;  // rows of T a compaction moves
    if (lfree && post_rows_keep_ > 0 && post_rows_keep_ <= n) post_move_rows = post_rows_keep_;
    // "vn_records": the variable-node launch sums the kept variables from this iteration's records and the check-node launch
    // stores no per-edge messages (vn_kernel's record form); with 16-bit flags only
    const bool vn_records = records && w.rec_flags[0] != nullptr && d_keep_rs_ && opt_vn_records_;
    last_vn_records_.store(vn_records, std::memory_order_relaxed);
    bool vn_bundles = false;  // (decided below, where the kept list's tiling is known)
    const bool quiet = records && opt_rec_quiet_;
    if (quiet) {
      st.slice_state = w.slice_state;
      HIP_TRY(hipMemsetAsync(w.slice_state, 0, size_t(G / 64) * sizeof(uint32_t), s));
    }
    const uint32_t rec_run = std::max<uint32_t>(1, std::min<uint32_t>(opt_rec_run_, m));
    const Tiling rec_t = make_tiling(G, tile, 64 * vec, (m + rec_run - 1) / rec_run, stream_block, target_waves);
    // "cn_row_shape": the record kernel's row-shape form behind the first iteration (launch.hip.h, cn_rec), where the form
    // exists -- f32, byte flags, no per-edge messages -- and some run of this call's walk conforms
    uint32_t shape_runs = 0, shape_rows = 0;
    if (vn_records && flags8 && opt_cn_row_shape_ && sizeof(T) == 4 && row_shape_span_.size() == m)
      count_row_shape_runs(row_shape_span_, m, rec_run, &shape_runs, &shape_rows);
    const bool cn_shape = shape_runs != 0 && max_iterations > 1;
    last_cn_row_shape_.store(cn_shape, std::memory_order_relaxed);
    last_cn_shape_runs_.store(cn_shape ? shape_runs : 0, std::memory_order_relaxed);
    last_cn_shape_rows_.store(cn_shape ? shape_rows : 0, std::memory_order_relaxed);
    dev::Graph g_keep = g, g_free = g;
    Tiling vn_keep_t = vn_t, vn_free_t = vn_t, vn_event_t = vn_t;
    if (lfree) {
      g_keep.list_var = d_keep_var_.get<uint32_t>();
      g_keep.list_ptr = d_keep_ptr_.get<uint32_t>();
      g_keep.list_edge = records ? d_keep_pos_.get<uint32_t>() : d_keep_edge_.get<uint32_t>();  // records: the messages are stored in this list's order
      g_keep.n_list = n_keep_;
      g_free.list_var = d_free_var_.get<uint32_t>();
      g_free.list_ptr = d_free_ptr_.get<uint32_t>();
      g_free.list_edge = d_free_edge_.get<uint32_t>();
      g_free.n_list = n_free_;
      const uint32_t wv = opt_waves_ ? opt_waves_ : kVnWaves;
      vn_keep_t = make_tiling(G, tile, 64 * vec, n_keep_, stream_block, wv);
      vn_keep_t.sched.reverse = 1u;  // tiles last to first: the ones the check-node pass wrote last are still in the Infinity Cache (+0.3 %)
      vn_free_t = make_tiling(G, tile, 64 * vec, n_free_, stream_block, wv);
      vn_event_t = make_tiling(G, tile, 64 * vec, n_free_, stream_block, 16 * 1024);
    }
    // "vn_bundles": the record form walks the kept list in bundles (graph_tables.h, build_vn_bundles).  The message form and the
    // event block keep g_keep; post_rows_keep_ is about variable numbers, not list positions.
    dev::Graph g_bundle = g_keep;
    uint32_t bundle_saved = 0, chain_rs_at = 0;
    if (vn_records && opt_vn_bundles_ && bundle_rs_at_ != 0) {
      vn_bundles = true;
      g_bundle.list_var = d_keep_rs_.get<uint32_t>() + bundle_var_at_;
      g_bundle.list_ptr = d_keep_rs_.get<uint32_t>() + bundle_ptr_at_;
      // the waves of a workgroup that see the same codewords: they sum an aligned run of this many list entries per step
      const uint32_t bundle_w = std::max<uint32_t>(1, (stream_block / 64) / vn_keep_t.sched.slices_per_tile);
      bundle_saved = vn_bundle_saved_[std::min(bundle_w, kVnBundleW)];
    }
    last_vn_bundles_.store(vn_bundles, std::memory_order_relaxed);
    last_vn_bundle_saved_.store(bundle_saved, std::memory_order_relaxed);
    // "vn_chains": the bundled walk in chains (graph_tables.h, build_vn_chains): the chained list and its keep_rs, and a launch
    // whose waves follow from the list's blocks
    dev::VnChain chain{};
    Tiling vn_chain_t = vn_keep_t;
    uint32_t chain_saved = 0;
    bool vn_chains = false;
    if (vn_bundles && opt_vn_chains_) {
      const VnChainAt &at = vn_chain_at_[opt_vn_chain_len_ == kVnChainLens[0] ? 0 : (opt_vn_chain_len_ == kVnChainLens[1] ? 1 : 2)];
      if (at.rs_at != 0) {
        vn_chains = true;
        chain.len = opt_vn_chain_len_;
        chain.width = kVnBundleW;
        chain.n_blocks = at.n_blocks;
        vn_chain_t = Launch<T>::chain_tiling(G, tile, 64 * vec, stream_block, opt_waves_ ? opt_waves_ : kVnWaves, &chain);
        vn_chain_t.sched.reverse = 1u;
        g_bundle.list_var = d_keep_rs_.get<uint32_t>() + at.var_at;
        g_bundle.list_ptr = d_keep_rs_.get<uint32_t>() + at.ptr_at;
        chain_rs_at = at.rs_at;
        chain_saved = chain.mates == kVnBundleW ? at.saved : at.saved_alone;
      }
    }
    last_vn_chains_.store(vn_chains, std::memory_order_relaxed);
    last_vn_chain_saved_.store(chain_saved, std::memory_order_relaxed);
    // a paced host (run_any) sees the group's running count: once the first codewords have converged, every iteration
    // ends with a checkpoint (the device still decides whether re-packing pays)
    const bool adaptive = opt_compact_ && poll.flag != nullptr && poll.throttle && !opt_compact_every_;
    bool seen_drop = false;
    auto tail_checkpoint = [&](uint32_t it) {
      const uint32_t first_ck = opt_compact_first_ ? opt_compact_first_ : 6u;
      return seen_drop && max_iterations >= 12 && it + 4 <= max_iterations && it >= first_ck;
    };
    for (uint32_t it = 1; it <= max_iterations; it++) {
      if (it > 1 && poll.finished(it)) break;  // everything below would return at once
      if (adaptive && !seen_drop && poll.running(static_cast<uint32_t>(nb)) < nb) seen_drop = true;
      const bool first = it == 1;
      uint32_t *unsat_out = unsat[it & 1];
      T *m_out = mbuf[it & 1];
      const T *m_in = mbuf[(it + 1) & 1];
      const dev::State stp = ticked(it);
      timed_begin(kKernelCheck, s);
      if (records)
        // (first && ingest_no_post: the kept variables' rows from `chan`; the FIRST form stores no posterior)
        launch.cn_rec(first, vec, rec_t, g, stp, chan, (first && ingest_no_post) ? chan : post, rbuf[(it + 1) & 1], rbuf[it & 1],
                      msg, unsat_out, rec_run, !vn_records, (cn_shape && !first) ? row_shape_kind_ : uint32_t(kRowShapeNone));
      else if (lfree)
        launch.cn_lfree(first, vec, wide_mask, cn_t, g, stp, chan, post, m_in, m_out, unsat_out);
      else if (streaming)
        launch.cn_minsum(first, vec, wide_mask, cn_t, g, stp, first ? chan : post, msg, unsat_out);
      else
        launch.cn_staged(first, impl_.rule, cn_reg, d_row_recs_.get<uint32_t>(), cn_t, st_lds, cn_scratch, g, stp, first ? chan : post, msg,
                         unsat_out, max_row_weight_);
      timed_end(kKernelCheck, s);
      timed_begin(kKernelVar, s);
      // (deferred L-free stores: the first convergences of a slice get their L-free posteriors from the records of the latched
      // iteration INSIDE this launch -- rounds 3-4 ran a small vn_free_rec_kernel launch behind it in every iteration, which
      // almost always found nothing: 4.4 us + a 5.7 us dispatch gap per iteration)
      if (vn_records) {
        const bool event = quiet && it > 1 && opt_vn_event_;
        launch.vn_rec(vec, vn_chains ? vn_chain_t : vn_keep_t, vn_bundles ? g_bundle : g_keep, st, chan, rbuf[it & 1],
                      d_keep_rs_.get<uint32_t>() + (vn_chains ? chain_rs_at : (vn_bundles ? bundle_rs_at_ : 0u)), post,
                      first ? nullptr : unsat_out, unsat[(it + 1) & 1], static_cast<int32_t>(it) - 1, d_free_var_.get<uint32_t>(),
                      d_free_rs_.get<uint32_t>(), event ? &rbuf[(it - 1) & 1] : nullptr, n_free_, vn_chains ? &chain : nullptr);
        if (quiet && it > 1 && !event)
          launch.vn_free_rec(vec, vn_event_t, g_free, st, d_free_rs_.get<uint32_t>(), chan, rbuf[(it - 1) & 1], post,
                             static_cast<int32_t>(it) - 1);
      } else if (quiet && it > 1 && opt_vn_event_) {
        launch.vn_event(vec, vn_keep_t, g_keep, st, chan, m_out, post, unsat_out, unsat[(it + 1) & 1],
                        static_cast<int32_t>(it) - 1, d_free_var_.get<uint32_t>(), d_free_rs_.get<uint32_t>(), rbuf[(it - 1) & 1],
                        n_free_);
      } else {
        launch.vn(lfree, vec, lfree ? vn_keep_t : vn_t, lfree ? g_keep : g, st, chan, m_out, post,
                  first ? nullptr : unsat_out, unsat[(it + 1) & 1], static_cast<int32_t>(it) - 1);
        if (quiet && it > 1)
          launch.vn_free_rec(vec, vn_event_t, g_free, st, d_free_rs_.get<uint32_t>(), chan, rbuf[(it - 1) & 1], post,
                             static_cast<int32_t>(it) - 1);
      }
      timed_end(kKernelVar, s);
      if (checkpoint_due(it) || tail_checkpoint(it)) {
        // what the next iteration reads: the records of this one (the per-edge messages have been consumed)
        if (records)
          compact(max_iterations - it, rbuf[it & 1].mag, true, rec_rows, w.rec_flags[it & 1], m, flags8);
        else
          compact(max_iterations - it, m_out, true, static_cast<uint32_t>(e_));
      }
    }
    // (2) the end of a call without a posterior: only the sign of the L-free variables' last posteriors is needed -- for the
    // last syndrome and for the caller -- so the pack covers the rows the variable-node launch writes, the closing launch
    // ballots the L-free variables' decisions into the packed words without storing a row (it runs BEHIND the pack: an L-free
    // variable may lie among the packed rows), and the final emit launch reads the packed words
    const bool close_hard = edges_no_post && records && lfree && max_iterations > 0;
    if (close_hard) {
      edges_ran |= kCallEdgeClose | kCallEdgeEmit;
      pack(post, post_move_rows ? post_move_rows : n, w.hard_ok);
      launch.vn_free_hard(vec, vn_free_t, g_free, st, d_free_rs_.get<uint32_t>(), chan, rbuf[max_iterations & 1], post, w.hardbits, W);
      emit_hard = w.hardbits;
    } else if (records && max_iterations > 0) {
      launch.vn_free_rec(vec, vn_free_t, g_free, st, d_free_rs_.get<uint32_t>(), chan, rbuf[max_iterations & 1], post, -1);
    } else if (lfree && max_iterations > 0) {
      // posterior of the L-free variables after the last iteration (no later check-node pass
      // rebuilds it): one variable-node pass over just them; frozen codewords are skipped
      dev::State st_nolatch = st;
      launch.vn(true, vec, vn_free_t, g_free, st_nolatch, chan, mbuf[max_iterations & 1], post, nullptr, w.scratch_flags, -1);
    }
    if (max_iterations > 0) {
      // syndrome of the last posterior (flooding.rs:69-79 at iteration == max_iterations)
      if (!close_hard) pack(post, n, nullptr);
      uint32_t *u = unsat[(max_iterations + 1) & 1];
      f.syndrome_of(w.hardbits, u);
      f.latch(u, static_cast<int32_t>(max_iterations));
    } else {
      zero_fill = 1;
    }
  } else {
    uint32_t threads = 64;
    size_t lds = 0;
    // (min-sum streams its rows whatever their length -- unless "staged_minsum" sends it through the LDS-staged kernel)
    const bool streaming = impl_.rule == Rule::Minsum && !opt_staged_minsum_;
    if (!staged_block(lds_columns, max_row_weight_, sizeof(T), &threads, &lds) && !streaming) {
      // some level has rows beyond the LDS: those levels keep their columns in HBM (a small launch, one region per wave)
      const size_t waves_bound = size_t(kScratchWaves) + size_t(G / 64) * (kScratchThreads / 64);
      if (int rc = ensure_row_scratch(w, waves_bound * 2 * max_row_weight_ * 64 * sizeof(T))) return rc;
    }
    const uint32_t n_levels = level_ptr_.empty() ? 0 : static_cast<uint32_t>(level_ptr_.size() - 1);
    const dev::State st0 = st;
    const uint32_t vec = pick_vec_for(tile, sizeof(T) == 4 ? 4 : 2, opt_vec_);
    // Row-serial mode: when the dependency levels are (almost) single rows -- DVB-S2's staircase
    // chains every row to the next -- one launch per level is launch-bound (32 400 launches per
    // iteration).  Codewords are independent, so ONE wave per codeword slice can walk all rows in
    // level order by itself: one launch per iteration, no inter-wave ordering needed.
    const bool serial = n_levels > opt_serial_levels_;
    const uint32_t n_launch = serial ? std::min<uint32_t>(n_levels, 1) : n_levels;
    // layered min-sum: row records instead of per-edge R (kernels.hip.h, hl_minsum_rec_kernel) when every row fits the
    // three-word record and the register-resident form, and the records fit the message array
    const bool hl_rec = streaming && opt_hl_records_ && opt_hl_reg_ && max_row_weight_ <= (sizeof(T) == 4 ? 26u : 58u) &&
                        Launch<T>::hl_reg_bucket(max_row_weight_) != 0 && m_ * 3 <= e_ &&
                        uint64_t(std::max(n_, m_ * 3)) * tile * sizeof(T) < (1ull << 32);
    for (uint32_t it = 1; it <= max_iterations; it++) {
      if (it > 1 && poll.finished(it)) break;
      const dev::State stp = ticked(it);
      for (uint32_t l = 0; l < n_launch; l++) {
        const dev::State &st = l == 0 ? stp : st0;
        const uint32_t r0 = serial ? 0 : level_ptr_[l], cnt = serial ? m : level_ptr_[l + 1] - level_ptr_[l];
        const uint32_t lmaxdeg = serial ? max_row_weight_ : level_maxdeg_[l];
        const uint32_t tnodes = serial ? 1 : cnt;        // serial: one wave per slice (make_tiling: wpc = 1)
        const uint32_t sblock = serial ? 64 : 256;
        const uint32_t reg_dmax = opt_hl_reg_ ? Launch<T>::hl_reg_bucket(lmaxdeg) : 0;
        if (hl_rec) {
          // the row's messages as one record in the message array (every level qualifies, or none does)
          const uint32_t rvec = Launch<T>::hl_rec_vec(vec, reg_dmax);
          const Tiling t = make_tiling(G, tile, 64 * rvec, tnodes, sblock, target_waves);
          timed_begin(kKernelLayer, s);
          const bool launched = launch.hl_minsum_rec(it == 1, rvec, reg_dmax, t, g, st, d_level_rows_.get<uint32_t>() + r0, cnt, post, msg);
          timed_end(kKernelLayer, s);
          if (!launched) {
            fail("internal error: no row-record layered kernel for this level");
            return -3;
          }
          continue;
        }
        if (streaming && reg_dmax) {
          const uint32_t rvec = Launch<T>::hl_reg_vec(vec, reg_dmax);
          const Tiling t = make_tiling(G, tile, 64 * rvec, tnodes, sblock, target_waves);
          timed_begin(kKernelLayer, s);
          const bool launched = launch.hl_minsum_reg(it == 1, rvec, reg_dmax, t, g, st, d_level_rows_.get<uint32_t>() + r0, cnt, post, msg);
          timed_end(kKernelLayer, s);
          if (!launched) {
            fail("internal error: no register-resident layered kernel for this level");
            return -3;
          }
          continue;
        }
        if (streaming) {
          const Tiling t = make_tiling(G, tile, 64 * vec, tnodes, sblock, target_waves);
          timed_begin(kKernelLayer, s);
          launch.hl_minsum(it == 1, vec, t, g, st, d_level_rows_.get<uint32_t>() + r0, cnt, post, msg);
          timed_end(kKernelLayer, s);
          continue;
        }
        // per level: LDS columns only as tall as this level's longest row (more workgroups per
        // CU for the short-row levels), and the register-resident form when the rows fit it
        const uint32_t ldmax = std::max<uint32_t>(lmaxdeg, 1);
        uint32_t lthreads = threads;
        size_t llds = lds;
        const bool lfits = staged_block(lds_columns, ldmax, sizeof(T), &lthreads, &llds);
        if (serial) {
          lthreads = 64;
          llds = size_t(lds_columns) * ldmax * 64 * sizeof(T);
        }
        if (!lfits) {
          lthreads = serial ? 64 : kScratchThreads;
          llds = 0;
        }
        // (the register-resident form addresses Qv and R through buffer descriptors with 32-bit byte offsets
        // inside a tile slice: graphs too large for that take the two-pass kernel)
        const bool fits32 = uint64_t(std::max(e_, n_)) * tile * sizeof(T) < (1ull << 32);
        // (a 10-edge bucket beside 12 and 24: 5G NR's extension rows have at most 10 edges, and the two registers per
        // edge it saves decide whether the Tanh rule's kernel keeps 7 or 8 waves per SIMD)
        const uint32_t lreg = (!opt_hl_reg_ || !fits32) ? 0 : (ldmax <= 10 ? 10 : (ldmax <= 12 ? 12 : (ldmax <= 24 ? 24 : 0)));
        // (the register-resident kernels read a level's row records, the two-pass kernel the row list)
        const uint32_t *ltab = !lreg ? d_level_rows_.get<uint32_t>() + r0 : (serial ? d_serial_recs_.get<uint32_t>() : d_level_recs_.get<uint32_t>() + level_rec_ptr_[l]);
        const Tiling t = make_tiling(G, tile, 64, tnodes, lthreads, lfits ? target_waves : std::min(target_waves, kScratchWaves));
        if (!lfits && scratch_bytes_for(t, ldmax, sizeof(T)) > w.row_scratch.capacity()) {
          fail("internal error: row scratch smaller than a level's launch");
          return -3;
        }
        timed_begin(kKernelLayer, s);
        launch.hl(it == 1, impl_.rule, lreg, t, llds, lfits ? nullptr : w.row_scratch.get<T>(), g, st, ltab, cnt, post,
                  msg, ldmax);
        timed_end(kKernelLayer, s);
      }
      // horizontal_layered.rs:66-78
      pack(post, n, nullptr);
      f.syndrome_of(w.hardbits, w.unsat0);
      f.latch(w.unsat0, static_cast<int32_t>(it));
      if (checkpoint_due(it)) compact(max_iterations - it, msg, false, hl_rec ? m * 3 : static_cast<uint32_t>(e_));
    }
  }

  emit(zero_fill, 0);
  last_call_edges_.fetch_or(edges_ran, std::memory_order_relaxed);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace ldpc
