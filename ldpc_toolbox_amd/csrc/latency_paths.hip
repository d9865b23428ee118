// The small-batch paths: one persistent launch per call (latency.hip.h, latency_edge.hip.h) and their kernels.
#include "device_decoder_internal.h"

namespace ldpc {

// ---- small-batch path ------------------------------------------------------------------------
// One persistent launch decodes the whole (small) batch: latency.hip.h.  host_pointers: the caller's buffers
// are staged through one pinned chunk each way on `s` and the call returns synchronised; else everything is
// device memory and the call only enqueues on `s`.
// The kernel's workgroups synchronise with each other, so all of them must be resident together -- one such
// kernel fills the chip's register files.  Two of them at once (two handles driven by two threads, as the
// reference's BER driver drives its worker threads) would each hold part of the chip and wait for the rest:
// the calls are therefore serialised per process, and always return synchronised.  Should the workgroups
// still not come together (another process's kernels hold CUs for longer than the bounded spins allow),
// the kernel gives up with its error word set and the call is redone by the batched kernels (kLatencyRetry).
static std::mutex g_latency_mutex;

// What a call of either small-batch path stages, the same way: the size of the persistent launch, the pinned chunks,
// the error word, and the retreat to the batched kernels.  The paths' tables, state and launches are their own.
struct DeviceDecoder::SmallBatchCall {
  DeviceDecoder &d;
  SmallBatchStaging &st;
  const bool host_pointers;
  const size_t batch;
  // the caller's buffers ...
  const void *const llrs;
  uint8_t *const bits;
  int32_t *const iterations;
  void *const posterior;
  const size_t in_bytes, bits_bytes, post_bytes;
  // ... and what the kernel reads and writes: those (device memory), or the pinned chunks of a host-pointer call
  const void *d_llrs;
  uint8_t *d_bits;
  int32_t *d_iters;
  void *d_post;
  uint32_t *o_err = nullptr;

  SmallBatchCall(DeviceDecoder &dec, SmallBatchStaging &staging, const void *llrs_, LlrType llrs_type, bool host, size_t batch_,
                 uint8_t *bits_, size_t out_len, int32_t *iterations_, void *posterior_)
      : d(dec), st(staging), host_pointers(host), batch(batch_), llrs(llrs_), bits(bits_), iterations(iterations_),
        posterior(posterior_), in_bytes(batch_ * dec.input_len_ * llr_bytes(llrs_type)), bits_bytes(batch_ * out_len),
        post_bytes(batch_ * dec.n_ * posterior_bytes(llrs_type)), d_llrs(llrs_), d_bits(bits_), d_iters(iterations_), d_post(posterior_) {
    d.last_lanes_ = 1;
    d.last_group_ = batch;
    d.last_vn_records_.store(false, std::memory_order_relaxed);
    d.last_vn_bundles_.store(false, std::memory_order_relaxed);
    d.last_vn_bundle_saved_.store(0, std::memory_order_relaxed);
    d.last_vn_chains_.store(false, std::memory_order_relaxed);
    d.last_vn_chain_saved_.store(0, std::memory_order_relaxed);
    d.last_cn_row_shape_.store(false, std::memory_order_relaxed);
    d.last_cn_shape_runs_.store(0, std::memory_order_relaxed);
    d.last_cn_shape_rows_.store(0, std::memory_order_relaxed);
    d.last_record_flag_bytes_.store(0, std::memory_order_relaxed);
  }

  int retreat() {
    d.opt_latency_ = 0;
    d.opt_latency_edge_ = 0;
    return kLatencyRetry;
  }
  // One workgroup of 1024 threads per CU, all of them resident together (the kernel's census waits for all of them, and
  // derives how many share an XCD at run time): the grid is what the device can hold at once of the kernel this handle
  // launches, for f32 and for f64 input -- 256 on an MI355X in SPX mode, fewer on a partitioned or smaller device --
  // and never more than 256.  Fewer than 8 cannot be co-resident in any useful number: the handle keeps the batched kernels.
  // (kernel_i8: the 8-bit rules' third kernel, for rows of 8-bit soft bits; null for the float rules)
  int size_grid(const void *kernel_f32, const void *kernel_f64, const void *kernel_i8 = nullptr) {
    if (st.grid != 0) return 0;
    int cus = 0, per_cu_f = 0, per_cu_d = 0, per_cu_b = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d.device_);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_f, kernel_f32, 1024, 0);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_d, kernel_f64, 1024, 0);
    if (e == hipSuccess && kernel_i8) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_b, kernel_i8, 1024, 0);
    const int resident = e == hipSuccess ? cus * std::min(std::min(per_cu_f, per_cu_d), kernel_i8 ? per_cu_b : per_cu_f) : 0;
    if (resident < 8) return retreat();
    st.grid = static_cast<uint32_t>(std::min(resident, 256));
    return 0;
  }
  // The kernel writes the error word into pinned host memory (system scope), and for host-pointer calls it also
  // reads the input there (its ingest: coalesced, in source order, over the bus) and writes the outputs there:
  // a call is memcpy -> one launch -> memcpy with no copy commands (each costs ~10 us of command latency, as
  // much as ten iterations of the decoder; measured -15..25 us per call, profiles/r02_latency.txt).
  int stage(size_t granule) {
    const size_t iters_at = round_up(256 + bits_bytes, 256), post_at = round_up(iters_at + batch * sizeof(int32_t), 256);
    const size_t out_need = host_pointers ? post_at + (posterior ? post_bytes : 0) : 256;
    if (st.h_out.ensure(out_need, granule) != hipSuccess || (host_pointers && st.h_in.ensure(in_bytes, granule) != hipSuccess)) {
      d.fail("pinned host memory for the small-batch path");
      return -1;
    }
    char *const h_out = st.h_out.get<char>();
    o_err = reinterpret_cast<uint32_t *>(h_out);
    *o_err = 0;
    if (host_pointers) {
      std::memcpy(st.h_in.get(), llrs, in_bytes);
      d_llrs = st.h_in.get();
      d_bits = reinterpret_cast<uint8_t *>(h_out + 256);
      d_iters = reinterpret_cast<int32_t *>(h_out + iters_at);
      d_post = posterior ? static_cast<void *>(h_out + post_at) : nullptr;
    }
    return 0;
  }
  // after the launch has been synchronised
  int finish() {
    if (*o_err != 0) {
      // the workgroups did not come together within the bounded spins (another process holds CUs, or the device
      // is not what the occupancy query promised): do not pay that timeout on every call -- this handle decodes
      // its small batches with the batched kernels from now on
      std::fprintf(stderr, "ldpc_toolbox (hip): the single-launch small-batch path could not get its %u workgroups resident; "
                           "this decoder uses the batched kernels from now on\n", st.grid);
      return retreat();
    }
    if (host_pointers) {
      if (bits_bytes) std::memcpy(bits, d_bits, bits_bytes);
      if (iterations) std::memcpy(iterations, d_iters, batch * sizeof(int32_t));
      if (posterior) std::memcpy(posterior, d_post, post_bytes);
    }
    return 0;
  }
};

int DeviceDecoder::decode_latency(const void *llrs, LlrType llrs_type, bool host_pointers, size_t batch,
                                  uint32_t max_iterations, uint8_t *bits, size_t out_len, int32_t *iterations,
                                  void *posterior, hipStream_t s) {
  std::lock_guard<std::mutex> one_at_a_time(g_latency_mutex);
  LatencyPath &lp = *lat_;
  const SlicedTables &tb = lp.tables;
  SmallBatchCall call(*this, lp.staging, llrs, llrs_type, host_pointers, batch, bits, out_len, iterations, posterior);
  const uint32_t n = static_cast<uint32_t>(n_), m = static_cast<uint32_t>(m_);
  if (!lp.uploaded) {
    hipError_t e = hipSuccess;
    for (auto [v, dst] : {std::pair{&tb.rslice_ptr, &lp.d_rslice_ptr}, {&tb.rdeg, &lp.d_rdeg}, {&tb.col, &lp.d_col},
                          {&tb.vslice_ptr, &lp.d_vslice_ptr}, {&tb.vdeg, &lp.d_vdeg}, {&tb.vedge, &lp.d_vedge},
                          {&tb.perm, &lp.d_perm}, {&tb.inv, &lp.d_inv}}) {
      *dst = upload(*v, &e);
      HIP_TRY(e);
    }
    // per-XCD codeword state, each array on a 256-byte boundary (msg: one word per edge id)
    const size_t a_n = round_up((size_t(n) * 2 + 64) * 4, 256), a_m = round_up((size_t(tb.rslice_ptr.back()) + 8 * 64) * 4, 256),
                 a_h = round_up(n, 256), slot = 2 * a_n + a_m + a_h;
    HIP_TRY(lp.slot_mem.ensure(8 * slot));
    lp.slots.base = lp.slot_mem.get<char>();
    lp.slots.slot_bytes = slot;
    lp.slots.off_post = a_n;
    lp.slots.off_msg = 2 * a_n;
    lp.slots.off_rawhard = 2 * a_n + a_m;
    HIP_TRY(lp.sync.ensure(sizeof(dev::LatencySync)));
    lp.uploaded = true;
  }
  if (int rc = call.stage(LatencyPath::kPinnedGranule)) return rc;
  dev::LatencySync *const d_sync = lp.sync.get<dev::LatencySync>();
  HIP_TRY(hipMemsetAsync(d_sync, 0, sizeof(dev::LatencySync), s));
  auto u32 = [](const DeviceBuffer &b) { return b.get<uint32_t>(); };
  dev::LatencyTables t{n, m, (m + 63) / 64, (n + 63) / 64, u32(lp.d_rslice_ptr), u32(lp.d_rdeg), u32(lp.d_col), u32(lp.d_vslice_ptr),
                       u32(lp.d_vdeg), u32(lp.d_vedge), u32(lp.d_perm), u32(lp.d_inv), d_src_block_.get<int32_t>(),
                       pattern_len_ ? n / pattern_len_ : 0};
  // plain / corrected arithmetic: f(auto... c) gets nothing or the kernel's last argument, and names the kernel
  // latency_minsum_kernel<SrcT, decltype(c)...> (a corrected implementation never takes the plain kernel)
  const dev::MinsumCorr<float> mc{static_cast<float>(impl_.alpha()), static_cast<float>(impl_.beta())};
  auto with_corr = [&](auto f) {
    if (impl_.correction != Correction::None)
      return f(mc);
    return f();
  };
  // (sized by the kernel this handle launches)
  if (int rc = with_corr([&](auto... c) {
        return call.size_grid(reinterpret_cast<const void *>(dev::latency_minsum_kernel<float, decltype(c)...>),
                              reinterpret_cast<const void *>(dev::latency_minsum_kernel<double, decltype(c)...>));
      }))
    return rc;
  const uint32_t grid = lp.staging.grid;
  // one launch, four kernels: the caller's LLR type x plain / corrected arithmetic
  with_corr([&](auto... c) {
    auto go = [&](auto kernel, auto *src, auto *dst) {
      kernel<<<grid, 1024, 0, s>>>(t, lp.slots, d_sync, src, static_cast<uint32_t>(input_len_), static_cast<uint32_t>(batch),
                                   max_iterations, call.d_bits, static_cast<uint32_t>(out_len), call.d_iters, dst, call.o_err, c...);
    };
    if (llrs_type == LlrType::F64)
      go(dev::latency_minsum_kernel<double, decltype(c)...>, static_cast<const double *>(call.d_llrs), static_cast<double *>(call.d_post));
    else
      go(dev::latency_minsum_kernel<float, decltype(c)...>, static_cast<const float *>(call.d_llrs), static_cast<float *>(call.d_post));
    return 0;
  });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  return call.finish();
}

// Largest batch the lane-per-edge path takes: 8 XCDs x the bundle an XCD decodes at once -- as many codewords as keep the
// bundle's state (soft values, messages, channel LLRs) within a few L2s' worth (measured, profiles/r03_latency.txt: 5G NR
// BG1 Zc=384 f32, 0.6 MB per codeword: ahead of the batched kernels up to 64; DVB-S2 1/2 Phif64, 3 MB: up to 32); the
// A-Min* rule's serial fold is repeated by every lane of a row: half of that.
size_t DeviceDecoder::edge_latency_limit() const {
  if (!lat_edge_ || opt_latency_edge_ == 0) return 0;
  const size_t elem = impl_.f64 ? 8 : 4;
  const size_t state = (n_ * (impl_.schedule == Schedule::Layered ? 1 : 2) + edge_lanes_) * elem;
  size_t bundle = std::max<size_t>(1, std::min<size_t>(8, (size_t(12) << 20) / std::max<size_t>(state, 1)));
  if (impl_.rule == Rule::Aminstar) bundle = std::max<size_t>(1, bundle / 2);
  // More codewords than 8 XCDs x bundle take further rounds inside the same launch.  A round costs what the first one
  // did while the batched kernels' time hardly grows with the batch at these sizes, so one extra round is where it ends:
  // BG1 Zc=384 HLTanhf32 128 / 192 / 256 codewords 2.9 / 4.4 / 6.1 ms in two / three / four rounds against 3.4 / 3.9 /
  // 4.7 ms batched, HLMinstarapproxi8 2.7 / 3.9 / 5.4 against 3.3 / 3.5 / 3.7 (profiles/r04_latency.txt; round 3 allowed
  // four rounds on the strength of a batched column timed on a cold chip).  Layered min-sum ties at one round; the
  // flooding schedule on a long code is level with the batched kernels from about 32 codewords (DVB-S2 1/2 Tanhf32:
  // 33 / 64 codewords 3.4 / 5.6 ms against 2.9 / 3.1): half the bundle there.
  if (impl_.schedule == Schedule::Flooding && n_ >= 16384) bundle = std::max<size_t>(1, std::min<size_t>(bundle, 4));
  const size_t rounds = (impl_.schedule == Schedule::Layered && impl_.rule != Rule::Minsum) ? 2 : 1;
  return std::min<size_t>(opt_latency_edge_, 8 * bundle * rounds);
}

// the lane-per-edge path (latency_edge.hip.h): layered schedule, and flooding for everything but Minsumf32
namespace {
// (MC: dev::MinsumCorr<T> with kRuleMinsumCorr -- the kernel then has one more argument -- nothing otherwise)
template <int RULE, typename T, typename SrcT, typename... MC>
const void *edge_kernel_s(bool layered) {
  return with_bool(layered, [](auto L) {
    return reinterpret_cast<const void *>(dev::latency_edge_kernel<RULE, T, SrcT, decltype(L)::value, MC...>);
  });
}
template <typename T, typename SrcT>
const void *edge_kernel_r(Rule rule, bool corrected, bool layered) {
  switch (rule) {
    case Rule::Phi: return edge_kernel_s<dev::kRulePhi, T, SrcT>(layered);
    case Rule::Tanh: return edge_kernel_s<dev::kRuleTanh, T, SrcT>(layered);
    case Rule::Minstarapprox: return edge_kernel_s<dev::kRuleMinstarapprox, T, SrcT>(layered);
    case Rule::Aminstar: return edge_kernel_s<dev::kRuleAminstar, T, SrcT>(layered);
    case Rule::Minsum:
      return corrected ? edge_kernel_s<dev::kRuleMinsumCorr, T, SrcT, dev::MinsumCorr<T>>(layered)
                       : edge_kernel_s<dev::kRuleMinsum, T, SrcT>(layered);
  }
  return nullptr;  // (no such rule: the launch fails)
}
const void *edge_kernel(Rule rule, bool corrected, bool arith_i8, bool arith_f64, LlrType src, bool layered) {
  const bool src_f64 = src == LlrType::F64;
  if (arith_i8) {  // the rule (Minstarapprox / A-Min*) and its options are run-time arguments (dev::I8Opts)
    if (src == LlrType::I8) return edge_kernel_s<dev::kRuleEdgeI8, int32_t, int8_t>(layered);
    return src_f64 ? edge_kernel_s<dev::kRuleEdgeI8, int32_t, double>(layered) : edge_kernel_s<dev::kRuleEdgeI8, int32_t, float>(layered);
  }
  if (src == LlrType::I8) return nullptr;  // (8-bit soft bits go to the 8-bit rules only: the launch fails)
  if (arith_f64)
    return src_f64 ? edge_kernel_r<double, double>(rule, corrected, layered) : edge_kernel_r<double, float>(rule, corrected, layered);
  return src_f64 ? edge_kernel_r<float, double>(rule, corrected, layered) : edge_kernel_r<float, float>(rule, corrected, layered);
}
}  // namespace

int DeviceDecoder::decode_latency_edge(const void *llrs, LlrType llrs_type, bool host_pointers, size_t batch,
                                          uint32_t max_iterations, uint8_t *bits, size_t out_len, int32_t *iterations,
                                          void *posterior, hipStream_t s) {
  std::lock_guard<std::mutex> one_at_a_time(g_latency_mutex);
  EdgeLatencyPath &lp = *lat_edge_;
  const EdgeLaneTables &tb = lp.tables;
  SmallBatchCall call(*this, lp.staging, llrs, llrs_type, host_pointers, batch, bits, out_len, iterations, posterior);
  const size_t elem = impl_.f64 ? 8 : 4;
  const bool corrected = impl_.correction != Correction::None;
  const uint32_t n = static_cast<uint32_t>(n_), m = static_cast<uint32_t>(m_);
  if (!lp.uploaded) {
    hipError_t e = hipSuccess;
    for (auto [v, dst] : {std::pair{&tb.level_chunk, &lp.d_level_chunk}, {&tb.lane_var, &lp.d_lane_var}, {&tb.lane_info, &lp.d_lane_info},
                          {&tb.var_ptr, &lp.d_var_ptr}, {&tb.var_lane, &lp.d_var_lane}}) {
      *dst = upload(*v, &e);
      HIP_TRY(e);
    }
    // per-XCD codeword state, each array on a 256-byte boundary: soft values | messages (one per lane slot) |
    // channel LLRs (flooding) | raw hard decisions
    const size_t a_q = round_up(size_t(n) * elem + 256, 256), a_r = round_up(size_t(tb.n_chunks) * 64 * elem + 256, 256),
                 a_c = tb.layered ? 0 : a_q, a_h = round_up(size_t(n) + 256, 256), slot = a_q + a_r + a_c + a_h;
    HIP_TRY(lp.slot_mem.ensure(size_t(8) * dev::kEdgeBundle * slot));
    lp.slots.base = lp.slot_mem.get<char>();
    lp.slots.slot_bytes = slot;
    lp.slots.off_msg = a_q;
    lp.slots.off_chan = a_q + a_r;
    lp.slots.off_rawhard = a_q + a_r + a_c;
    HIP_TRY(lp.flag_mem.ensure(size_t(8) * 2 * dev::kEdgeBundle * sizeof(uint32_t)));
    lp.slots.flags = lp.flag_mem.get<uint32_t>();
    HIP_TRY(lp.sync.ensure(sizeof(dev::LatencySync)));
    lp.uploaded = true;
  }
  // every workgroup of the persistent launch must be resident (see decode_latency)
  if (int rc = call.size_grid(edge_kernel(impl_.rule, corrected, impl_.i8, impl_.f64, LlrType::F32, tb.layered),
                              edge_kernel(impl_.rule, corrected, impl_.i8, impl_.f64, LlrType::F64, tb.layered),
                              impl_.i8 ? edge_kernel(impl_.rule, corrected, true, false, LlrType::I8, tb.layered) : nullptr))
    return rc;
  if (int rc = call.stage(EdgeLatencyPath::kPinnedGranule)) return rc;
  dev::LatencySync *d_sync = lp.sync.get<dev::LatencySync>();
  HIP_TRY(hipMemsetAsync(d_sync, 0, sizeof(dev::LatencySync), s));
  // up to 8 codewords: one per XCD; more: every XCD takes a bundle of up to kEdgeBundle that share each phase and barrier
  uint32_t bundle = static_cast<uint32_t>(std::min<size_t>(dev::kEdgeBundle, (batch + 7) / 8));
  if (bundle > 1) HIP_TRY(hipMemsetAsync(lp.slots.flags, 0, size_t(8) * 2 * dev::kEdgeBundle * sizeof(uint32_t), s));
  auto u32 = [](const DeviceBuffer &b) { return b.get<uint32_t>(); };
  dev::EdgeLatTables t{n, m, static_cast<uint32_t>(tb.level_chunk.size() - 1), tb.n_chunks, u32(lp.d_level_chunk), u32(lp.d_lane_var),
                       u32(lp.d_lane_info), u32(lp.d_var_ptr), u32(lp.d_var_lane), d_src_block_.get<int32_t>(),
                       pattern_len_ ? n / pattern_len_ : 0};
  uint32_t in_len = static_cast<uint32_t>(input_len_), nb = static_cast<uint32_t>(batch), ol = static_cast<uint32_t>(out_len);
  dev::I8Opts i8o{impl_.rule == Rule::Aminstar, impl_.jones, impl_.hardlimit, impl_.deg1clip};
  // the corrected kernels' last argument, in the decoder's type (the others take the first 14)
  dev::MinsumCorr<float> mc_f{static_cast<float>(impl_.alpha()), static_cast<float>(impl_.beta())};
  dev::MinsumCorr<double> mc_d{impl_.alpha(), impl_.beta()};
  void *args[] = {&t, &lp.slots, &d_sync, &call.d_llrs, &in_len, &nb, &max_iterations, &call.d_bits, &ol, &call.d_iters, &call.d_post,
                  &call.o_err, &bundle, &i8o, impl_.f64 ? static_cast<void *>(&mc_d) : static_cast<void *>(&mc_f)};
  const void *kernel = edge_kernel(impl_.rule, corrected, impl_.i8, impl_.f64, llrs_type, tb.layered);
  if (kernel == nullptr) {
    fail("internal error: no small-batch kernel for this rule");
    return -3;
  }
  HIP_TRY(hipLaunchKernel(kernel, dim3(lp.staging.grid), dim3(1024), args, 0, s));
  HIP_TRY(hipStreamSynchronize(s));
  return call.finish();
}

}  // namespace ldpc
