// The 8-bit quantised rules: DeviceDecoder::run_group_i8 and every kernel it launches (kernels_i8.hip.h,
// kernels_i8_minsum.hip.h).
#define LDPC_I8_KERNELS_TU 1  // this translation unit compiles the 8-bit rules' one non-template kernel
#include "device_decoder_internal.h"
#include "kernels_i8.hip.h"
#include "kernels_i8_minsum.hip.h"

namespace ldpc {

// ---- one group of codewords, 8-bit quantised arithmetics (kernels_i8.hip.h) ------------------

int DeviceDecoder::run_group_i8(Workspace &w, const GroupCall &call) {
  const uint32_t max_iterations = call.max_iterations;
  GroupFrame f(*this, w, call, 256);
  const uint32_t G = f.G, n = f.n, m = f.m, tile = f.tile;
  const hipStream_t s = f.s;
  const dev::State &st = f.st;
  int8_t *chan = static_cast<int8_t *>(w.chan), *msg = static_cast<int8_t *>(w.msg);
  int16_t *post = static_cast<int16_t *>(w.post);
  const uint32_t target_waves = opt_waves_ ? opt_waves_ : 128 * 1024;
  const dev::Graph g = f.graph(nullptr, nullptr);
  const dev::I8Opts o{impl_.rule == Rule::Aminstar, impl_.jones, impl_.hardlimit, impl_.deg1clip};
  // Minsumi8*: check nodes without LDS or scratch (kernels_i8_minsum.hip.h); a = 16 and b = 0 are the plain rule
  const bool minsum = impl_.rule == Rule::Minsum;
  const dev::I8MinsumOpts mo{impl_.hardlimit, impl_.correction == Correction::Normalized ? impl_.correction_int : 16,
                             impl_.correction == Correction::Offset ? impl_.correction_int : 0};

  if (int rc = f.begin(dev::ingest_i8_kernel<float>, dev::ingest_i8_kernel<double>, chan, post, dev::ingest_i8_kernel<int8_t>)) return rc;
  const Tiling pack_t = make_tiling(G, tile, 128, n, 256, target_waves);
  auto pack = [&]() {
    dev::pack_hard_pair_kernel<int16_t><<<pack_t.blocks, pack_t.threads, 0, s>>>(post, w.hardbits, w.n_active, w.n_slots,
                                                                                n, tile, f.W, pack_t.sched.waves_per_chunk);
  };

  uint32_t threads = 256;
  size_t lds = 0;
  // rows beyond the LDS (more than 320 edges): the columns live in HBM, one region per wavefront of a small launch
  const bool i8_fits = minsum || (staged_block(2, max_row_weight_, 4, &threads, &lds) && lds + 32 <= 160 * 1024);
  if (minsum) {
    threads = 256;
    lds = 0;
  }
  if (!i8_fits) {
    threads = kScratchThreads;
    lds = 0;
    const size_t waves_bound = size_t(kScratchWaves) + size_t(G / 256) * (kScratchThreads / 64);
    if (int rc = ensure_row_scratch(w, waves_bound * 2 * max_row_weight_ * 64 * 4)) return rc;
  }
  uint32_t *const i8_scratch = w.row_scratch.get<uint32_t>();
  if (!minsum) lds += 32;  // the correction lookup table (kernels_i8.hip.h, i8_table_init)
  auto set_lds = [&](const void *k) {
    if (lds > 48 * 1024)
      (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
  };
  uint32_t *unsat[2] = {w.unsat0, w.unsat1};
  int zero_fill = 0;
  if (impl_.schedule == Schedule::Flooding) {
    const Tiling cn_t = make_tiling(G, tile, 256, m, threads, i8_fits ? target_waves : std::min(target_waves, kScratchWaves));
    const Tiling vn_t = make_tiling(G, tile, 256, n, 256, target_waves);
    if (!i8_fits && scratch_bytes_for(cn_t, max_row_weight_, 4) > w.row_scratch.capacity()) {
      fail("internal error: row scratch smaller than the check-node launch");
      return -3;
    }
    set_lds(reinterpret_cast<const void *>(dev::cn_i8_kernel<true>));
    set_lds(reinterpret_cast<const void *>(dev::cn_i8_kernel<false>));
    for (uint32_t it = 1; it <= max_iterations; it++) {
      if (it > 1 && f.poll.finished(it)) break;
      const bool first = it == 1;
      uint32_t *unsat_out = unsat[it & 1];
      const dev::State stp = f.ticked(it);
      timed_begin(kKernelCheck, s);
      with_bool(first, [&](auto FIRST) {
        constexpr bool F = decltype(FIRST)::value;
        if (minsum)
          dev::cn_i8_minsum_kernel<F><<<cn_t.blocks, cn_t.threads, 0, s>>>(g, cn_t.sched, stp, mo, chan, post, msg, unsat_out);
        else if (!i8_fits)
          dev::cn_i8_kernel<F, true><<<cn_t.blocks, cn_t.threads, 0, s>>>(g, cn_t.sched, stp, o, chan, post, msg, unsat_out,
                                                                          max_row_weight_, i8_scratch);
        else
          dev::cn_i8_kernel<F><<<cn_t.blocks, cn_t.threads, lds, s>>>(g, cn_t.sched, stp, o, chan, post, msg, unsat_out,
                                                                      max_row_weight_);
      });
      timed_end(kKernelCheck, s);
      timed_begin(kKernelVar, s);
      dev::vn_i8_kernel<<<vn_t.blocks, vn_t.threads, 0, s>>>(g, vn_t.sched, st, o, chan, msg, post,
                                                             first ? nullptr : unsat_out, unsat[(it + 1) & 1],
                                                             static_cast<int32_t>(it) - 1);
      timed_end(kKernelVar, s);
    }
    if (max_iterations > 0) {
      pack();
      uint32_t *u = unsat[(max_iterations + 1) & 1];
      f.syndrome_of(w.hardbits, u);
      f.latch(u, static_cast<int32_t>(max_iterations));
    } else {
      zero_fill = 1;
    }
  } else {
    const uint32_t n_levels = level_ptr_.empty() ? 0 : static_cast<uint32_t>(level_ptr_.size() - 1);
    const dev::State st0 = st;
    set_lds(reinterpret_cast<const void *>(dev::hl_i8_kernel<true>));
    set_lds(reinterpret_cast<const void *>(dev::hl_i8_kernel<false>));
    const bool serial = n_levels > opt_serial_levels_;
    const uint32_t n_launch = serial ? std::min<uint32_t>(n_levels, 1) : n_levels;
    for (uint32_t it = 1; it <= max_iterations; it++) {
      if (it > 1 && f.poll.finished(it)) break;
      const dev::State stp = f.ticked(it);
      for (uint32_t l = 0; l < n_launch; l++) {
        const dev::State &st = l == 0 ? stp : st0;
        const uint32_t r0 = serial ? 0 : level_ptr_[l], cnt = serial ? m : level_ptr_[l + 1] - level_ptr_[l];
        // per level: LDS columns as tall as this level's longest row; register-resident rows when short
        const uint32_t ldmax = std::max<uint32_t>(serial ? max_row_weight_ : level_maxdeg_[l], 1);
        uint32_t lthreads = threads;
        size_t llds = 0;
        bool lfits = staged_block(2, ldmax, 4, &lthreads, &llds);
        if (serial) {
          lthreads = 64;          // row-serial mode (see run_group): one wave per 256-codeword slice
          llds = size_t(2) * ldmax * 64 * 4;
        }
        llds += 32;
        lfits = lfits && llds <= 160 * 1024;
        if (!lfits) {
          lthreads = serial ? 64 : kScratchThreads;
          llds = 0;
        }
        const uint32_t lreg = !opt_hl_reg_ ? 0 : (ldmax <= 12 ? 12 : (ldmax <= 24 ? 24 : 0));
        const Tiling t = make_tiling(G, tile, 256, serial ? 1 : cnt, lthreads, lfits ? target_waves : std::min(target_waves, kScratchWaves));
        if (!minsum && !lfits && scratch_bytes_for(t, ldmax, 4) > w.row_scratch.capacity()) {
          fail("internal error: row scratch smaller than a level's launch");
          return -3;
        }
        // k(..., tail...): hl_i8_reg_kernel ends with dmax, hl_i8_kernel with dmax and its scratch
        auto launch = [&](auto k, auto... tail) {
          if (llds > 48 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      static_cast<int>(llds));
          k<<<t.blocks, t.threads, llds, s>>>(g, t.sched, st, o, d_level_rows_.get<uint32_t>() + r0, cnt, post, msg, tail...);
        };
        auto launch_minsum = [&](auto k) {
          const Tiling mt = make_tiling(G, tile, 256, serial ? 1 : cnt, serial ? 64 : 256, target_waves);
          k<<<mt.blocks, mt.threads, 0, s>>>(g, mt.sched, st, mo, d_level_rows_.get<uint32_t>() + r0, cnt, post, msg);
        };
        timed_begin(kKernelLayer, s);
        with_bool(it == 1, [&](auto FIRST) {
          constexpr bool F = decltype(FIRST)::value;
          if (minsum) {
            if (lreg == 12)
              launch_minsum(dev::hl_i8_minsum_kernel<12, F>);
            else if (lreg == 24)
              launch_minsum(dev::hl_i8_minsum_kernel<24, F>);
            else
              launch_minsum(dev::hl_i8_minsum_kernel<0, F>);
          } else if (lreg == 12)
            launch(dev::hl_i8_reg_kernel<12, F>, ldmax);
          else if (lreg == 24)
            launch(dev::hl_i8_reg_kernel<24, F>, ldmax);
          else if (!lfits)
            launch(dev::hl_i8_kernel<F, true>, ldmax, i8_scratch);
          else
            launch(dev::hl_i8_kernel<F>, ldmax, nullptr);
        });
        timed_end(kKernelLayer, s);
      }
      pack();
      f.syndrome_of(w.hardbits, w.unsat0);
      f.latch(w.unsat0, static_cast<int32_t>(it));
    }
  }
  f.emit(post, nullptr, zero_fill, 0);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // namespace ldpc
