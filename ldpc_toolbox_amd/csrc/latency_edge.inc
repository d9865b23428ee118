// The lane-per-edge small-batch kernel (latency_edge.hip.h), every rule; *_kernel_corr is instantiated with kRuleMinsumCorr.
// Included TWICE by latency_edge.hip.h, inside namespace ldpc::dev: with LDPC_MINSUM_CORR 0 it is the kernel as it was before the
// normalized / offset min-sum forms existed, token for token (its code object is unchanged); with LDPC_MINSUM_CORR 1 the
// same kernel named *_kernel_corr, with one more argument (MinsumCorr<T> mc) and the correction of kernels_common.hip.h.
// LDPC_MS_KERNEL(x): x_kernel / x_kernel_corr; LDPC_MS_PARAM(T): nothing / `, MinsumCorr<T> mc`; LDPC_MS_ARG: nothing /
// `, mc`; LDPC_MS_TARG: nothing / `, true` (the CORR template argument of the phase functions).  No include guard, on purpose.

template <int RULE, typename T, typename SrcT, bool LAYERED>
__global__ __launch_bounds__(1024) void LDPC_MS_KERNEL(latency_edge)(EdgeLatTables g, EdgeLatState slots, LatencySync *sync,
                                                            const SrcT *__restrict__ llrs, uint32_t input_len, uint32_t batch,
                                                            uint32_t max_iterations, uint8_t *__restrict__ bits,
                                                            uint32_t out_len, int32_t *__restrict__ iterations,
                                                            SrcT *__restrict__ posterior, uint32_t *error_word,
                                                            uint32_t bundle, I8Opts o LDPC_MS_PARAM(T)) {
  constexpr bool I8 = RULE == kRuleEdgeI8;
  static_assert(I8 == std::is_integral<T>::value, "the 8-bit rules compute in int32_t words");
  __shared__ uint32_t s_slot, s_count, s_rank, s_nx;
  const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u;  // HW_REG_XCC_ID[3:0]
  if (threadIdx.x == 0) {
    s_slot = __hip_atomic_fetch_add(&sync->arrived[xcc], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&sync->total, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // census: every workgroup of the grid is resident and has reported (the grid is sized to fit)
    bool dead = false;
    lat_spin_until(&sync->total, gridDim.x, error_word, &dead);
    uint32_t nx = 0, rank = 0;
    for (uint32_t x = 0; x < 8; x++) {
      const uint32_t a = lat_atomic_load(&sync->arrived[x]);
      if (a != 0) {
        if (x < xcc) rank++;
        nx++;
      }
    }
    s_count = lat_atomic_load(&sync->arrived[xcc]);
    s_rank = rank;
    s_nx = nx;
  }
  __syncthreads();
  const uint32_t count = s_count, nthreads = count * blockDim.x, t0 = s_slot * blockDim.x + threadIdx.x;
  const uint32_t nwaves = lat_uniform(nthreads >> 6), w0 = lat_uniform(t0 >> 6), lane = threadIdx.x & 63u;
  LatEpoch epoch;
  uint64_t (*const bar)[16] = sync->barrier[xcc];
  const uint32_t my_slot = s_slot;
  const uint32_t n = g.n, n_lanes = g.n_chunks * 64;
  const TablePtr level_chunk = table_ptr(g.level_chunk);
  uint32_t *const flags = slots.flags + s_rank * 2 * kEdgeBundle;  // [2][kEdgeBundle]: number of the last vote that saw an odd row
  uint32_t vote_no = 0;
  // state of codeword j of the bundle
  auto soft_of = [&](uint32_t j) { return reinterpret_cast<T *>(slots.base + (size_t(s_rank) * kEdgeBundle + j) * slots.slot_bytes); };
  auto msg_of = [&](uint32_t j) { return reinterpret_cast<T *>(reinterpret_cast<char *>(soft_of(j)) + slots.off_msg); };
  auto chan_of = [&](uint32_t j) { return reinterpret_cast<T *>(reinterpret_cast<char *>(soft_of(j)) + slots.off_chan); };
  auto raw_of = [&](uint32_t j) { return reinterpret_cast<uint8_t *>(soft_of(j)) + slots.off_rawhard; };

  // bundles of `bundle` consecutive codewords; the XCDs that have workgroups share them round-robin
  for (uint32_t cw0 = s_rank * bundle; cw0 < batch; cw0 += s_nx * bundle) {
    const uint32_t kb = min(bundle, batch - cw0);

    // barrier + which codewords of `candidates` had an odd row somewhere (oddmask: this thread's view, bit j)
    auto vote = [&](uint32_t oddmask, uint32_t candidates) -> uint32_t {
      if (kb == 1) return xcd_barrier(bar, count, my_slot, &epoch, error_word, oddmask & 1u) ? 1u : 0u;
      vote_no += 1;
      uint32_t *const f = flags + (vote_no & 1u) * kEdgeBundle;
      for (uint32_t j = 0; j < kb; j++)
        if (__builtin_amdgcn_ballot_w64(((oddmask >> j) & 1u) != 0) != 0 && lane == 0) f[j] = vote_no;  // same value from all
      xcd_barrier(bar, count, my_slot, &epoch, error_word);
      uint32_t m = 0;
      for (uint32_t j = 0; j < kb; j++)
        if (((candidates >> j) & 1u) && lat_atomic_load(f + j) == vote_no) m |= 1u << j;
      return m;
    };

    // ingest: depuncture (puncturing.rs:83-101), quantise (arithmetic.rs:194-196), raw hard decisions for the
    // pre-check; messages = +0.0: the first iteration's `x - 0.0` (and `out - 0.0`) is the reference's initial state
    for (uint32_t idx = t0; idx < kb * n; idx += nthreads) {
      const uint32_t j = idx / n, v = idx - j * n;
      const SrcT *src = llrs + size_t(cw0 + j) * input_len;
      SrcT raw;
      if (g.src_block) {
        const int32_t sb = g.src_block[v / g.block_size];
        raw = sb < 0 ? SrcT(0.0) : src[size_t(sb) * g.block_size + v % g.block_size];
      } else {
        raw = src[v];
      }
      const T quantized = edge_quantize<T, SrcT>(raw);
      soft_of(j)[v] = quantized;
      if (!LAYERED) chan_of(j)[v] = quantized;
      raw_of(j)[v] = raw <= SrcT(0.0) ? 1 : 0;
    }
    for (uint32_t idx = t0; idx < kb * n_lanes; idx += nthreads) {
      const uint32_t j = idx / n_lanes;
      msg_of(j)[idx - j * n_lanes] = T(0.0);
    }
    xcd_barrier(bar, count, my_slot, &epoch, error_word);

    // syndrome of hard decisions over every row of the codewords in `which`: the raw input (pre-check: flooding.rs:57-64,
    // horizontal_layered.rs:55-62) or the soft values (flooding.rs:69-79 at the last iteration, horizontal_layered.rs:66-78)
    auto odd_rows = [&](bool raw, uint32_t which) -> uint32_t {
      uint32_t oddmask = 0;
      for (uint32_t t = w0; t < g.n_chunks * kb; t += nwaves) {
        const uint32_t j = t / g.n_chunks, c = t - j * g.n_chunks;
        if (!((which >> j) & 1u)) continue;  // wave-uniform
        const uint32_t k = c * 64 + lane, var = g.lane_var[k], info = g.lane_info[k];
        const bool on = var != kNoLane;
        bool bit = false;
        if (on) bit = raw ? lat_load(raw_of(j) + var) != 0 : lat_ld(soft_of(j) + var) <= T(0.0);
        if (chunk_has_odd_row(bit, lane, info & 0xFFu, on ? ((info >> 8) & 0xFFu) : 0u)) oddmask |= 1u << j;
      }
      return oddmask;
    };

    int32_t result[kEdgeBundle];  // iterations on success, -1 while running / failed
#pragma unroll
    for (uint32_t j = 0; j < kEdgeBundle; j++) result[j] = -1;
    const uint32_t all = (1u << kb) - 1u;
    uint32_t live = vote(odd_rows(true, all), all);  // a codeword whose raw input has no odd row is done: 0 iterations
#pragma unroll
    for (uint32_t j = 0; j < kEdgeBundle; j++)
      if (j < kb && !((live >> j) & 1u)) result[j] = 0;

    if constexpr (LAYERED) {
      // One codeword: a wavefront's first chunk of a level is the same in every iteration; its table entries and its
      // R values (which only this lane ever writes) are requested one level ahead, before the barrier, so that a
      // level's critical path is the Qv gather, the rule, the stores and the barrier.
      uint32_t p_var = kNoLane, p_info = 0;
      T p_r = T(0.0);
      T *const msg0 = msg_of(0);
      auto prefetch = [&](uint32_t l) {
        const uint32_t c = level_chunk[l] + w0;
        p_var = kNoLane;
        p_info = 0;
        if (c < level_chunk[l + 1]) {
          const uint32_t k = c * 64 + lane;
          p_var = g.lane_var[k];
          p_info = g.lane_info[k];
          p_r = lat_ld(msg0 + k);  // (a padding lane's slot exists too: no dependence on the table entry)
        }
      };
      // (with a single level "one level ahead" would read this level's R before it is written)
      const bool ahead = kb == 1 && g.n_levels > 1;
      if (live && max_iterations > 0 && ahead) prefetch(0);
      for (uint32_t it = 1; live != 0 && it <= max_iterations; it++) {
        for (uint32_t l = 0; l < g.n_levels; l++) {
          const uint32_t lc0 = level_chunk[l], nch = level_chunk[l + 1] - lc0;
          const uint32_t next_level = l + 1 == g.n_levels ? 0 : l + 1;
          if (w0 >= nch && ahead) prefetch(next_level);
          for (uint32_t t = w0; t < nch * kb; t += nwaves) {
            const uint32_t j = t / nch, c = lc0 + (t - j * nch);
            if (!((live >> j) & 1u)) continue;  // wave-uniform
            T *__restrict__ soft = soft_of(j);
            T *__restrict__ msg = msg_of(j);
            const uint32_t k = c * 64 + lane;
            const bool pre = ahead && t == w0;
            uint32_t var, info;
            T r;
            if (pre) {
              var = p_var;
              info = p_info;
              r = p_r;
            } else {
              var = g.lane_var[k];
              info = g.lane_info[k];
              r = lat_ld(msg + k);
            }
            const bool on = var != kNoLane;
            const uint32_t i = info & 0xFFu, d = on ? ((info >> 8) & 0xFFu) : 0u;
            const uint32_t dmax = lat_uniform(info >> 16);  // largest degree in the chunk (every lane carries it)
            T q = T(0.0);
            if (on) q = lat_ld(soft + var);
            if (pre) prefetch(next_level);  // in flight behind the gather, consumed after the barrier
            const T x = edge_v2c(q, r);
            T out;
            if constexpr (I8) out = rule_edge_i8(x, lane - i, i, d, dmax, o);
            else out = rule_edge<RULE, T>(x, lane - i, i, d, dmax LDPC_MS_ARG);
            if (on) {
              // Phi / Aminstar: Qv = x + out (arithmetic.rs:284-291, 1052-1065); the others: Qv += out - R (:423-424, 570-573;
              // 8-bit: :798, 1244-1254, x being the clipped copy of Qv - R)
              soft[var] = (RULE == kRulePhi || RULE == kRuleAminstar) ? (x + out) : (q + (out - r));
              msg[k] = out;
            }
          }
          xcd_barrier(bar, count, my_slot, &epoch, error_word);
        }
        const uint32_t still = vote(odd_rows(false, live), live);
#pragma unroll
        for (uint32_t j = 0; j < kEdgeBundle; j++)
          if (j < kb && ((live >> j) & 1u) && !((still >> j) & 1u)) result[j] = static_cast<int32_t>(it);
        live = still;
      }
    } else {
      // flooding: iteration `it` = check nodes from (L, c2v) of the previous one, with the parity of hard(L) over every
      // row fused in (it is the syndrome of iteration it - 1; iteration 1's is the pre-check above), then variable nodes
      uint32_t it = 1;
      for (; live != 0 && it <= max_iterations; it++) {
        uint32_t oddmask = it == 1 ? live : 0u;
        for (uint32_t t = w0; t < g.n_chunks * kb; t += nwaves) {
          const uint32_t j = t / g.n_chunks, c = t - j * g.n_chunks;
          if (!((live >> j) & 1u)) continue;  // wave-uniform
          T *__restrict__ msg = msg_of(j);
          const uint32_t k = c * 64 + lane, var = g.lane_var[k], info = g.lane_info[k];
          const bool on = var != kNoLane;
          const uint32_t i = info & 0xFFu, d = on ? ((info >> 8) & 0xFFu) : 0u;
          const uint32_t dmax = lat_uniform(info >> 16);
          T l = T(0.0), mo = T(0.0);
          if (on) {
            l = lat_ld(soft_of(j) + var);
            mo = lat_ld(msg + k);
          }
          if (chunk_has_odd_row(on && l <= T(0.0), lane, i, d)) oddmask |= 1u << j;
          const T x = edge_v2c(l, mo);  // v2c = L - c2v (arithmetic.rs:152)
          T out;
          if constexpr (I8) out = rule_edge_i8(x, lane - i, i, d, dmax, o);
          else out = rule_edge<RULE, T>(x, lane - i, i, d, dmax LDPC_MS_ARG);
          if (on) msg[k] = out;
        }
        // (the messages just written are this iteration's; a codeword whose previous posterior turns out to be a
        // codeword simply does not use them)
        const uint32_t still = vote(oddmask, live);
#pragma unroll
        for (uint32_t j = 0; j < kEdgeBundle; j++)
          if (j < kb && ((live >> j) & 1u) && !((still >> j) & 1u)) result[j] = static_cast<int32_t>(it) - 1;
        live = still;
        if (live == 0) break;
        for (uint32_t idx = t0; idx < kb * n; idx += nthreads) {
          const uint32_t j = idx / n, v = idx - j * n;
          if (!((live >> j) & 1u)) continue;
          const T *__restrict__ msg = msg_of(j);
          const uint32_t e0 = g.var_ptr[v], e1 = g.var_ptr[v + 1];
          if constexpr (I8) {
            // arithmetic.rs:622-654: degree-one clipping of the input (:826-842), Jones clipping of the sum (:806-810)
            int llr = lat_ld(chan_of(j) + v);
            if (o.deg1clip && e1 - e0 == 1) llr = llr <= -116 ? -116 : (llr >= 116 ? 116 : llr);
            for (uint32_t e = e0; e < e1; e++) llr += lat_ld(msg + g.var_lane[e]);
            soft_of(j)[v] = o.jones ? i8_clip(llr) : llr;
          } else {
            T sum = -T(0.0);  // Rust's float Sum identity (arithmetic.rs:146)
            for (uint32_t e = e0; e < e1; e++) sum = sum + lat_ld(msg + g.var_lane[e]);
            soft_of(j)[v] = lat_ld(chan_of(j) + v) + sum;
          }
        }
        xcd_barrier(bar, count, my_slot, &epoch, error_word);
      }
      // the syndrome of the last posterior (flooding.rs:69-79 at iteration == max_iterations)
      if (live != 0 && max_iterations > 0) {
        const uint32_t still = vote(odd_rows(false, live), live);
#pragma unroll
        for (uint32_t j = 0; j < kEdgeBundle; j++)
          if (j < kb && ((live >> j) & 1u) && !((still >> j) & 1u)) result[j] = static_cast<int32_t>(max_iterations);
        live = still;
      }
    }

    // emit: converged at 0 -> the raw input's hard decisions; flooding with max_iterations = 0 and not a codeword ->
    // the reference's never-written output_llrs (all ones, 0.0; flooding.rs:27-28, 82-85); else hard(soft)
#pragma unroll
    for (uint32_t j = 0; j < kEdgeBundle; j++) {
      if (j < kb) {
        const int32_t res = result[j];
        const bool zero_fill = !LAYERED && res < 0 && max_iterations == 0;
        const T *__restrict__ soft = soft_of(j);
        const uint8_t *__restrict__ rawhard = raw_of(j);
        for (uint32_t v = t0; v < n; v += nthreads) {
          T val = lat_ld(soft + v);
          uint8_t bit = res == 0 ? static_cast<uint8_t>(lat_load(rawhard + v)) : (val <= T(0.0) ? 1 : 0);
          if (zero_fill) {
            val = T(0.0);
            bit = 1;
          }
          if (v < out_len) bits[size_t(cw0 + j) * out_len + v] = bit;
          // (8-bit: the soft output is the 8-bit LLR clip(llr), arithmetic.rs:651, 713-715)
          if constexpr (I8) {
            if (posterior) posterior[size_t(cw0 + j) * n + v] = static_cast<SrcT>(i8_clip(val));
          } else {
            if (posterior) posterior[size_t(cw0 + j) * n + v] = static_cast<SrcT>(val);
          }
        }
        if (t0 == 0 && iterations) iterations[cw0 + j] = res;
      }
    }
    xcd_barrier(bar, count, my_slot, &epoch, error_word);  // the slots' arrays are reused by this XCD's next bundle
  }
}
