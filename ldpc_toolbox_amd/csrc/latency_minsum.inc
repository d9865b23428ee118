// The row-lane small-batch kernel of flooding Minsumf32 (latency.hip.h).
// Included TWICE by latency.hip.h, inside namespace ldpc::dev: with LDPC_MINSUM_CORR 0 it is the kernel as it was before the
// normalized / offset min-sum forms existed, token for token (its code object is unchanged); with LDPC_MINSUM_CORR 1 the
// same kernel named *_kernel_corr, with one more argument (MinsumCorr<T> mc) and the correction of kernels_common.hip.h.
// LDPC_MS_KERNEL(x): x_kernel / x_kernel_corr; LDPC_MS_PARAM(T): nothing / `, MinsumCorr<T> mc`; LDPC_MS_ARG: nothing /
// `, mc`; LDPC_MS_TARG: nothing / `, true` (the CORR template argument of the phase functions).  No include guard, on purpose.

template <typename SrcT>
__global__ __launch_bounds__(1024) void LDPC_MS_KERNEL(latency_minsum)(LatencyTables g, LatencyState slots,
                                                              LatencySync *sync, const SrcT *__restrict__ llrs,
                                                              uint32_t input_len, uint32_t batch, uint32_t max_iterations,
                                                              uint8_t *__restrict__ bits, uint32_t out_len,
                                                              int32_t *__restrict__ iterations,
                                                              SrcT *__restrict__ posterior, uint32_t *error_word LDPC_MS_PARAM(float)) {
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
  const uint32_t n = g.n;
  // this wavefront's first row slice and first two variable slices: indices into registers, once per call
  LatRowCache rc{};
  LatVarCache vc[2]{};
  if (w0 < g.n_rslices) {
    rc.e0 = lat_uniform(g.rslice_ptr[w0]);
    rc.width = lat_uniform((g.rslice_ptr[w0 + 1] - rc.e0) >> 6);
    rc.deg = g.rdeg[w0 * 64 + lane];
#pragma unroll
    for (uint32_t u = 0; u < 8; u++) rc.col4[u] = g.col[rc.e0 + lane + u * 64] * 4;
  }
#pragma unroll
  for (uint32_t i = 0; i < 2; i++) {
    const uint32_t sl = w0 + i * nwaves;
    if (sl < g.n_vslices) {
      vc[i].k0 = lat_uniform(g.vslice_ptr[sl]);
      vc[i].width = lat_uniform((g.vslice_ptr[sl + 1] - vc[i].k0) >> 6);
      vc[i].deg = g.vdeg[sl * 64 + lane];
#pragma unroll
      for (uint32_t u = 0; u < 8; u++) vc[i].edge4[u] = g.vedge[vc[i].k0 + lane + u * 64] * 4;
    }
  }

  // the XCDs that have workgroups share the codewords round-robin
  for (uint32_t cw = s_rank; cw < batch; cw += s_nx) {
    char *const slot = slots.base + size_t(s_rank) * slots.slot_bytes;
    float *__restrict__ chan = reinterpret_cast<float *>(slot);
    float *__restrict__ post = reinterpret_cast<float *>(slot + slots.off_post);
    float *__restrict__ msg = reinterpret_cast<float *>(slot + slots.off_msg);
    uint8_t *__restrict__ rawhard = reinterpret_cast<uint8_t *>(slot + slots.off_rawhard);
    const SrcT *src = llrs + size_t(cw) * input_len;
    const uint32_t soft_bytes = static_cast<uint32_t>(slots.off_post), msg_bytes = static_cast<uint32_t>(slots.off_rawhard - slots.off_msg);
    const LatBuf b_msg = lat_buf(msg, msg_bytes);
    const LatArrays a_first{lat_buf(chan, soft_bytes), b_msg, lat_buf(rawhard, static_cast<uint32_t>(slots.slot_bytes - slots.off_rawhard))};
    const LatArrays a_iter{lat_buf(post, soft_bytes), b_msg, a_first.rawhard};

    // ingest: depuncture (puncturing.rs:83-101), quantise (`x as f32`), raw hard decisions for the pre-check
    // (in source order: `llrs` may be the caller's pinned host buffer, read over the bus -- coalesced reads there,
    // the scatter lands in device memory)
    for (uint32_t v = t0; v < n; v += nthreads) {
      const uint32_t t = g.perm[v];
      SrcT raw;
      if (g.src_block) {
        const int32_t sb = g.src_block[v / g.block_size];
        raw = sb < 0 ? SrcT(0.0) : src[size_t(sb) * g.block_size + v % g.block_size];
      } else {
        raw = src[v];
      }
      chan[t] = static_cast<float>(raw);
      rawhard[t] = raw <= SrcT(0.0) ? 1 : 0;
    }
    xcd_barrier(bar, count, my_slot, &epoch, error_word);
#pragma unroll
    for (uint32_t i = 0; i < 2; i++) {
      const uint32_t sl = w0 + i * nwaves;
      if (sl < g.n_vslices) vc[i].chan = lat_load(chan + min(sl * 64 + lane, n - 1));
    }

    int32_t result = -1;  // iterations on success
    for (uint32_t it = 1; it <= max_iterations + 1; it++) {
      const bool first = it == 1, last = it == max_iterations + 1;
      // check nodes: messages of iteration `it` (not when `last`) and the parity of the previous posterior's
      // hard decisions over every row (the raw input's when `first`)
      uint32_t odd;
      if (first)
        odd = last ? latency_cn_phase<true, false LDPC_MS_TARG>(g, a_first, w0, nwaves, lane, rc LDPC_MS_ARG)
                   : latency_cn_phase<true, true LDPC_MS_TARG>(g, a_first, w0, nwaves, lane, rc LDPC_MS_ARG);
      else
        odd = last ? latency_cn_phase<false, false LDPC_MS_TARG>(g, a_iter, w0, nwaves, lane, rc LDPC_MS_ARG)
                   : latency_cn_phase<false, true LDPC_MS_TARG>(g, a_iter, w0, nwaves, lane, rc LDPC_MS_ARG);
      const bool converged = !xcd_barrier(bar, count, my_slot, &epoch, error_word, odd);  // no row anywhere is odd
      if (converged) {
        result = static_cast<int32_t>(it) - 1;  // flooding.rs:57-64 (0) / 69-79
        break;
      }
      if (last) break;
      latency_vn_phase(g, chan, b_msg, post, w0, nwaves, lane, vc);
      xcd_barrier(bar, count, my_slot, &epoch, error_word);
    }

    // emit: converged at 0 -> the raw input's hard decisions and the (quantised) input; max_iterations = 0 and
    // not a codeword -> the reference's never-written output_llrs (all ones, 0.0); else hard(posterior)
    const bool zero_fill = result < 0 && max_iterations == 0;
    for (uint32_t v = t0; v < n; v += nthreads) {
      const uint32_t t = g.perm[v];
      float val;
      uint8_t bit;
      if (result == 0) {
        val = lat_load(chan + t);
        bit = lat_load(rawhard + t);
      } else if (zero_fill) {
        val = 0.0f;
        bit = 1;
      } else {
        val = lat_load(post + t);
        bit = val <= 0.0f ? 1 : 0;
      }
      if (v < out_len) bits[size_t(cw) * out_len + v] = bit;
      if (posterior) posterior[size_t(cw) * n + v] = static_cast<SrcT>(val);
    }
    if (t0 == 0 && iterations) iterations[cw] = result;
    xcd_barrier(bar, count, my_slot, &epoch, error_word);  // the slot's arrays are reused by this XCD's next codeword
  }
}
