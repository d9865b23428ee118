// Flooding schedule: the check-node kernels min-sum can take (streaming, L-free, row records, LDS-staged).
// Included TWICE by kernels_flooding.hip.h, inside namespace ldpc::dev: once with LDPC_MINSUM_CORR 0 -- the kernels of plain min-sum (and of
// the other rules), token for token what they were before the normalized / offset forms existed, so their code objects are
// unchanged -- and once with LDPC_MINSUM_CORR 1: the same kernels named *_kernel_corr, with one more argument
// (MinsumCorr<T> mc: alpha, beta) and the correction of kernels_common.hip.h (MinsumCorr) where a magnitude leaves the fold.
//   LDPC_MS_KERNEL(x)   x_kernel / x_kernel_corr
//   LDPC_MS_PARAM(T)    nothing / `, MinsumCorr<T> mc`   (last kernel parameter; defaulted, as it may follow a defaulted one)
//   LDPC_MS_ARG         nothing / `, mc`                 (last argument of rule_check_node / rule_edge / the phase functions)
// (x_kernel_corr, not x_corr_kernel: the two forms of a kernel share the stem that tools and tests select kernels by.)
// No include guard, on purpose.

// ---------------------------------------------------------------------------------------
// Flooding, min-sum check nodes: streaming kernel, state in registers.
//   L    [N][tile]   posterior of the previous iteration (channel LLRs when FIRST)
//   msg  [E][tile]   check->variable messages, rewritten in place
// v2c is never stored: x = L[v] - msg[e] is the same subtraction the reference's
// variable node performs (arithmetic.rs:152), evaluated here by the consumer.
// The parity of hard(L) over the row is the syndrome bit of the PREVIOUS iteration's
// posterior (flooding.rs:69-79), accumulated per codeword across this wave's rows.
// The graph indices of the NEXT row are fetched (scalar loads) while the current row's
// vector loads are in flight, so a wave's dependent chain per row is one memory latency.
// ---------------------------------------------------------------------------------------
template <typename T, int VEC, typename MASK, int U, bool FIRST, bool NT>
__global__ __launch_bounds__(256) void LDPC_MS_KERNEL(cn_minsum)(
    Graph g, Sched sc, State st, const T *__restrict__ L, T *__restrict__ msg,
    uint32_t *__restrict__ unsat_out LDPC_MS_PARAM(T)) {
  if (group_finished(st)) return;  // (publishes the progress word when the launch carries one: a paced host follows it)
  const TablePtr row_ptr = table_ptr(g.row_ptr);
  const TablePtr edge_col = table_ptr(g.edge_col);
  const uint32_t *__restrict__ done = st.done;
  const uint32_t n_rows = g.n_rows, waves_per_chunk = sc.waves_per_chunk;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uniform((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  uint32_t chunk, node0;
  wave_slot(sc, wave, &chunk, &node0);
  if (chunk >= sc.nchunks) return;
  const uint32_t b0 = chunk * (64 * VEC);
  if (b0 >= *st.n_slots) return;
  const size_t off = size_t(b0) + lane * VEC;  // codeword index (flag arrays)
  const size_t G = sc.tile;                       // row stride inside a tile
  L += tile_base(b0, g.n_cols, sc) + lane * VEC;
  msg += tile_base(b0, g.n_edges, sc) + lane * VEC;
  {
    bool all_done = true;
#pragma unroll
    for (int k = 0; k < VEC; k++) all_done = all_done && (done[off + k] != 0);
    if (__builtin_amdgcn_ballot_w64(!all_done) == 0) return;
  }
  uint32_t odd_acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; k++) odd_acc[k] = 0;

  // indices of the current row: edge range and the variables of its first U edges
  uint32_t c = node0, e0 = 0, e1 = 0, cols[U];
  if (c < n_rows) {
    e0 = row_ptr[c];
    e1 = row_ptr[c + 1];
  }
#pragma unroll
  for (int u = 0; u < U; u++) cols[u] = edge_col[min(e0 + u, g.n_edges - 1)];

  while (c < n_rows) {
    T min1[VEC], min2[VEC];
    uint32_t arg[VEC], par[VEC];
    MASK sgn[VEC];
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      min1[k] = Limits<T>::inf();
      min2[k] = Limits<T>::inf();
      arg[k] = 0;
      par[k] = 0;
      sgn[k] = 0;
    }
    // next row's edge range: issued now, consumed after this row's loads are in flight
    const uint32_t cn = c + waves_per_chunk;
    uint32_t ne0 = 0, ne1 = 0;
    if (cn < n_rows) {
      ne0 = row_ptr[cn];
      ne1 = row_ptr[cn + 1];
    }
    uint32_t ncols[U];
    for (uint32_t i0 = e0; i0 < e1; i0 += U) {
      Pack<T, VEC> lv[U], mv[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const uint32_t e = min(i0 + u, e1 - 1);
        // slots beyond the degree re-read slot 0 / the last edge (cache hits), masked below
        const uint32_t v = (i0 + u < e1) ? ((i0 == e0) ? cols[u] : edge_col[e]) : cols[0];
        lv[u] = load_pack<T, VEC>(L + size_t(v) * G);
        if (!FIRST) mv[u] = load_msg<T, VEC, NT>(msg + size_t(e) * G);
      }
      if (i0 == e0) {
#pragma unroll
        for (int u = 0; u < U; u++) ncols[u] = edge_col[min(ne0 + u, g.n_edges - 1)];
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (i0 + u < e1) {
          const uint32_t slot = i0 + u - e0;
#pragma unroll
          for (int k = 0; k < VEC; k++) {
            const T l = lv[u].v[k];
            const T x = FIRST ? l : (l - mv[u].v[k]);
            const T a = m_abs(x);
            if (x < T(0.0)) sgn[k] |= MASK(1) << slot;
            if (l <= T(0.0)) par[k] ^= 1u;
            if (a < min1[k]) {
              min2[k] = min1[k];
              min1[k] = a;
              arg[k] = slot;
            } else if (a < min2[k]) {
              min2[k] = a;
            }
          }
        }
      }
    }
    if (e0 == e1) {  // empty row: nothing loaded, still fetch the next row's variables
#pragma unroll
      for (int u = 0; u < U; u++) ncols[u] = edge_col[min(ne0 + u, g.n_edges - 1)];
    }
    uint32_t tot[VEC];
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      tot[k] = (sizeof(MASK) == 8 ? __popcll(sgn[k]) : __popc(uint32_t(sgn[k]))) & 1u;
      odd_acc[k] |= par[k];
    }
#if LDPC_MINSUM_CORR
    // once per row: every message of the row is one of these two magnitudes
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      min1[k] = minsum_corrected(min1[k], mc);
      min2[k] = minsum_corrected(min2[k], mc);
    }
#endif
    const uint32_t d = e1 - e0;
    for (uint32_t slot = 0; slot < d; slot++) {
      Pack<T, VEC> o;
#pragma unroll
      for (int k = 0; k < VEC; k++) {
        const uint32_t neg = uint32_t(sgn[k] >> slot) & 1u;
        const T mag = (arg[k] == slot) ? min2[k] : min1[k];
        o.v[k] = (tot[k] ^ neg) ? -mag : mag;
      }
      store_msg<T, VEC, NT>(msg + size_t(e0 + slot) * G, o);
    }
    c = cn;
    e0 = ne0;
    e1 = ne1;
#pragma unroll
    for (int u = 0; u < U; u++) cols[u] = ncols[u];
  }
  if (!FIRST) {
#pragma unroll
    for (int k = 0; k < VEC; k++)
      if (odd_acc[k]) unsat_out[off + k] = 1u;
  }
}

// ---------------------------------------------------------------------------------------
// Flooding min-sum check nodes with L-free variables (Graph::edge_aux): for an edge whose
// variable has degree <= 2 the kernel reads the channel LLR and the variable's other message
// and forms L = chan + (m_own + m_other) itself -- the two-term slot-ordered sum of
// arithmetic.rs:146 is commutative, so this is bit-identical -- then x = L - m_own.  The
// variable's first slot also stores L into `post` (kept for frozen codewords), so `post` is
// always the previous iteration's posterior, exactly as with the plain kernels.  Saves the
// variable-node kernel 4 row accesses per such variable (half of DVB-S2's variables).
// Because a check now reads a neighbour's message, messages are double-buffered: read from
// msg_in (previous iteration), write to msg.
// ---------------------------------------------------------------------------------------
template <typename T, int VEC, typename MASK, int U, bool FIRST, bool NT, bool NT_IN>
__global__ __launch_bounds__(256) void LDPC_MS_KERNEL(cn_minsum_lfree)(
    Graph g, Sched sc, State st, const T *__restrict__ chan, T *__restrict__ post,
    const T *__restrict__ msg_in, T *__restrict__ msg, uint32_t *__restrict__ unsat_out LDPC_MS_PARAM(T)) {
  if (group_finished(st)) return;  // (publishes the progress word when the launch carries one: a paced host follows it)
  const TablePtr row_ptr = table_ptr(g.row_ptr);
  const TablePtr edge_col = table_ptr(g.edge_col);
  const TablePtr edge_aux = table_ptr(g.edge_aux);
  const uint32_t *__restrict__ done = st.done;
  const uint32_t n_rows = g.n_rows, waves_per_chunk = sc.waves_per_chunk;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uniform((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  uint32_t chunk, node0;
  wave_slot(sc, wave, &chunk, &node0);
  if (chunk >= sc.nchunks) return;
  const uint32_t b0 = chunk * (64 * VEC);
  if (b0 >= *st.n_slots) return;
  const size_t off = size_t(b0) + lane * VEC;
  const size_t G = sc.tile;
  chan += tile_base(b0, g.n_cols, sc) + lane * VEC;
  post += tile_base(b0, g.n_cols, sc) + lane * VEC;
  msg += tile_base(b0, g.n_edges, sc) + lane * VEC;
  msg_in += tile_base(b0, g.n_edges, sc) + lane * VEC;
  bool live[VEC];
  bool any_live = false, all_live = true;
#pragma unroll
  for (int k = 0; k < VEC; k++) {
    live[k] = done[off + k] == 0;
    any_live = any_live || live[k];
    all_live = all_live && live[k];
  }
  if (__builtin_amdgcn_ballot_w64(any_live) == 0) return;
  uint32_t odd_acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; k++) odd_acc[k] = 0;

  for (uint32_t c = node0; c < n_rows; c += waves_per_chunk) {
    const uint32_t e0 = row_ptr[c], e1 = row_ptr[c + 1];
    if (e0 == e1) continue;
    T min1[VEC], min2[VEC];
    uint32_t arg[VEC], par[VEC];
    MASK sgn[VEC];
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      min1[k] = Limits<T>::inf();
      min2[k] = Limits<T>::inf();
      arg[k] = 0;
      par[k] = 0;
      sgn[k] = 0;
    }
    for (uint32_t i0 = e0; i0 < e1; i0 += U) {
      Pack<T, VEC> lv[U], mv[U], mo[U];
      uint32_t aux[U], var[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        aux[u] = kAuxNone;
        var[u] = 0;
        if (i0 + u < e1) {  // wave-uniform
          const uint32_t e = i0 + u;
          var[u] = edge_col[e];
          aux[u] = edge_aux[e];
          if (aux[u] == kAuxNone) {
            lv[u] = load_pack<T, VEC>(post + size_t(var[u]) * G);
          } else {
            lv[u] = load_pack<T, VEC>(chan + size_t(var[u]) * G);
            if (!FIRST && (aux[u] & kAuxMask) != kAuxSingle)
              mo[u] = load_pack<T, VEC>(msg_in + size_t(aux[u] & kAuxMask) * G);  // re-read by the neighbour: keep cached
          }
          if (!FIRST) mv[u] = load_msg<T, VEC, NT_IN>(msg_in + size_t(e) * G);
        }
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (i0 + u < e1) {
          const uint32_t slot = i0 + u - e0;
          const bool lfree = aux[u] != kAuxNone;
          const bool single = (aux[u] & kAuxMask) == kAuxSingle;
          Pack<T, VEC> lnew;
#pragma unroll
          for (int k = 0; k < VEC; k++) {
            T l = lv[u].v[k];
            if (lfree && !FIRST) {
              const T ssum = single ? mv[u].v[k] : (mv[u].v[k] + mo[u].v[k]);
              l = l + ssum;  // chan + (m_a + m_b)
            }
            lnew.v[k] = l;
            const T x = FIRST ? l : (l - mv[u].v[k]);
            const T a = m_abs(x);
            if (x < T(0.0)) sgn[k] |= MASK(1) << slot;
            if (l <= T(0.0)) par[k] ^= 1u;
            if (a < min1[k]) {
              min2[k] = min1[k];
              min1[k] = a;
              arg[k] = slot;
            } else if (a < min2[k]) {
              min2[k] = a;
            }
          }
          if (lfree && !FIRST && (aux[u] & kAuxWriter)) {
            T *dst = post + size_t(var[u]) * G;
            if (all_live) {
              store_pack<T, VEC>(dst, lnew);
            } else {
#pragma unroll
              for (int k = 0; k < VEC; k++)
                if (live[k]) dst[k] = lnew.v[k];
            }
          }
        }
      }
    }
    uint32_t tot[VEC];
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      tot[k] = (sizeof(MASK) == 8 ? __popcll(sgn[k]) : __popc(uint32_t(sgn[k]))) & 1u;
      odd_acc[k] |= par[k];
    }
#if LDPC_MINSUM_CORR
    // once per row: every message of the row is one of these two magnitudes
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      min1[k] = minsum_corrected(min1[k], mc);
      min2[k] = minsum_corrected(min2[k], mc);
    }
#endif
    const uint32_t d = e1 - e0;
    for (uint32_t slot = 0; slot < d; slot++) {
      Pack<T, VEC> o;
#pragma unroll
      for (int k = 0; k < VEC; k++) {
        const uint32_t neg = uint32_t(sgn[k] >> slot) & 1u;
        const T mag = (arg[k] == slot) ? min2[k] : min1[k];
        o.v[k] = (tot[k] ^ neg) ? -mag : mag;
      }
      store_msg<T, VEC, NT>(msg + size_t(e0 + slot) * G, o);
    }
  }
  if (!FIRST) {
#pragma unroll
    for (int k = 0; k < VEC; k++)
      if (odd_acc[k]) unsat_out[off + k] = 1u;
  }
}

// U: edges of a row whose data loads are issued together with the next record's (rows longer than U take
// further rounds); the graph tables must be padded by U entries (the index fetch of a row reads U of them).
// Wavefronts walk runs of `run` consecutive rows, even runs upwards and odd runs downwards: the two records at
// a run boundary are then wanted by both neighbours at the same moment (their first steps, or their last),
// so one of the two fetches is a cache hit.
// STREAM (continuous batching): a lane whose codeword starts with this launch (State::it0 == the launch's
// iteration - 1) has no previous messages: its own and its peers' read as +0.0 -- `Qv - 0.0`, the reference's initial
// state -- whatever the record arrays hold from the slot's previous codeword.
// LONG: some row has more than U edges (further rounds of U loads; compiled out otherwise: the extra code costs the
// short-row case 2 % in registers and scheduling).
template <typename T, int VEC, int RECW, int U, bool FIRST, bool NT, bool STREAM = false, bool LONG = true>
__global__ __launch_bounds__(256) void LDPC_MS_KERNEL(cn_minsum_rec)(
    Graph g, Sched sc, State st, const T *__restrict__ chan, T *__restrict__ post, const T *__restrict__ rec_in,
    T *__restrict__ rec_out, T *__restrict__ msg, uint32_t *__restrict__ unsat_out, uint32_t run LDPC_MS_PARAM(T)) {
  typedef typename RecWord<T>::type W;
  if (group_finished(st)) return;  // (publishes the progress word when the launch carries one: a paced host follows it)
  const TablePtr row_ptr = table_ptr(g.row_ptr);
  const TablePtr edge_col = table_ptr(g.edge_col);
  const TablePtr edge_peer = table_ptr(g.edge_peer);
  const uint32_t *__restrict__ done = st.done;
  const uint32_t n_rows = g.n_rows, waves_per_chunk = sc.waves_per_chunk, tile = sc.tile;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uniform((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  uint32_t chunk, node0;
  wave_slot(sc, wave, &chunk, &node0);
  if (chunk >= sc.nchunks) return;
  const uint32_t b0 = chunk * (64 * VEC);
  if (b0 >= *st.n_slots) return;
  const size_t off = size_t(b0) + lane * VEC;
  bool live[VEC];
  bool any_live = false, all_live = true;
#pragma unroll
  for (int k = 0; k < VEC; k++) {
    live[k] = done[off + k] == 0;
    any_live = any_live || live[k];
    all_live = all_live && live[k];
  }
  if (__builtin_amdgcn_ballot_w64(any_live) == 0) return;
  all_live = __builtin_amdgcn_ballot_w64(!all_live) == 0;  // wave-uniform
  bool fresh[VEC];
#pragma unroll
  for (int k = 0; k < VEC; k++) fresh[k] = STREAM && st.it0[off + k] + 1u == st.tick;
  // Posterior of the L-free variables: stored (by the variable's first slot) only in slices where a codeword has
  // converged before -- as long as none has, nothing reads it (State::slice_state; the first convergences of a
  // slice are served by vn_free_rec_kernel's event mode)
  uint32_t write_post = 1;
  if (st.slice_state != nullptr) {
    write_post = st.slice_state[chunk];
    if (write_post == 1 && node0 == 0 && lane == 0) st.slice_state[chunk] = 2;
  }
  if (FIRST) write_post = 0;
  // the wavefront's slice of every [row][tile] array behind a buffer descriptor: a row access is an SGPR offset
  const uint32_t row_bytes = tile * uint32_t(sizeof(T)), lane_off = lane * uint32_t(VEC * sizeof(T));
  const uint32_t in_tile = in_tile_of(b0, sc) * uint32_t(sizeof(T));
  const RowBuf b_chan = row_buf(chan + tile_base(b0, g.n_cols, sc), uint64_t(g.n_cols) * row_bytes - in_tile);
  const RowBuf b_post = row_buf(post + tile_base(b0, g.n_cols, sc), uint64_t(g.n_cols) * row_bytes - in_tile);
  const RowBuf b_msg = row_buf(msg + tile_base(b0, g.n_edges, sc), uint64_t(g.n_edges) * row_bytes - in_tile);
  const RowBuf b_rin = row_buf(rec_in + tile_base(b0, g.n_rows * RECW, sc), uint64_t(g.n_rows) * RECW * row_bytes - in_tile);
  const RowBuf b_rout = row_buf(rec_out + tile_base(b0, g.n_rows * RECW, sc), uint64_t(g.n_rows) * RECW * row_bytes - in_tile);
  const uint32_t rec_bytes = RECW * row_bytes;
  uint64_t odd_m[VEC];  // lane masks (SGPR pairs): codeword k of the lane has seen an odd row
#pragma unroll
  for (int k = 0; k < VEC; k++) odd_m[k] = 0;

  for (uint32_t r = node0; r * run < n_rows; r += waves_per_chunk) {
    const uint32_t lo = r * run, hi = min(lo + run, n_rows);
    const uint32_t dir = (r & 1u) ? 0xFFFFFFFFu : 1u;  // +1 / -1 (row numbers wrap: an invalid row is >= n_rows)
    uint32_t c = (r & 1u) ? hi - 1 : lo;
    // own = record of the current row, nxt = record of the row the walk reaches next (this row's peer now, `own`
    // one step later); carry = the message the PREVIOUS row of the walk sent to the variable it shares with this
    // one (it had that value in hand as its own message: the previous row's record need not be kept)
    RowRec<T, VEC, RECW> recA, recB;
    T carry[VEC];
#pragma unroll
    for (int k = 0; k < VEC; k++) carry[k] = T(0.0);
    uint32_t carry_slot = kAuxNone;  // slot of the previous row whose old message `carry` holds
    uint32_t e0 = row_ptr[c], e1 = row_ptr[c + 1], ne0 = 0, ne1 = 0;
    if (c + dir < n_rows) {
      ne0 = row_ptr[c + dir];
      ne1 = row_ptr[c + dir + 1];
    }
    uint32_t cols[U], peers[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      cols[u] = edge_col[e0 + u];
      peers[u] = edge_peer[e0 + u];
    }
    if (!FIRST) recA.load(b_rin, lane_off, c * rec_bytes, row_bytes);

    auto row_step = [&](RowRec<T, VEC, RECW> &own, RowRec<T, VEC, RECW> &nxt) {
      const uint32_t d = e1 - e0, cn = c + dir, cp = c - dir;
      if (!FIRST && cn < n_rows) nxt.load(b_rin, lane_off, cn * rec_bytes, row_bytes);
      Pack<T, VEC> lv[U];
#pragma unroll
      for (int u = 0; u < U; u++)
        if (uint32_t(u) < d)
          lv[u] = buf_load<T, VEC, false>((peers[u] & kPeerKeep) ? b_post : b_chan, lane_off,
                                          cols[u] * row_bytes);
      // the next row's indices and the range of the row after it: scalar loads that complete while this row's
      // data is in flight
      uint32_t nne0 = 0, nne1 = 0, ncols[U], npeers[U];
      if (cn < n_rows && cn + dir < n_rows) {
        nne0 = row_ptr[cn + dir];
        nne1 = row_ptr[cn + dir + 1];
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        ncols[u] = edge_col[ne0 + u];
        npeers[u] = edge_peer[ne0 + u];
      }
      T min1[VEC], min2[VEC];
      uint32_t arg[VEC];
      W sgn[VEC];
      uint64_t par_m[VEC];
#pragma unroll
      for (int k = 0; k < VEC; k++) {
        min1[k] = Limits<T>::inf();
        min2[k] = Limits<T>::inf();
        arg[k] = 0;
        sgn[k] = 0;
        par_m[k] = 0;
      }
      uint32_t next_carry_slot = kAuxNone;
      T next_carry[VEC];
#pragma unroll
      for (int k = 0; k < VEC; k++) next_carry[k] = T(0.0);  // (read below whether or not an edge has set it)
      // one edge: slot, variable, peer word, the loaded soft value (posterior, or channel LLR for an L-free variable)
      auto edge = [&](uint32_t slot, uint32_t var, uint32_t peer, const Pack<T, VEC> &lvu) {
        const bool lfree = !(peer & kPeerKeep);
        const uint32_t prow = (peer >> 6) & kPeerRowMask, pslot = peer & 63u;
        const bool single = prow == kPeerSingle;
        // the variable's other message (wave-uniform choice of where it comes from)
        T m_other[VEC];
        if (lfree && !FIRST && !single) {
          if (prow == cn) {
#pragma unroll
            for (int k = 0; k < VEC; k++) m_other[k] = nxt.value(pslot, k);
          } else if (prow == cp && pslot == carry_slot) {
#pragma unroll
            for (int k = 0; k < VEC; k++) m_other[k] = carry[k];
          } else {
            RowRec<T, VEC, RECW> far;  // not a neighbour inside the run: fetch the peer's record
            far.load(b_rin, lane_off, prow * rec_bytes, row_bytes);
#pragma unroll
            for (int k = 0; k < VEC; k++) m_other[k] = far.value(pslot, k);
          }
          if constexpr (STREAM) {
#pragma unroll
            for (int k = 0; k < VEC; k++) m_other[k] = fresh[k] ? T(0.0) : m_other[k];
          }
        }
        Pack<T, VEC> lnew;
#pragma unroll
        for (int k = 0; k < VEC; k++) {
          T l = lvu.v[k];
          T m_own = T(0.0);
          if (!FIRST) {
            m_own = own.value(slot, k);
            if constexpr (STREAM) m_own = fresh[k] ? T(0.0) : m_own;
            if (lfree) l = l + (single ? m_own : (m_own + m_other[k]));  // chan + (m_a + m_b)
          }
          lnew.v[k] = l;
          if (lfree && !FIRST && prow == cn) next_carry[k] = m_own;
          const T x = FIRST ? l : (l - m_own);
          const T a = m_abs(x);
          if (x < T(0.0)) sgn[k] |= W(1) << slot;
          par_m[k] ^= __builtin_amdgcn_ballot_w64(l <= T(0.0));
          if (a < min1[k]) {
            min2[k] = min1[k];
            min1[k] = a;
            arg[k] = slot;
          } else if (a < min2[k]) {
            min2[k] = a;
          }
        }
        if (lfree && !FIRST && prow == cn) next_carry_slot = slot;
        if (lfree && write_post && (peer & kPeerWriter)) {
          if (all_live) {
            buf_store<T, VEC, false>(b_post, lane_off, var * row_bytes, lnew);
          } else {
#pragma unroll
            for (int k = 0; k < VEC; k++)
              if (live[k]) row_store<T, false>(b_post, lane_off + k * uint32_t(sizeof(T)), var * row_bytes, lnew.v[k]);
          }
        }
      };
#pragma unroll
      for (int u = 0; u < U; u++)
        if (uint32_t(u) < d) edge(u, cols[u], peers[u], lv[u]);
      if constexpr (LONG)
      for (uint32_t i0 = U; i0 < d; i0 += U) {  // rows longer than U: further rounds of U loads in flight
        uint32_t cv[U], pv[U];
        Pack<T, VEC> lw[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          cv[u] = edge_col[e0 + i0 + u];  // (the tables are padded: in bounds)
          pv[u] = edge_peer[e0 + i0 + u];
        }
#pragma unroll
        for (int u = 0; u < U; u++)
          if (i0 + u < d) lw[u] = buf_load<T, VEC, false>((pv[u] & kPeerKeep) ? b_post : b_chan, lane_off, cv[u] * row_bytes);
#pragma unroll
        for (int u = 0; u < U; u++)
          if (i0 + u < d) edge(i0 + u, cv[u], pv[u], lw[u]);
      }
      carry_slot = next_carry_slot;
#pragma unroll
      for (int k = 0; k < VEC; k++) carry[k] = next_carry[k];
      if (d != 0) {
        // the new record: flip[slot] = (parity of all signs) ^ (x_slot < 0)
        RowRec<T, VEC, RECW> out;
#pragma unroll
        for (int k = 0; k < VEC; k++) {
          const uint32_t tot = (sizeof(W) == 8 ? __popcll(sgn[k]) : __popc(uint32_t(sgn[k]))) & 1u;
          odd_m[k] |= par_m[k];
#if LDPC_MINSUM_CORR
          // the record holds the corrected pair, so every reader of the record (value()) sees corrected messages
          out.min1.v[k] = minsum_corrected(min1[k], mc);
          out.min2.v[k] = minsum_corrected(min2[k], mc);
#else
          out.min1.v[k] = min1[k];
          out.min2.v[k] = min2[k];
#endif
          const W fl = tot ? ~sgn[k] : sgn[k];
          if constexpr (RECW == 4) {
            out.flip.v[k] = fl;
            out.arg.v[k] = W(arg[k]);
          } else {
            out.flip.v[k] = (fl & ((W(1) << RecWord<T>::kArgShift) - 1)) | (W(arg[k]) << RecWord<T>::kArgShift);
          }
        }
        // (Round 4 kept this store behind an always-true `run != 0`: with it unconditional two variants returned results that
        // differed from run to run.  Round 5 found why -- the gfx950 store-data hazard described at store_data_pad above, a
        // `v_and_b32 v2, ...` issued right behind `buffer_store_dwordx4 v[0:3], ...` -- so the condition is gone: every 128-bit
        // buffer store carries its pad and the build lints the code object.)
        out.template store<NT>(b_rout, lane_off, c * rec_bytes, row_bytes);
        // per-edge messages for the variables the variable-node kernel walks, at the position it reads them from
        auto send = [&](uint32_t slot, uint32_t peer) {
          if (!(peer & kPeerKeep)) return;  // wave-uniform
          Pack<T, VEC> o;
#pragma unroll
          for (int k = 0; k < VEC; k++) o.v[k] = out.value(slot, k);
          buf_store<T, VEC, NT>(b_msg, lane_off, (peer & kPeerPosMask) * row_bytes, o);
        };
#pragma unroll
        for (int u = 0; u < U; u++)
          if (uint32_t(u) < d) send(u, peers[u]);
        if constexpr (LONG)
          for (uint32_t i = U; i < d; i++) send(i, edge_peer[e0 + i]);
      }
      c = cn;
      e0 = ne0;
      e1 = ne1;
      ne0 = nne0;
      ne1 = nne1;
#pragma unroll
      for (int u = 0; u < U; u++) {
        cols[u] = ncols[u];
        peers[u] = npeers[u];
      }
    };
    // two rows per round: the records alternate between recA and recB, no register copies
    for (uint32_t i = lo; i < hi; i += 2) {
      row_step(recA, recB);
      if (i + 1 < hi) row_step(recB, recA);
    }
  }
  if (!FIRST) {
#pragma unroll
    for (int k = 0; k < VEC; k++)
      if ((odd_m[k] >> lane) & 1ull) unsat_out[off + k] = 1u;
  }
}

// ---------------------------------------------------------------------------------------
// Flooding, any rule: the check row's d inputs are staged in two LDS columns per thread
// ([slot][thread], conflict-free); global loads and stores are issued U at a time.
// dynamic LDS: 2 * dmax * blockDim.x * sizeof(T)
// ---------------------------------------------------------------------------------------
// SCRATCH (round 5): rows too long for the CU's LDS (2 * dmax * 64 * sizeof(T) > 160 KB: more than 320 edges in f32, 160
// in f64 -- the reference takes any alist, /root/reference/src/sparse.rs:352-389) keep the two columns in a per-wavefront
// region of `scratch` in HBM, [2 * dmax][64] -- the same code, the same order of operations, global instead of LDS
// accesses.  Slow by design (nothing real has such rows); the launch is sized to a few thousand waves.
template <int RULE, typename T, bool FIRST, bool SCRATCH = false>
__global__ void LDPC_MS_KERNEL(cn_staged)(Graph g, Sched sc, State st, const T *__restrict__ L,
                                 T *__restrict__ msg, uint32_t *__restrict__ unsat_out, uint32_t dmax,
                                 T *__restrict__ scratch = nullptr LDPC_MS_PARAM(T)) {
  constexpr int U = 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (group_finished(st)) return;
  const TablePtr row_ptr = table_ptr(g.row_ptr);
  const TablePtr edge_col = table_ptr(g.edge_col);
  const uint32_t n_rows = g.n_rows, waves_per_chunk = sc.waves_per_chunk, tile = sc.tile;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uniform((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const uint32_t S = SCRATCH ? 64u : blockDim.x;
  T *A = SCRATCH ? scratch + size_t(wave) * 2u * dmax * 64u + lane : reinterpret_cast<T *>(smem) + threadIdx.x;
  T *B = A + size_t(dmax) * S;
  uint32_t chunk, node0;
  wave_slot(sc, wave, &chunk, &node0);
  if (chunk >= sc.nchunks) return;
  const uint32_t b0 = chunk * 64;
  if (b0 >= *st.n_slots) return;
  const size_t off = size_t(b0) + lane;
  const size_t G = tile;
  L += tile_base(b0, g.n_cols, sc) + lane;
  msg += tile_base(b0, g.n_edges, sc) + lane;
  if (__builtin_amdgcn_ballot_w64(st.done[off] == 0) == 0) return;
  uint32_t odd_acc = 0;
  for (uint32_t c = node0; c < n_rows; c += waves_per_chunk) {
    const uint32_t e0 = row_ptr[c], e1 = row_ptr[c + 1];
    const uint32_t d = e1 - e0;
    if (d == 0) continue;
    uint32_t par = 0;
    for (uint32_t i0 = 0; i0 < d; i0 += U) {
      T lv[U], mv[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (i0 + u < d) {
          const uint32_t v = edge_col[e0 + i0 + u];
          lv[u] = L[size_t(v) * G];
          if (!FIRST) mv[u] = load_msg<T, 1, true>(msg + size_t(e0 + i0 + u) * G).v[0];  // streamed once
        }
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (i0 + u < d) {
          A[(i0 + u) * S] = FIRST ? lv[u] : (lv[u] - mv[u]);
          if (lv[u] <= T(0.0)) par ^= 1u;
        }
      }
    }
    odd_acc |= par;
    const T *out = rule_check_node<RULE, T>(A, B, d, S LDPC_MS_ARG);
    for (uint32_t i0 = 0; i0 < d; i0 += U) {
#pragma unroll
      for (int u = 0; u < U; u++)
        if (i0 + u < d) {
          Pack<T, 1> ov;
          ov.v[0] = out[(i0 + u) * S];
          store_msg<T, 1, true>(msg + size_t(e0 + i0 + u) * G, ov);
        }
    }
  }
  if (!FIRST && odd_acc) unsat_out[off] = 1u;
}
