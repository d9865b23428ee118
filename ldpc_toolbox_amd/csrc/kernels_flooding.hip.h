// Flooding schedule: min-sum check nodes (per-edge messages, L-free variant, ROW RECORDS -- the headline kernel), the
// LDS-staged check nodes of the other rules, the variable-node kernel.  Part of kernels.hip.h (include that).
#pragma once
namespace ldpc {
namespace dev {



// ---------------------------------------------------------------------------------------
// Flooding min-sum check nodes with ROW RECORDS (default for Minsum f32/f64 when the rows fit the record's
// sign word).  A min-sum check row sends only two magnitudes: every c2v of the row is +-min1, except the one
// on the argmin slot, +-min2 (arithmetic.rs:487-521 without the correction: SURVEY.md Appendix A.6).  So the
// row's d messages ARE the record {min1, min2, flip bits, argmin} -- three words (four when d > 26 in f32):
//   c2v(slot) = (slot == argmin ? min2 : min1) with the sign bit  flip[slot] = total sign parity ^ (x_slot < 0),
// bit for bit the value the per-edge kernels store.  This kernel therefore
//   * reads its own previous messages as ONE record instead of d words (DVB-S2 1/2: 3 instead of 7),
//   * for an edge whose variable is L-free (degree <= 2, see cn_minsum_lfree_kernel) rebuilds the variable's
//     other message from the PEER row's record (Graph::edge_peer = peer row | peer slot).  A wavefront walks
//     runs of `run` consecutive rows: in DVB-S2's staircase the peers are rows c-1 and c+1, whose records the
//     same wavefront loads as its own one step earlier / later (cache hits, not HBM traffic),
//   * writes the new record, and per-edge messages ONLY for the edges of the variables the variable-node
//     kernel still walks (degree >= 3): 5 of 7 words for DVB-S2 1/2.
// Records are double-buffered (a row reads its neighbours' previous records while they write their new ones);
// the per-edge messages no longer are (nobody but vn_kernel reads them).  Per row of DVB-S2 1/2 the launch
// moves 3 + 5 + 1 + 3 + 5 + 1 = 18 words where cn_minsum_lfree_kernel moves 22-24.
//   rec_in / rec_out  [M * RECW][tile]  words of T's size: row c occupies rows c*RECW .. c*RECW + RECW-1
// ---------------------------------------------------------------------------------------
template <typename T>
struct RecWord {
  typedef uint32_t type;
  static constexpr int kArgShift = 26;  // RECW == 3: argmin above the flip bits (rows of at most 26 edges)
};
template <>
struct RecWord<double> {
  typedef uint64_t type;
  static constexpr int kArgShift = 58;
};
// edge_peer[e], an edge whose variable the variable-node kernel walks: kPeerKeep | position of its message in `msg`
// (the variable-major order that kernel reads); an edge of an L-free variable: writer << 30 | peer row << 6 | peer
// slot -- where the variable's OTHER message lives (row field kPeerSingle: there is none, degree 1)
enum : uint32_t { kPeerKeep = 0x80000000u, kPeerPosMask = 0x7FFFFFFFu, kPeerWriter = 0x40000000u, kPeerRowMask = 0xFFFFFFu,
                  kPeerSingle = 0xFFFFFFu };

// gfx950 store-data hazard the compiler does not know (found in round 5; tools/mb/store_hazard_repro.hip reproduces it
// stand-alone, profiles/r05_store_hazard.txt has the run): a MUBUF store of more than 64 bits reads its data registers
// AFTER issue.  With a literal soffset a vector instruction that rewrites one of them needs 2 wait states behind the store
// (LLVM's GCNHazardRecognizer pads those); with the soffset in an SGPR -- the form every [row][tile] access here takes -- it
// still needs ONE, but the ISA manuals exempt that form and the hazard recogniser follows them (createsVALUHazard:
// "this hazard only exists if the instruction is not using a register in the soffset field"), so nothing is inserted:
// `buffer_store_dwordx4 v[0:3], v58, s[56:59], s0 offen` followed directly by `v_and_b32 v2, 63, v53` stored the new v2 in
// lanes 12-15 of every 16 in about one store of 200 -- round 4's "element 2 of lanes 12-15 differs from run to run".
// The pad is an instruction that USES the data registers: they stay live up to it, so whatever rewrites them is issued
// behind it -- at least one wait state behind the store -- wherever the scheduler moves things.  The build checks the
// result in the code object itself (tools/mb/store_hazard_scan.py, `make lint`, tests/test_isa_lint.py).
typedef uint32_t store_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_data_pad(const store_u32x4 &data) { asm volatile("s_nop 0" ::"v"(data)); }

// [row][tile] accesses of a whole Pack through a buffer descriptor: SGPR row offset, one constant VGPR lane offset
template <typename T, int VEC, bool NT>
__device__ __forceinline__ Pack<T, VEC> buf_load(const RowBuf &b, uint32_t lane_off, uint32_t row_off) {
  constexpr int kBytes = sizeof(T) * VEC;
  static_assert(kBytes == 4 || kBytes == 8 || kBytes == 16, "pack size");
  if constexpr (kBytes == 4)
    return __builtin_bit_cast(Pack<T, VEC>, __builtin_amdgcn_raw_buffer_load_b32(b.r, lane_off, row_off, NT ? 2 : 0));
  else if constexpr (kBytes == 8)
    return __builtin_bit_cast(Pack<T, VEC>, __builtin_amdgcn_raw_buffer_load_b64(b.r, lane_off, row_off, NT ? 2 : 0));
  else
    return __builtin_bit_cast(Pack<T, VEC>, __builtin_amdgcn_raw_buffer_load_b128(b.r, lane_off, row_off, NT ? 2 : 0));
}
template <typename T, int VEC, bool NT>
__device__ __forceinline__ void buf_store(const RowBuf &b, uint32_t lane_off, uint32_t row_off, const Pack<T, VEC> &x) {
  constexpr int kBytes = sizeof(T) * VEC;
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  if constexpr (kBytes == 4)
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, x), b.r, lane_off, row_off, NT ? 2 : 0);
  else if constexpr (kBytes == 8)
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, x), b.r, lane_off, row_off, NT ? 2 : 0);
  else {
    const u32x4 data = __builtin_bit_cast(u32x4, x);
    __builtin_amdgcn_raw_buffer_store_b128(data, b.r, lane_off, row_off, NT ? 2 : 0);
    store_data_pad(data);
  }
}

template <typename T, int VEC, int RECW>
struct RowRec {
  typedef typename RecWord<T>::type W;
  Pack<T, VEC> min1, min2;
  Pack<W, VEC> flip, arg;  // RECW == 3: `flip` is the whole third word, `arg` unused
  // row_off: byte offset of the record's first row in the wavefront's slice; row_bytes: bytes between rows
  __device__ __forceinline__ void load(const RowBuf &b, uint32_t lane_off, uint32_t row_off, uint32_t row_bytes) {
    min1 = buf_load<T, VEC, false>(b, lane_off, row_off);
    min2 = buf_load<T, VEC, false>(b, lane_off, row_off + row_bytes);
    flip = __builtin_bit_cast(Pack<W, VEC>, buf_load<T, VEC, false>(b, lane_off, row_off + 2 * row_bytes));
    if constexpr (RECW == 4) arg = __builtin_bit_cast(Pack<W, VEC>, buf_load<T, VEC, false>(b, lane_off, row_off + 3 * row_bytes));
  }
  template <bool NT>
  __device__ __forceinline__ void store(const RowBuf &b, uint32_t lane_off, uint32_t row_off, uint32_t row_bytes) const {
    buf_store<T, VEC, NT>(b, lane_off, row_off, min1);
    buf_store<T, VEC, NT>(b, lane_off, row_off + row_bytes, min2);
    buf_store<T, VEC, NT>(b, lane_off, row_off + 2 * row_bytes, __builtin_bit_cast(Pack<T, VEC>, flip));
    if constexpr (RECW == 4) buf_store<T, VEC, NT>(b, lane_off, row_off + 3 * row_bytes, __builtin_bit_cast(Pack<T, VEC>, arg));
  }
  // the message this row sends on `slot` (wave-uniform) to codeword k of the lane.  The magnitudes are never
  // negative (nor NaN: a NaN input never wins a `<`), so OR-ing the sign bit in is exactly the negation.
  __device__ __forceinline__ T value(uint32_t slot, int k) const {
    const W a = RECW == 4 ? arg.v[k] : (flip.v[k] >> RecWord<T>::kArgShift);
    const T mag = (a == W(slot)) ? min2.v[k] : min1.v[k];
    const W sign = (flip.v[k] >> slot) << (8 * sizeof(W) - 1);
    return __builtin_bit_cast(T, __builtin_bit_cast(W, mag) | sign);
  }
};


// Posterior of the L-free variables from the row records: L = chan + (m_a + m_b), the messages read out of the
// records of the variable's one or two rows (free_rs: row << 6 | slot per edge, kAuxNone = no such edge).
//   event_iteration < 0: after the last iteration (no later check-node pass rebuilds it), for the codewords
//                        still running; frozen codewords are skipped;
//   event_iteration >= 0: after the variable-node pass that latched the FIRST converged codewords of a slice
//                        (State::slice_state == 1) at that iteration count: for exactly those codewords, whose
//                        L-free posteriors the check-node kernel had not been storing.
template <typename T, int VEC, int RECW>
__global__ __launch_bounds__(256) void vn_free_rec_kernel(Graph g, Sched sc, State st, const uint32_t *__restrict__ free_rs_,
                                                          const T *__restrict__ chan, const T *__restrict__ rec,
                                                          T *__restrict__ post, int32_t event_iteration) {
  if (event_iteration < 0 && *st.n_active == 0) return;
  const TablePtr free_var = table_ptr(g.list_var), free_rs = table_ptr(free_rs_);
  const uint32_t lane = threadIdx.x & 63u, tile = sc.tile;
  const uint32_t wave = uniform((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  uint32_t chunk, i0;
  wave_slot(sc, wave, &chunk, &i0);
  if (chunk >= sc.nchunks) return;
  const uint32_t b0 = chunk * (64 * VEC);
  if (b0 >= *st.n_slots) return;
  if (event_iteration >= 0 && st.slice_state[chunk] != 1) return;
  const size_t off = size_t(b0) + lane * VEC;
  const size_t G = tile;
  chan += tile_base(b0, g.n_cols, sc) + lane * VEC;
  post += tile_base(b0, g.n_cols, sc) + lane * VEC;
  const uint32_t row_bytes = tile * uint32_t(sizeof(T)), lane_off = lane * uint32_t(VEC * sizeof(T));
  const RowBuf b_rec = row_buf(rec + tile_base(b0, g.n_rows * RECW, sc),
                               uint64_t(g.n_rows) * RECW * row_bytes - in_tile_of(b0, sc) * uint32_t(sizeof(T)));
  bool live[VEC];  // the codewords this pass writes
  bool any_live = false;
#pragma unroll
  for (int k = 0; k < VEC; k++) {
    live[k] = event_iteration < 0 ? st.done[off + k] == 0 : (st.done[off + k] != 0 && st.iters[off + k] == event_iteration);
    any_live = any_live || live[k];
  }
  if (__builtin_amdgcn_ballot_w64(any_live) == 0) return;
  for (uint32_t i = i0; i < g.n_list; i += sc.waves_per_chunk) {
    const uint32_t v = free_var[i], a = free_rs[2 * i], b = free_rs[2 * i + 1];
    const Pack<T, VEC> ch = load_pack<T, VEC>(chan + size_t(v) * G);
    RowRec<T, VEC, RECW> ra, rb;
    if (a != kAuxNone) ra.load(b_rec, lane_off, (a >> 6) * RECW * row_bytes, row_bytes);
    if (b != kAuxNone) rb.load(b_rec, lane_off, (b >> 6) * RECW * row_bytes, row_bytes);
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      T sum = -T(0.0);  // arithmetic.rs:146: the slot-ordered sum, from Rust's float Sum identity
      if (a != kAuxNone) sum = sum + ra.value(a & 63u, k);
      if (b != kAuxNone) sum = sum + rb.value(b & 63u, k);
      if (live[k]) post[size_t(v) * G + k] = ch.v[k] + sum;
    }
  }
}


// ---------------------------------------------------------------------------------------
// Flooding, variable nodes (all float rules share arithmetic.rs:140-156):
//   S = sum of the incoming check messages in cols[v] order, folded from -0.0 (Rust's
//   float Sum identity), L = channel + S.  Only L is written; the consumer recomputes
//   L - m.  Also latches codewords whose previous posterior had a zero syndrome
//   (flooding.rs:69-79): they stop being rewritten from this pass on.
// Index fetches of the next variable overlap the current variable's loads (as in the
// check-node kernel).
// ---------------------------------------------------------------------------------------
// EVW != 0 (round 5; flooding min-sum with row records and deferred L-free stores): the launch also does what a separate
// vn_free_rec_kernel launch did after it in every iteration -- the L-free posteriors of the FIRST codewords of a slice to
// converge, rebuilt from the records of the iteration being latched (State::slice_state) -- spread over the launch's own
// waves instead of a small grid of its own: one launch and one dispatch gap fewer per iteration (4.4 + 5.7 us of 2050), and
// the one pass that does find work runs at the full grid's width.  Which codewords are "newly converged" must not depend on
// what the bookkeeping wave of the slice has already written in this same launch: see `fresh` below.
template <typename T>
struct VnEvent {
  const uint32_t *free_var, *free_rs;  // the L-free variables and, per variable, its two (row << 6 | slot) words
  const T *rec;                        // records of the iteration being latched
  uint32_t n_free;
};
template <typename T, int VEC, int U, bool NT, bool LIST, int EVW = 0>
__global__ __launch_bounds__(256) void vn_kernel(
    Graph g, Sched sc, State st, const T *__restrict__ chan, const T *__restrict__ msg,
    T *__restrict__ post, const uint32_t *__restrict__ unsat_in, uint32_t *__restrict__ unsat_clear,
    int32_t latch_iteration, VnEvent<T> ev = VnEvent<T>{nullptr, nullptr, nullptr, 0}) {
  uint32_t *__restrict__ n_active = st.n_active;
  // A finished group's launches return at once.  With EVW the count can also reach zero INSIDE this launch -- the
  // bookkeeping waves below subtract the codewords they latch -- and a wave that starts after the last subtraction must
  // still take its share of the rebuild of those codewords' L-free posteriors: it goes on to the EVW block (where a group
  // that had finished BEFORE the launch has no `fresh` codeword and costs a few loads) and returns behind it.
  const bool idle = *n_active == 0;
  if (EVW == 0 && idle) return;
  const TablePtr col_ptr = table_ptr(LIST ? g.list_ptr : g.col_ptr);
  const TablePtr col_edge = table_ptr(LIST ? g.list_edge : g.col_edge);
  uint32_t *__restrict__ done = st.done;
  int32_t *__restrict__ iters = st.iters;
  const uint32_t n_cols = LIST ? g.n_list : g.n_cols;  // items to process
  const uint32_t waves_per_chunk = sc.waves_per_chunk, tile = sc.tile;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uniform((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  uint32_t chunk, v_first;
  wave_slot(sc, wave, &chunk, &v_first);
  if (chunk >= sc.nchunks) return;
  const uint32_t b0 = chunk * (64 * VEC);
  if (b0 >= *st.n_slots) return;
  if constexpr (EVW != 0) {
    if (idle && (ev.rec == nullptr || unsat_in == nullptr || st.slice_state == nullptr || st.slice_state[chunk] == 2u)) return;
  }
  const size_t off = size_t(b0) + lane * VEC;
  const size_t G = tile;
  chan += tile_base(b0, g.n_cols, sc) + lane * VEC;
  post += tile_base(b0, g.n_cols, sc) + lane * VEC;
  msg += tile_base(b0, g.n_edges, sc) + lane * VEC;
  bool skip[VEC];
  bool any_live = false, any_new = false;
#pragma unroll
  for (int k = 0; k < VEC; k++) {
    const bool was_done = done[off + k] != 0;
    const bool converged = !was_done && unsat_in != nullptr && unsat_in[off + k] == 0;
    // continuous batching: the codeword's own iteration count; one that has used all of its iterations without
    // converging fails here and keeps its last posterior (flooding.rs:82-85)
    int32_t own_iterations = latch_iteration;
    bool expired = false;
    if (st.it0 != nullptr) {
      own_iterations = latch_iteration - static_cast<int32_t>(st.it0[off + k]);
      expired = !was_done && !converged && own_iterations >= static_cast<int32_t>(st.max_it);
    }
    skip[k] = was_done || converged || expired;
    any_live = any_live || !skip[k];
    if (v_first == 0 && !idle) {
      // exactly one wave per slice does the per-codeword bookkeeping (idle: the count is zero only once EVERY bookkeeping
      // wave has subtracted its codewords, this one included -- or the group had finished before the launch)
      if (converged || expired) {
        done[off + k] = 1u;
        iters[off + k] = converged ? own_iterations : -1;
        atomicSub(n_active, 1u);
        any_new = true;
      }
      unsat_clear[off + k] = 0u;
    }
  }
  if constexpr (EVW != 0) {
    // The slice's first convergences (slice_state 0, or 1 when the bookkeeping wave has already marked it in this launch;
    // 2 = the check-node kernel has been storing the L-free posteriors all along): every wave of the slice takes its share
    // of the L-free variables.  `fresh`: converging in THIS launch -- from what this launch does not change (the syndrome
    // flag the last check-node pass left, the slot's codeword) and from `iters`, which is -1 before the launch and
    // latch_iteration once the bookkeeping wave has been here: both mean "this launch" (an earlier convergence carries its
    // own, smaller count; an empty slot has no codeword).
    if (ev.rec != nullptr && unsat_in != nullptr && st.slice_state != nullptr && st.slice_state[chunk] != 2u) {
      bool fresh[VEC];
      bool any_fresh = false;
#pragma unroll
      for (int k = 0; k < VEC; k++) {
        const int32_t was = iters[off + k];
        fresh[k] = unsat_in[off + k] == 0 && st.slot_cw[off + k] != kNoCodeword && (was < 0 || was == latch_iteration);
        any_fresh = any_fresh || fresh[k];
      }
      if (__builtin_amdgcn_ballot_w64(any_fresh) != 0) {
        const TablePtr free_var = table_ptr(ev.free_var), free_rs = table_ptr(ev.free_rs);
        const uint32_t row_bytes = tile * uint32_t(sizeof(T)), lane_off = lane * uint32_t(VEC * sizeof(T));
        const RowBuf b_rec = row_buf(ev.rec + tile_base(b0, g.n_rows * EVW, sc),
                                     uint64_t(g.n_rows) * EVW * row_bytes - in_tile_of(b0, sc) * uint32_t(sizeof(T)));
        for (uint32_t i = v_first; i < ev.n_free; i += waves_per_chunk) {
          const uint32_t fv = free_var[i], a = free_rs[2 * i], b = free_rs[2 * i + 1];
          const Pack<T, VEC> ch = load_pack<T, VEC>(chan + size_t(fv) * G);
          RowRec<T, VEC, EVW> ra, rb;
          if (a != kAuxNone) ra.load(b_rec, lane_off, (a >> 6) * EVW * row_bytes, row_bytes);
          if (b != kAuxNone) rb.load(b_rec, lane_off, (b >> 6) * EVW * row_bytes, row_bytes);
#pragma unroll
          for (int k = 0; k < VEC; k++) {
            T sum = -T(0.0);  // arithmetic.rs:146: the slot-ordered sum, from Rust's float Sum identity
            if (a != kAuxNone) sum = sum + ra.value(a & 63u, k);
            if (b != kAuxNone) sum = sum + rb.value(b & 63u, k);
            if (fresh[k]) post[size_t(fv) * G + k] = ch.v[k] + sum;
          }
        }
      }
    }
  }
  if (idle) return;
  if (v_first == 0 && st.slice_state != nullptr && __builtin_amdgcn_ballot_w64(any_new) != 0 && lane == 0 &&
      st.slice_state[chunk] == 0)
    st.slice_state[chunk] = 1;  // the first convergences of this slice: see State::slice_state
  if (__builtin_amdgcn_ballot_w64(any_live) == 0) return;
  bool all = true;
#pragma unroll
  for (int k = 0; k < VEC; k++) all = all && !skip[k];

  const uint32_t last_slot = g.n_edges ? g.n_edges - 1 : 0;
  uint32_t v = v_first, s0 = 0, s1 = 0, ed[U], var = v_first;
  if (v < n_cols) {
    s0 = col_ptr[v];
    s1 = col_ptr[v + 1];
    if (LIST) var = table_ptr(g.list_var)[v];
  }
#pragma unroll
  for (int u = 0; u < U; u++) ed[u] = col_edge[min(s0 + u, last_slot)];

  while (v < n_cols) {
    T sum[VEC];
#pragma unroll
    for (int k = 0; k < VEC; k++) sum[k] = -T(0.0);
    // (a nontemporal load here -- nobody else reads these channel rows in the list variant -- takes 7 us off this kernel
    // and puts 14 us on the check-node kernel that follows: profiles/r04_vn_kernel.txt)
    const Pack<T, VEC> ch = load_pack<T, VEC>(chan + size_t(var) * G);
    const uint32_t vn = v + waves_per_chunk;
    uint32_t ns0 = 0, ns1 = 0, nvar = vn;
    if (vn < n_cols) {
      ns0 = col_ptr[vn];
      ns1 = col_ptr[vn + 1];
      if (LIST) nvar = table_ptr(g.list_var)[vn];
    }
    uint32_t ned[U];
    for (uint32_t j0 = s0; j0 < s1; j0 += U) {
      Pack<T, VEC> mv[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (j0 + u < s1) {  // wave-uniform
          const uint32_t e = (j0 == s0) ? ed[u] : col_edge[j0 + u];
          mv[u] = load_msg<T, VEC, NT>(msg + size_t(e) * G);
        }
      }
      if (j0 == s0) {
#pragma unroll
        for (int u = 0; u < U; u++) ned[u] = col_edge[min(ns0 + u, last_slot)];
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (j0 + u < s1) {
#pragma unroll
          for (int k = 0; k < VEC; k++) sum[k] = sum[k] + mv[u].v[k];
        }
      }
    }
    if (s0 == s1) {
#pragma unroll
      for (int u = 0; u < U; u++) ned[u] = col_edge[min(ns0 + u, last_slot)];
    }
    Pack<T, VEC> o;
#pragma unroll
    for (int k = 0; k < VEC; k++) o.v[k] = ch.v[k] + sum[k];
    T *dst = post + size_t(var) * G;
    if (all) {
      store_pack<T, VEC>(dst, o);
    } else {
      // (reading the frozen codewords' values back and storing whole packs instead was measured in round 5: no gain at
      // +2 dB, 0.5 % on the fixed-work pass for the extra branch -- profiles/r05_p2_timeline.txt)
#pragma unroll
      for (int k = 0; k < VEC; k++)
        if (!skip[k]) dst[k] = o.v[k];
    }
    v = vn;
    var = nvar;
    s0 = ns0;
    s1 = ns1;
#pragma unroll
    for (int u = 0; u < U; u++) ed[u] = ned[u];
  }
}

// The check-node kernels min-sum can take (cn_minsum, cn_minsum_lfree, cn_minsum_rec, cn_staged): kernels_flooding_minsum.inc, once plain and once as the normalized / offset
// min-sum forms (*_kernel_corr) -- see the head of that file
#define LDPC_MINSUM_CORR 0
#define LDPC_MS_KERNEL(x) x##_kernel
#define LDPC_MS_PARAM(T)
#define LDPC_MS_ARG
#include "kernels_flooding_minsum.inc"
#undef LDPC_MINSUM_CORR
#undef LDPC_MS_KERNEL
#undef LDPC_MS_PARAM
#undef LDPC_MS_ARG
#define LDPC_MINSUM_CORR 1
#define LDPC_MS_KERNEL(x) x##_kernel_corr
#define LDPC_MS_PARAM(T) , MinsumCorr<T> mc = MinsumCorr<T>{}
#define LDPC_MS_ARG , mc
#include "kernels_flooding_minsum.inc"
#undef LDPC_MINSUM_CORR
#undef LDPC_MS_KERNEL
#undef LDPC_MS_PARAM
#undef LDPC_MS_ARG

}  // namespace dev
}  // namespace ldpc
