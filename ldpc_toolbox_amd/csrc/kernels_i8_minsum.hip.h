// HIP kernels for the 8-bit min-sum family, [HL]Minsumi8[Norm|Offset][Jones][PartialHardLimit][Deg1Clip][:value]
// (this build's addition; the integer definition is in DESIGN.md section 1).  The arithmetic is Minstarapproxi8's with the
// fold step reduced to min: edge i of a check row gets the magnitude m_i = min over the OTHER edges of |x_j|, corrected once
// -- (a * m + 8) >> 4 for Norm, max(m - b, 0) for Offset -- then the optional partial hard limit, then the sign (parity of
// x_j < 0 over the other edges).  A row therefore needs min1, min2, the first argmin and a sign parity per codeword: no table,
// no LDS, no O(d^2) fold.
//
// Layout, tiling, quantiser, variable nodes, emit and compaction are those of kernels_i8.hip.h: a lane owns four codewords
// (one packed word of i8 messages, four i16 posteriors), a wave a 256-codeword slice, and v2c is rebuilt as clip(post - msg).
#pragma once
#include "kernels_i8.hip.h"

namespace ldpc {
namespace dev {

struct I8MinsumOpts {
  int hardlimit;  // partial_hard_limit! on the corrected, signed message
  int a;          // Norm: 16 * alpha, 1..16 (16 = no normalisation)
  int b;          // Offset: 8 * beta, 0..127 (0 = no offset)
};

// min1 / min2 / first argmin of one codeword of a row, as keys (|x| << 16 | slot): equal magnitudes order by slot, so the
// smallest key is the FIRST minimum and the second smallest key carries min2 (equal to min1 on a tie).  k1 <= k2 always.
struct I8MinPair {
  uint32_t k1, k2;
};
__device__ __forceinline__ void i8_min_track(I8MinPair &p, uint32_t mag, uint32_t slot) {
  const uint32_t key = (mag << 16) | slot;
  p.k2 = min(p.k2, max(p.k1, key));
  p.k1 = min(p.k1, key);
}
// the correction and the hard limit of a magnitude 0..127: max(((a * m + 8) >> 4) - b, 0), then >= 100 -> 127
__device__ __forceinline__ uint32_t i8_minsum_correct(uint32_t m, I8MinsumOpts o) {
  const uint32_t n = (uint32_t(o.a) * m + 8u) >> 4;
  const uint32_t c = n > uint32_t(o.b) ? n - uint32_t(o.b) : 0u;
  return (o.hardlimit && c >= 100u) ? 127u : c;
}
// what a row sends: per codeword byte the corrected min1 (every edge but the argmin), min2 (the argmin) and the argmin slot
struct I8RowOut {
  uint32_t c1[4], c2[4], arg[4];
};
__device__ __forceinline__ I8RowOut i8_minsum_row(const I8MinPair *p, I8MinsumOpts o) {
  I8RowOut r;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    r.c1[k] = i8_minsum_correct(p[k].k1 >> 16, o);
    r.c2[k] = i8_minsum_correct(min(p[k].k2 >> 16, 127u), o);  // (a row of one edge has no min2: refused at construction)
    r.arg[k] = p[k].k1 & 0xFFFFu;
  }
  return r;
}
// the packed message word of slot i; s01: byte k is 1 where the message of codeword k is negative
__device__ __forceinline__ uint32_t i8_minsum_word(const I8RowOut &r, uint32_t i, uint32_t s01) {
  uint32_t mag = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) mag |= (r.arg[k] == i ? r.c2[k] : r.c1[k]) << (8 * k);
  return pk_negate_where(mag, s01);
}

// ---- flooding check nodes ------------------------------------------------------------------------
// One pass over the row's edges in bursts of U: x = clip(post - msg) (FIRST: the channel value), min1 / min2 / argmin, the sign
// parity and the row's syndrome parity per codeword byte.  Rows of at most 32 edges keep the signs of their inputs as one bit
// per slot and codeword (four mask registers) and the second pass only stores; longer rows re-read post and msg for the sign.
// No LDS, no scratch, rows of any length (the slot takes the key's low 16 bits: up to 65535 edges, far beyond any alist here).
template <bool FIRST>
__global__ __launch_bounds__(256) void cn_i8_minsum_kernel(Graph g, Sched sc, State st, I8MinsumOpts o,
                                                           const int8_t *__restrict__ chan, const int16_t *__restrict__ post,
                                                           int8_t *__restrict__ msg, uint32_t *__restrict__ unsat_out) {
  constexpr int U = 8;
  if (group_finished(st)) return;
  const TablePtr row_ptr = table_ptr(g.row_ptr), edge_col = table_ptr(g.edge_col);
  const uint32_t tile = sc.tile;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uniform((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  uint32_t chunk, node0;
  wave_slot(sc, wave, &chunk, &node0);
  if (chunk >= sc.nchunks) return;
  const uint32_t b0 = chunk * 256;
  if (b0 >= *st.n_slots) return;
  const size_t off = size_t(b0) + lane * 4;
  chan += tile_base(b0, g.n_cols, sc) + lane * 4;
  post += tile_base(b0, g.n_cols, sc) + lane * 4;
  msg += tile_base(b0, g.n_edges, sc) + lane * 4;
  {
    bool any_live = false;
#pragma unroll
    for (int k = 0; k < 4; k++) any_live = any_live || st.done[off + k] == 0;
    if (__builtin_amdgcn_ballot_w64(any_live) == 0) return;
  }
  uint32_t odd_acc = 0;  // bit k: codeword k of this lane saw an odd check
  for (uint32_t c = node0; c < g.n_rows; c += sc.waves_per_chunk) {
    const uint32_t e0 = row_ptr[c], e1 = row_ptr[c + 1];
    const uint32_t d = e1 - e0;
    if (d == 0) continue;
    const bool masks = d <= 32;  // wave-uniform
    I8MinPair p[4];
    uint32_t neg[4] = {0, 0, 0, 0};  // bit i: input i of codeword k is negative (rows of at most 32 edges)
    uint32_t sgn = 0;                // XOR of the packed inputs: bit 7 of byte k = parity of the negative inputs
    uint32_t par = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) p[k].k1 = p[k].k2 = ~0u;
    for (uint32_t i0 = 0; i0 < d; i0 += U) {
      Post4 pv[U];
      uint32_t cv[U], mv[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (i0 + u < d) {
          const uint32_t v = edge_col[e0 + i0 + u];
          if (FIRST) {
            cv[u] = *reinterpret_cast<const uint32_t *>(chan + size_t(v) * tile);
          } else {
            pv[u] = *reinterpret_cast<const Post4 *>(post + size_t(v) * tile);
            mv[u] = *reinterpret_cast<const uint32_t *>(msg + size_t(e0 + i0 + u) * tile);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (i0 + u < d) {
          const uint32_t i = i0 + u;
#pragma unroll
          for (int k = 0; k < 4; k++) {
            int x;
            if (FIRST) {
              x = byte_of(cv[u], k);  // first variable messages are the channel LLRs
            } else {
              const int l = pv[u].v[k];
              x = i8_clip(l - byte_of(mv[u], k));
              if (l <= 0) par ^= 1u << k;
            }
            i8_min_track(p[k], uint32_t(iabs(x)), i);
            const uint32_t n = uint32_t(x) >> 31;
            sgn ^= n << (8 * k);
            if (masks) neg[k] |= n << (i & 31u);
          }
        }
      }
    }
    odd_acc |= par;
    const I8RowOut r = i8_minsum_row(p, o);
    if (masks) {
      for (uint32_t i = 0; i < d; i++) {
        uint32_t s01 = sgn;
#pragma unroll
        for (int k = 0; k < 4; k++) s01 ^= ((neg[k] >> i) & 1u) << (8 * k);
        *reinterpret_cast<uint32_t *>(msg + size_t(e0 + i) * tile) = i8_minsum_word(r, i, s01);
      }
    } else {
      for (uint32_t i0 = 0; i0 < d; i0 += U) {
        Post4 pv[U];
        uint32_t cv[U], mv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          if (i0 + u < d) {
            const uint32_t v = edge_col[e0 + i0 + u];
            if (FIRST) {
              cv[u] = *reinterpret_cast<const uint32_t *>(chan + size_t(v) * tile);
            } else {
              pv[u] = *reinterpret_cast<const Post4 *>(post + size_t(v) * tile);
              mv[u] = *reinterpret_cast<const uint32_t *>(msg + size_t(e0 + i0 + u) * tile);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
          if (i0 + u < d) {
            uint32_t s01 = sgn;
#pragma unroll
            for (int k = 0; k < 4; k++) {
              // the sign of clip(l - m) is the sign of l - m
              const int x = FIRST ? byte_of(cv[u], k) : pv[u].v[k] - byte_of(mv[u], k);
              s01 ^= (uint32_t(x) >> 31) << (8 * k);
            }
            *reinterpret_cast<uint32_t *>(msg + size_t(e0 + i0 + u) * tile) = i8_minsum_word(r, i0 + u, s01);
          }
        }
      }
    }
  }
  if (!FIRST) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (odd_acc & (1u << k)) unsat_out[off + k] = 1u;
  }
}

// ---- layered schedule: one dependency level ------------------------------------------------------
// The rows of a level share no variable, so a row's Qv can be read twice.  DMAX > 0: the level's rows have at most DMAX edges
// and Qv / R of the whole row stay in registers between the two passes (as hl_i8_reg_kernel); DMAX = 0: rows of any length,
// the second pass re-reads them.  Qv += new - old, R = new; the sign of an input clip(Qv - R) is the sign of Qv - R.
template <int DMAX, bool FIRST>
__global__ __launch_bounds__(256) void hl_i8_minsum_kernel(Graph g, Sched sc, State st, I8MinsumOpts o,
                                                           const uint32_t *__restrict__ level_rows, uint32_t n_level_rows,
                                                           int16_t *__restrict__ Q, int8_t *__restrict__ R) {
  constexpr int U = 8;
  constexpr int NR = DMAX > 0 ? DMAX : 1;
  if (group_finished(st)) return;
  const TablePtr row_ptr = table_ptr(g.row_ptr), edge_col = table_ptr(g.edge_col);
  const uint32_t tile = sc.tile;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uniform((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  uint32_t chunk, node0;
  wave_slot(sc, wave, &chunk, &node0);
  if (chunk >= sc.nchunks) return;
  const uint32_t b0 = chunk * 256;
  if (b0 >= *st.n_slots) return;
  const size_t off = size_t(b0) + lane * 4;
  Q += tile_base(b0, g.n_cols, sc) + lane * 4;
  R += tile_base(b0, g.n_edges, sc) + lane * 4;
  bool frozen[4];
  bool any_live = false, all_live = true;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    frozen[k] = st.done[off + k] != 0;
    any_live = any_live || !frozen[k];
    all_live = all_live && !frozen[k];
  }
  if (__builtin_amdgcn_ballot_w64(any_live) == 0) return;
  // frozen codewords are never rewritten
  auto update = [&](uint32_t v, uint32_t e, uint32_t i, const Post4 &q, uint32_t r, uint32_t sgn, const I8RowOut &out) {
    uint32_t s01 = sgn;
#pragma unroll
    for (int k = 0; k < 4; k++) s01 ^= (uint32_t(q.v[k] - byte_of(r, k)) >> 31) << (8 * k);
    const uint32_t ow = i8_minsum_word(out, i, s01);
    int16_t *qp = Q + size_t(v) * tile;
    int8_t *rp = R + size_t(e) * tile;
    Post4 qn;
#pragma unroll
    for (int k = 0; k < 4; k++) qn.v[k] = static_cast<int16_t>(q.v[k] - byte_of(r, k) + byte_of(ow, k));
    if (all_live) {
      *reinterpret_cast<Post4 *>(qp) = qn;
      *reinterpret_cast<uint32_t *>(rp) = ow;
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (!frozen[k]) {
          qp[k] = qn.v[k];
          rp[k] = static_cast<int8_t>(byte_of(ow, k));
        }
    }
  };
  auto track = [&](I8MinPair *p, uint32_t &sgn, uint32_t i, const Post4 &q, uint32_t r) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int x = i8_clip(q.v[k] - byte_of(r, k));
      i8_min_track(p[k], uint32_t(iabs(x)), i);
      sgn ^= (uint32_t(x) >> 31) << (8 * k);
    }
  };
  for (uint32_t idx = node0; idx < n_level_rows; idx += sc.waves_per_chunk) {
    const uint32_t c = table_ptr(level_rows)[idx];
    const uint32_t e0 = row_ptr[c], e1 = row_ptr[c + 1];
    const uint32_t d = e1 - e0;
    if (d == 0) continue;
    I8MinPair p[4];
    uint32_t sgn = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) p[k].k1 = p[k].k2 = ~0u;
    if constexpr (DMAX > 0) {
      uint32_t cols[NR];
#pragma unroll
      for (int i = 0; i < NR; i++) cols[i] = edge_col[e0 + min(uint32_t(i), d - 1)];
      Post4 q[NR];
      uint32_t r[NR];
#pragma unroll
      for (int i = 0; i < NR; i++) {
        if (uint32_t(i) < d) {
          q[i] = *reinterpret_cast<const Post4 *>(Q + size_t(cols[i]) * tile);
          r[i] = FIRST ? 0u : *reinterpret_cast<const uint32_t *>(R + size_t(e0 + i) * tile);
        }
      }
#pragma unroll
      for (int i = 0; i < NR; i++)
        if (uint32_t(i) < d) track(p, sgn, uint32_t(i), q[i], r[i]);
      const I8RowOut out = i8_minsum_row(p, o);
#pragma unroll
      for (int i = 0; i < NR; i++)
        if (uint32_t(i) < d) update(cols[i], e0 + i, uint32_t(i), q[i], r[i], sgn, out);
    } else {
      for (int pass = 0; pass < 2; pass++) {
        I8RowOut out;
        if (pass == 1) out = i8_minsum_row(p, o);
        for (uint32_t i0 = 0; i0 < d; i0 += U) {
          Post4 q[U];
          uint32_t r[U], cols[U];
#pragma unroll
          for (int u = 0; u < U; u++) {
            if (i0 + u < d) {
              cols[u] = edge_col[e0 + i0 + u];
              q[u] = *reinterpret_cast<const Post4 *>(Q + size_t(cols[u]) * tile);
              r[u] = FIRST ? 0u : *reinterpret_cast<const uint32_t *>(R + size_t(e0 + i0 + u) * tile);
            }
          }
#pragma unroll
          for (int u = 0; u < U; u++) {
            if (i0 + u < d) {
              if (pass == 0)
                track(p, sgn, i0 + u, q[u], r[u]);
              else
                update(cols[u], e0 + i0 + u, i0 + u, q[u], r[u], sgn, out);
            }
          }
        }
      }
    }
  }
}

}  // namespace dev
}  // namespace ldpc
