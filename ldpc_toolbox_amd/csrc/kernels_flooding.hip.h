// Flooding schedule: the row-record helpers and the variable-node kernels, then the check-node kernels -- min-sum (per-edge
// messages, L-free variant, ROW RECORDS -- the headline kernel) and the LDS-staged check nodes of every rule.  The kernels
// min-sum can take are templates with a trailing pack for the normalized / offset correction (see the note above
// cn_minsum_kernel).  Part of kernels.hip.h (include that).
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
// moves 3 + 5 + 1 + 3 + 5 + 1 = 18 words where cn_minsum_lfree_kernel moves 22-24 -- 17 with 16-bit flags, below.
//   rec_in / rec_out  [M * RECW][tile]  words of T's size: row c occupies rows c*RECW .. c*RECW + RECW-1
//   with 16-bit flags (F16; rows of at most 12 edges, graph_tables.h record_flag_bits) a pair of arrays, RecPair:
//     mag    [M * 2][tile]  of T: min1 and min2 of row c in rows 2c and 2c + 1
//     flags  [M][tile]      of uint16_t: flip bits 0..11, argmin in bits 12..15
//   a record is then 2.5 words of f32 (2.25 of f64) in each direction
//   with byte flags (F8; rows of at most 7 edges, graph_tables.h record_flag_bytes) the same pair with flags [M][tile] of
//   uint8_t and two argmin bits in the magnitudes' sign bits (record_flags8.h): 2.25 words of f32 (2.125 of f64)
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
// (the constants themselves: graph_tables.h)

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

// 16-bit flags (flooding records of rows of at most 12 edges: graph_tables.h, record_flag_bits): the flags leave the
// record's rows for an array of their own, [M][tile] of uint16_t beside the magnitudes' [2M][tile] of T (rows 2c, 2c+1),
// both tiled like every other array.  Byte flags (rows of at most 7 edges: graph_tables.h, record_flag_bytes; the format:
// record_flags8.h): the same array with one byte per row and codeword.  A lane's VEC flag words of type FW are one buffer
// access of sizeof(FW) * VEC bytes: b64 / b32 / b16 / b8.
constexpr int kArgShift16 = 12;  // flip bits at 0..11, argmin at 12..15
static_assert(kArgShift16 == kRecArgShift16, "record_flags8.h encodes the register form of the 16-bit flags");
template <typename FW, int VEC, bool NT>
__device__ __forceinline__ Pack<FW, VEC> flags_load(const RowBuf &b, uint32_t lane_off, uint32_t row_off) {
  constexpr int kBytes = sizeof(FW) * VEC;
  static_assert(kBytes == 1 || kBytes == 2 || kBytes == 4 || kBytes == 8, "pack size");
  if constexpr (kBytes == 1)
    return __builtin_bit_cast(Pack<FW, VEC>, __builtin_amdgcn_raw_buffer_load_b8(b.r, lane_off, row_off, NT ? 2 : 0));
  else if constexpr (kBytes == 2)
    return __builtin_bit_cast(Pack<FW, VEC>, __builtin_amdgcn_raw_buffer_load_b16(b.r, lane_off, row_off, NT ? 2 : 0));
  else if constexpr (kBytes == 4)
    return __builtin_bit_cast(Pack<FW, VEC>, __builtin_amdgcn_raw_buffer_load_b32(b.r, lane_off, row_off, NT ? 2 : 0));
  else
    return __builtin_bit_cast(Pack<FW, VEC>, __builtin_amdgcn_raw_buffer_load_b64(b.r, lane_off, row_off, NT ? 2 : 0));
}
template <typename FW, int VEC, bool NT>
__device__ __forceinline__ void flags_store(const RowBuf &b, uint32_t lane_off, uint32_t row_off, const Pack<FW, VEC> &x) {
  constexpr int kBytes = sizeof(FW) * VEC;
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  if constexpr (kBytes == 1)
    __builtin_amdgcn_raw_buffer_store_b8(__builtin_bit_cast(uint8_t, x), b.r, lane_off, row_off, NT ? 2 : 0);
  else if constexpr (kBytes == 2)
    __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(uint16_t, x), b.r, lane_off, row_off, NT ? 2 : 0);
  else if constexpr (kBytes == 4)
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, x), b.r, lane_off, row_off, NT ? 2 : 0);
  else
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, x), b.r, lane_off, row_off, NT ? 2 : 0);
}

// Where a launch finds the records: one array of T (flags in the record's own rows), or with 16-bit flags the magnitudes
// and the flags array, RecPair.  Ref: the kernel argument; Buf: the wavefront's slice behind buffer descriptors.
// F8 (with F16: the byte form stores the 16-bit family's records): the same pair, the flags as bytes.
template <typename T, bool F16, bool F8 = false>
struct RecRef {
  static_assert(!F8, "byte flags: a form of the 16-bit family");
  typedef const T *__restrict__ in;
  typedef T *__restrict__ out;
};
template <typename T, typename FW>
struct RecPair {
  static_assert(std::is_same_v<FW, uint16_t> || std::is_same_v<FW, uint8_t>, "flags word: uint16_t or uint8_t");
  T *mag;
  FW *flags;
};
template <typename T, bool F8>
struct RecRef<T, true, F8> {
  typedef RecPair<const T, std::conditional_t<F8, uint8_t, uint16_t>> in;
  typedef RecPair<T, std::conditional_t<F8, uint8_t, uint16_t>> out;
};
// the type of a record's stored flags word: the decoder's own word, uint16_t (F16) or uint8_t (F16 and F8)
template <typename T, bool F16, bool F8 = false>
using RecFlagWord = std::conditional_t<F16, std::conditional_t<F8, uint8_t, uint16_t>, typename RecWord<T>::type>;
template <bool F16>
struct RecBuf {
  RowBuf b;
};
template <>
struct RecBuf<true> {
  RowBuf b, f;
};
// the slice of codewords b0.. of the records of n_rows rows (row_bytes: tile * sizeof(T))
template <typename T, int RECW>
__device__ __forceinline__ RecBuf<false> rec_buf(const T *rec, uint32_t b0, uint32_t n_rows, const Sched &sc, uint32_t row_bytes) {
  return RecBuf<false>{row_buf(rec + tile_base(b0, n_rows * RECW, sc),
                               uint64_t(n_rows) * RECW * row_bytes - in_tile_of(b0, sc) * uint32_t(sizeof(T)))};
}
template <typename T, int RECW, typename TT, typename FW>
__device__ __forceinline__ RecBuf<true> rec_buf(const RecPair<TT, FW> &rec, uint32_t b0, uint32_t n_rows, const Sched &sc,
                                                uint32_t row_bytes) {
  static_assert(RECW == 3, "16-bit and byte flags: the three-word family");
  const uint32_t in_tile = in_tile_of(b0, sc);
  return RecBuf<true>{row_buf(rec.mag + tile_base(b0, n_rows * 2, sc), uint64_t(n_rows) * 2 * row_bytes - in_tile * uint32_t(sizeof(T))),
                      row_buf(rec.flags + tile_base(b0, n_rows, sc), (uint64_t(n_rows) * sc.tile - in_tile) * sizeof(FW))};
}

// FW, the type of the stored flags word: the decoder's own word (this form: the flags are the record's third row, and a
// fourth for RECW == 4) or uint16_t / uint8_t (the specialisations below)
template <typename T, int VEC, int RECW, typename FW = typename RecWord<T>::type>
struct RowRec {
  static_assert(std::is_same_v<FW, typename RecWord<T>::type>, "flags word: RecWord<T>::type, uint16_t or uint8_t");
  typedef typename RecWord<T>::type W;
  // the flags word of a new record (RECW == 3): flip bits below the argmin
  static __device__ __forceinline__ W pack_flags(W fl, uint32_t arg) {
    return (fl & ((W(1) << RecWord<T>::kArgShift) - 1)) | (W(arg) << RecWord<T>::kArgShift);
  }
  typedef RowRec New;  // a record built in registers
  static constexpr uint32_t kRows = RECW;  // rows of T per record: row c's record is at row_off = c * kRows * row_bytes
  __device__ __forceinline__ void load(const RecBuf<false> &b, uint32_t lane_off, uint32_t row_off, uint32_t row_bytes) {
    load(b.b, lane_off, row_off, row_bytes);
  }
  template <bool NT>
  __device__ __forceinline__ void store(const RecBuf<false> &b, uint32_t lane_off, uint32_t row_off, uint32_t row_bytes) const {
    store<NT>(b.b, lane_off, row_off, row_bytes);
  }
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
// the three-word family with its flags as 16-bit words in an array of their own: every row still has flags of its own,
// `value` returns what the wide form returns
template <typename T, int VEC>
struct RowRec<T, VEC, 3, uint16_t> {
  typedef typename RecWord<T>::type W;
  static __device__ __forceinline__ uint16_t pack_flags(W fl, uint32_t arg) {
    return uint16_t((uint32_t(fl) & ((1u << kArgShift16) - 1)) | (arg << kArgShift16));
  }
  typedef RowRec New;
  static constexpr uint32_t kRows = 2;
  Pack<T, VEC> min1, min2;
  Pack<uint16_t, VEC> flip;
  // lane_off, row_off: byte offsets in the magnitudes (row c: c * 2 * tile * sizeof(T)).  The flags of the same codewords
  // and row sit at lane_off * 2 / sizeof(T) and c * tile * 2 = row_off / sizeof(T) in theirs.
  __device__ __forceinline__ void load(const RecBuf<true> &b, uint32_t lane_off, uint32_t row_off, uint32_t row_bytes) {
    min1 = buf_load<T, VEC, false>(b.b, lane_off, row_off);
    min2 = buf_load<T, VEC, false>(b.b, lane_off, row_off + row_bytes);
    flip = flags_load<uint16_t, VEC, false>(b.f, lane_off / uint32_t(sizeof(T) / sizeof(uint16_t)), row_off / uint32_t(sizeof(T)));
  }
  template <bool NT>
  __device__ __forceinline__ void store(const RecBuf<true> &b, uint32_t lane_off, uint32_t row_off, uint32_t row_bytes) const {
    buf_store<T, VEC, NT>(b.b, lane_off, row_off, min1);
    buf_store<T, VEC, NT>(b.b, lane_off, row_off + row_bytes, min2);
    flags_store<uint16_t, VEC, NT>(b.f, lane_off / uint32_t(sizeof(T) / sizeof(uint16_t)), row_off / uint32_t(sizeof(T)), flip);
  }
  __device__ __forceinline__ T value(uint32_t slot, int k) const {
    const uint32_t f = flip.v[k];
    const T mag = ((f >> kArgShift16) == slot) ? min2.v[k] : min1.v[k];
    const W sign = W(f >> slot) << (8 * sizeof(W) - 1);  // widened before the shift that makes the sign bit
    return __builtin_bit_cast(T, __builtin_bit_cast(W, mag) | sign);
  }
};
// The same records with their flags as bytes (record_flags8.h).  New: a record built in registers (the 16-bit form's
// members), encoded at `store`.  A loaded record has two forms.  RowRec<T, VEC, 3, uint8_t>, the form of the variable-node
// kernels (vn_kernel: its record form and its event block; vn_free_rec_kernel), holds what `load` read, as it is in memory,
// and `value` decodes it into the 16-bit form's registers on the spot: they take one value, or two, of each record they
// load.  RowRec8Once below is the check-node kernel's, which takes up to eight values of a record and decodes it once.
// (Until profiles/cn_flags8_decode.txt the check-node kernel used the first form too: 4804 vector instructions against the
// 16-bit twin's 2903, and 25 us of 812 lost to them -- profiles/record_flags8.txt, sections 3 to 5.)
template <typename T, int VEC>
struct RowRec8New : RowRec<T, VEC, 3, uint16_t> {
  typedef typename RecWord<T>::type W;
  template <bool NT>
  __device__ __forceinline__ void store(const RecBuf<true> &b, uint32_t lane_off, uint32_t row_off, uint32_t row_bytes) const {
    Pack<T, VEC> m1, m2;
    Pack<uint8_t, VEC> fl;
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      const RecFlags8Stored<W> r = record_flags8_encode<W>(__builtin_bit_cast(W, this->min1.v[k]),
                                                           __builtin_bit_cast(W, this->min2.v[k]), this->flip.v[k]);
      m1.v[k] = __builtin_bit_cast(T, r.min1);
      m2.v[k] = __builtin_bit_cast(T, r.min2);
      fl.v[k] = r.byte;
    }
    buf_store<T, VEC, NT>(b.b, lane_off, row_off, m1);
    buf_store<T, VEC, NT>(b.b, lane_off, row_off + row_bytes, m2);
    flags_store<uint8_t, VEC, NT>(b.f, lane_off / uint32_t(sizeof(T)), row_off / uint32_t(2 * sizeof(T)), fl);
  }
};
template <typename T, int VEC>
struct RowRec<T, VEC, 3, uint8_t> {
  typedef typename RecWord<T>::type W;
  typedef RowRec8New<T, VEC> New;
  static __device__ __forceinline__ uint16_t pack_flags(W fl, uint32_t arg) { return New::pack_flags(fl, arg); }
  static constexpr uint32_t kRows = 2;
  Pack<T, VEC> min1, min2;   // as stored: argmin bits 1 and 2 in the sign bits
  Pack<uint8_t, VEC> fl;
  __device__ __forceinline__ void load(const RecBuf<true> &b, uint32_t lane_off, uint32_t row_off, uint32_t row_bytes) {
    min1 = buf_load<T, VEC, false>(b.b, lane_off, row_off);
    min2 = buf_load<T, VEC, false>(b.b, lane_off, row_off + row_bytes);
    fl = flags_load<uint8_t, VEC, false>(b.f, lane_off / uint32_t(sizeof(T)), row_off / uint32_t(2 * sizeof(T)));
  }
  __device__ __forceinline__ T value(uint32_t slot, int k) const {
    const RecFlags8Loaded<W> r = record_flags8_decode<W>(__builtin_bit_cast(W, min1.v[k]), __builtin_bit_cast(W, min2.v[k]), fl.v[k]);
    const uint32_t f = r.flags;
    const W mag = ((f >> kArgShift16) == slot) ? r.min2 : r.min1;
    const W sign = W(f >> slot) << (8 * sizeof(W) - 1);
    return __builtin_bit_cast(T, mag | sign);
  }
};
// The byte form as the check-node kernel holds it (cn_minsum_rec_kernel with F8): the magnitudes and the lane's VEC flag
// bytes as stored, in one register, and beside them ONE register of argmins, byte k the argmin of codeword k, put together
// once at `load`.  A value is then record_flags8_value's select between the two stored words and one bit-field insert of the
// shifted flip bit over the stored sign bit -- compare, select, shift, insert: what the 16-bit form spends -- in the ten
// registers per record (f32 pack of 4) that form holds, and nothing is masked at `load`.
template <typename T, int VEC>
struct RowRec8Once {
  typedef typename RecWord<T>::type W;
  typedef RowRec8New<T, VEC> New;
  static constexpr uint32_t kRows = 2;
  Pack<T, VEC> min1, min2;  // as stored: argmin bits 1 and 2 in the sign bits
  uint32_t fl, arg;         // byte k: codeword k's stored flags byte; its argmin
  __device__ __forceinline__ void load(const RecBuf<true> &b, uint32_t lane_off, uint32_t row_off, uint32_t row_bytes) {
    min1 = buf_load<T, VEC, false>(b.b, lane_off, row_off);
    min2 = buf_load<T, VEC, false>(b.b, lane_off, row_off + row_bytes);
    const Pack<uint8_t, VEC> bytes = flags_load<uint8_t, VEC, false>(b.f, lane_off / uint32_t(sizeof(T)), row_off / uint32_t(2 * sizeof(T)));
    fl = 0;
#pragma unroll
    for (int k = 0; k < VEC; k++) fl |= uint32_t(bytes.v[k]) << (8 * k);
    // bit 0 of all VEC argmins with one shift and one mask, then bits 1 and 2 from each codeword's sign bits
    uint32_t a = (fl >> 7) & 0x01010101u;
#pragma unroll
    for (int k = 0; k < VEC; k++)
      a |= record_flags8_arg<W>(__builtin_bit_cast(W, min1.v[k]), __builtin_bit_cast(W, min2.v[k]), uint8_t(0)) << (8 * k);
    // (both words opaque to the compiler: it would otherwise take them apart again and keep a byte and an argmin per codeword
    // in registers of their own, which is the register count this form exists to avoid)
    asm("" : "+v"(fl));
    asm("" : "+v"(a));
    arg = a;
  }
  __device__ __forceinline__ T value(uint32_t slot, int k) const {
    return __builtin_bit_cast(T, record_flags8_value<W>(__builtin_bit_cast(W, min1.v[k]), __builtin_bit_cast(W, min2.v[k]),
                                                        uint8_t(fl >> (8 * k)), (arg >> (8 * k)) & 0xFFu, slot));
  }
};


// Posterior of the L-free variables from the row records: L = chan + (m_a + m_b), the messages read out of the
// records of the variable's one or two rows (free_rs: row << 6 | slot per edge, kAuxNone = no such edge).
//   event_iteration < 0: after the last iteration (no later check-node pass rebuilds it), for the codewords
//                        still running; frozen codewords are skipped;
//   event_iteration >= 0: after the variable-node pass that latched the FIRST converged codewords of a slice
//                        (State::slice_state == 1) at that iteration count: for exactly those codewords, whose
//                        L-free posteriors the check-node kernel had not been storing.
// F16: the records' flags are 16-bit words in an array of their own (RecRef / RowRec above); F8: bytes.
template <typename T, int VEC, int RECW, bool F16 = false, bool F8 = false>
__global__ __launch_bounds__(256) void vn_free_rec_kernel(Graph g, Sched sc, State st, const uint32_t *__restrict__ free_rs_,
                                                          const T *__restrict__ chan, typename RecRef<T, F16, F8>::in rec,
                                                          T *__restrict__ post, int32_t event_iteration) {
  typedef RowRec<T, VEC, RECW, RecFlagWord<T, F16, F8>> Rec;
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
  const RecBuf<F16> b_rec = rec_buf<T, RECW>(rec, b0, g.n_rows, sc, row_bytes);
  bool live[VEC];  // the codewords this pass writes
  bool any_live = false;
#pragma unroll
  for (int k = 0; k < VEC; k++) {
    live[k] = event_iteration < 0 ? st.done[off + k] == 0 : (st.done[off + k] != 0 && st.iters[off + k] == event_iteration);
    any_live = any_live || live[k];
  }
  if (__builtin_amdgcn_ballot_w64(any_live) == 0) return;
  // (the L-free rebuild loop: vn_kernel's event block has the other copy)
  for (uint32_t i = i0; i < g.n_list; i += sc.waves_per_chunk) {
    const uint32_t v = free_var[i], a = free_rs[2 * i], b = free_rs[2 * i + 1];
    const Pack<T, VEC> ch = load_pack<T, VEC>(chan + size_t(v) * G);
    Rec ra, rb;
    if (a != kAuxNone) ra.load(b_rec, lane_off, (a >> 6) * Rec::kRows * row_bytes, row_bytes);
    if (b != kAuxNone) rb.load(b_rec, lane_off, (b >> 6) * Rec::kRows * row_bytes, row_bytes);
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      T sum = -T(0.0);  // arithmetic.rs:146: the slot-ordered sum, from Rust's float Sum identity
      if (a != kAuxNone) sum = sum + ra.value(a & 63u, k);
      if (b != kAuxNone) sum = sum + rb.value(b & 63u, k);
      if (live[k]) post[size_t(v) * G + k] = ch.v[k] + sum;
    }
  }
}

// The closing launch of a call that asked for no posterior ("call_edges"): vn_free_rec_kernel's event_iteration < 0 form with
// the hard decisions L <= 0 (arithmetic.rs:198-200) as its only output -- L = chan + (m_a + m_b) is formed as above and
// ballotted straight into pack_hard_kernel's words, bits[v][W]; no posterior row is stored.  The words of a frozen codeword
// come from its stored row (its L-free rows were stored when it converged): a wave whose codewords are all live reads no
// posterior, one whose codewords are all frozen no records.  Runs behind the pack of the rows the variable-node launch writes
// and covers every L-free variable, wherever its row lies.
// A lane holds the VEC codewords b0 + VEC * lane + k; packed word j of the slice holds b0 + 64 j + i in bit i, which is
// element i % VEC of lane (64 j + i) / VEC: each lane picks its bit out of the VEC ballots and the wave ballots again.
template <typename T, int VEC, int RECW, bool F16 = false, bool F8 = false>
__global__ __launch_bounds__(256) void vn_free_hard_kernel(Graph g, Sched sc, State st, const uint32_t *__restrict__ free_rs_,
                                                           const T *__restrict__ chan, typename RecRef<T, F16, F8>::in rec,
                                                           const T *__restrict__ post, uint64_t *__restrict__ bits, uint32_t W) {
  typedef RowRec<T, VEC, RECW, RecFlagWord<T, F16, F8>> Rec;
  if (*st.n_active == 0) return;
  const TablePtr free_var = table_ptr(g.list_var), free_rs = table_ptr(free_rs_);
  const uint32_t lane = threadIdx.x & 63u, tile = sc.tile;
  const uint32_t wave = uniform((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  uint32_t chunk, i0;
  wave_slot(sc, wave, &chunk, &i0);
  if (chunk >= sc.nchunks) return;
  const uint32_t b0 = chunk * (64 * VEC);
  if (b0 >= *st.n_slots) return;
  const size_t off = size_t(b0) + lane * VEC;
  const size_t G = tile;
  chan += tile_base(b0, g.n_cols, sc) + lane * VEC;
  post += tile_base(b0, g.n_cols, sc) + lane * VEC;
  bits += chunk * VEC;
  const uint32_t row_bytes = tile * uint32_t(sizeof(T)), lane_off = lane * uint32_t(VEC * sizeof(T));
  const RecBuf<F16> b_rec = rec_buf<T, RECW>(rec, b0, g.n_rows, sc, row_bytes);
  bool live[VEC];
  bool any_live = false, all_live = true;
#pragma unroll
  for (int k = 0; k < VEC; k++) {
    live[k] = st.done[off + k] == 0;
    any_live = any_live || live[k];
    all_live = all_live && live[k];
  }
  any_live = __builtin_amdgcn_ballot_w64(any_live) != 0;   // wave-uniform, both
  all_live = __builtin_amdgcn_ballot_w64(!all_live) == 0;
  const uint32_t mine = lane % VEC, at = lane / VEC;
  for (uint32_t i = i0; i < g.n_list; i += sc.waves_per_chunk) {
    const uint32_t v = free_var[i], a = free_rs[2 * i], b = free_rs[2 * i + 1];
    Pack<T, VEC> x;
    if (any_live) {
      const Pack<T, VEC> ch = load_pack<T, VEC>(chan + size_t(v) * G);
      Rec ra, rb;
      if (a != kAuxNone) ra.load(b_rec, lane_off, (a >> 6) * Rec::kRows * row_bytes, row_bytes);
      if (b != kAuxNone) rb.load(b_rec, lane_off, (b >> 6) * Rec::kRows * row_bytes, row_bytes);
#pragma unroll
      for (int k = 0; k < VEC; k++) {
        T sum = -T(0.0);  // arithmetic.rs:146: the slot-ordered sum, from Rust's float Sum identity
        if (a != kAuxNone) sum = sum + ra.value(a & 63u, k);
        if (b != kAuxNone) sum = sum + rb.value(b & 63u, k);
        x.v[k] = ch.v[k] + sum;
      }
    }
    if (!all_live) {
      const Pack<T, VEC> old = load_pack<T, VEC>(post + size_t(v) * G);
#pragma unroll
      for (int k = 0; k < VEC; k++) x.v[k] = (any_live && live[k]) ? x.v[k] : old.v[k];
    }
    uint64_t picked = 0;  // the ballot of this lane's element of every lane
#pragma unroll
    for (int k = 0; k < VEC; k++) {
      const uint64_t bal = __builtin_amdgcn_ballot_w64(x.v[k] <= T(0.0));
      picked = (mine == uint32_t(k)) ? bal : picked;
    }
#pragma unroll
    for (int j = 0; j < VEC; j++) {
      const uint64_t word = __builtin_amdgcn_ballot_w64(((picked >> (uint32_t(j) * (64 / VEC) + at)) & 1ull) != 0);
      if (lane == 0) bits[size_t(v) * W + j] = word;
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
template <typename RecIn>
struct VnEvent {
  const uint32_t *free_var, *free_rs;  // the L-free variables and, per variable, its two (row << 6 | slot) words
  RecIn rec;                           // records of the iteration being latched
  uint32_t n_free;
};
// (EVF16, EVF8: those records' flags are 16-bit words in an array of their own; stored as bytes)
template <typename T, bool EVF16, bool EVF8 = false>
using VnEventOf = VnEvent<typename RecRef<T, EVF16, EVF8>::in>;
__device__ __forceinline__ bool has_records(const void *rec) { return rec != nullptr; }
template <typename T, typename FW>
__device__ __forceinline__ bool has_records(const RecPair<T, FW> &rec) { return rec.mag != nullptr; }
// What the kernel sums, SRC... src: one kernel argument or two, where they have always been.  The per-edge messages the
// check-node launch stored -- `const T *__restrict__ msg`, [E][tile], gathered through col_edge ...
template <typename... SRC>
struct VnSource;
template <typename M>
struct VnSource<M> {
  M msg;
};
// ... or, REC, the ROW RECORDS the check-node launch of THIS iteration wrote -- `RecRef<T, true, EVF8>::in rec, const uint32_t
// *__restrict__ keep_rs`: the list variant with the per-edge message array taken out of the iteration.  The message on a kept
// edge is already in the record its row wrote in the same iteration -- Rec::value(slot, k) is the very pack
// cn_minsum_rec_kernel's `send` stores -- so the kernel gathers, per edge, the record of the edge's row (keep_rs: row << 6 |
// slot per edge of the kept list, graph_tables.h build_keep_rs) and the check-node launch stores no per-edge messages at all
// (its SEND = false form).  Same sum, same order.  The 16-bit-flags record form only (rows of at most 12 edges; EVF8: stored
// with byte flags, rows of at most 7 edges, rec and ev.rec alike); a record is 2.5 words of f32 where a message was one, but a
// row's record is wanted by every kept edge of the row and is fetched from HBM once per tile.
template <typename R, typename K>
struct VnSource<R, K> {
  R rec;
  K keep_rs;
};
// ... or, CHAIN, those two and a third argument, `VnChain chain`: the kept list in CHAINS (graph_tables.h, build_vn_chains).
// The list comes in blocks of width * len entries, block position (t, w) at index (block * len + t) * width + w.  The waves of
// a slice form groups of `mates`: group g takes the blocks g, g + n_groups, ...; its wave m walks, in every block, the runs
// w = m, m + mates, ... one after the other, each from t = 0 to len - 1.  Along a run the wave keeps ONE record in registers
// (the carry, as memory holds it): an edge marked kChainFrom fetches no record of its own and takes its value from the carry,
// at its own position of the sum; the record of the edge marked kChainLeave is copied into the carry once it has arrived.
// Both marks are wave-uniform, and the tables never mark kChainFrom at t = 0: a run starts with whatever the carry holds and
// never reads it.
struct VnChain {
  uint32_t len, width, mates, n_blocks, n_groups;
};
template <typename R, typename K, typename C>
struct VnSource<R, K, C> {
  R rec;
  K keep_rs;
  C chain;
};
// The carry: a record of the 16-bit family as memory holds it, its VEC flag words packed into one or two registers (the
// compiler would keep a register per codeword) -- nine registers for an f32 pack of 4 with byte flags.
template <typename Rec, typename T, int VEC, typename FW>
struct VnCarry {
  static_assert(VEC * sizeof(FW) <= 8, "the flag words of a lane fit two registers");
  Pack<T, VEC> min1, min2;
  uint32_t fl[2];
  static __device__ __forceinline__ Pack<FW, VEC> &flags_of(RowRec<T, VEC, 3, uint16_t> &r) { return r.flip; }
  static __device__ __forceinline__ Pack<FW, VEC> &flags_of(RowRec<T, VEC, 3, uint8_t> &r) { return r.fl; }
  __device__ __forceinline__ void keep(Rec r) {
    min1 = r.min1;
    min2 = r.min2;
    uint64_t bits = 0;
#pragma unroll
    for (int k = 0; k < VEC; k++) bits |= uint64_t(flags_of(r).v[k]) << (8 * sizeof(FW) * k);
    fl[0] = uint32_t(bits);
    fl[1] = uint32_t(bits >> 32);
    asm("" : "+v"(fl[0]));
    if constexpr (VEC * sizeof(FW) > 4) asm("" : "+v"(fl[1]));
  }
  __device__ __forceinline__ T value(uint32_t slot, int k) const {
    Rec r;
    r.min1 = min1;
    r.min2 = min2;
    const uint64_t bits = uint64_t(fl[0]) | (uint64_t(fl[1]) << 32);
    flags_of(r).v[k] = FW(bits >> (8 * sizeof(FW) * k));
    return r.value(slot, k);
  }
};
struct VnChainWalk {
  uint32_t blk, w, t, mate;
  // the list index of the position, moved on to the next one that lies in the list; n_list: the walk is over
  __device__ __forceinline__ uint32_t settle(const VnChain &c, uint32_t n_list) {
    while (blk < c.n_blocks) {
      const uint32_t i = (blk * c.len + t) * c.width + w;
      if (t < c.len && i < n_list) return i;
      t = 0;
      w += c.mates;
      if (w >= c.width) {
        w = mate;
        blk += c.n_groups;
      }
    }
    return n_list;
  }
};
// (Arguments of their own and not one struct: a pointer inside a struct is not `noalias` to the compiler, and a struct's
// members are loaded apart from the arguments beside them -- either gives every instantiation other instructions,
// profiles/vn_kernel_merge.txt.)
//   U     messages / records in flight per lane; a variable of more edges takes further rounds
//   NT    nontemporal loads of what no other kernel reads: the messages; REC: the channel rows
//   LIST  only the variables of Graph::list_* (REC: always)
// Both forms are this one kernel, and in both it IS the iteration's variable-node launch: whoever accounts for the launches
// of an iteration by kernel name (bench.py's counter passes sum "vn_kernel") finds it.
template <typename T, int VEC, int U, bool NT, bool LIST, int EVW = 0, bool EVF16 = false, bool EVF8 = false, typename... SRC>
__global__ __launch_bounds__(256) void vn_kernel(
    Graph g, Sched sc, State st, const T *__restrict__ chan, SRC... src,
    T *__restrict__ post, const uint32_t *__restrict__ unsat_in, uint32_t *__restrict__ unsat_clear,
    int32_t latch_iteration, VnEventOf<T, EVF16, EVF8> ev = {}) {
  constexpr bool REC = sizeof...(SRC) >= 2, CHAIN = sizeof...(SRC) == 3;
  const VnSource<const SRC &...> from{src...};  // (a view: references)
  static_assert(!REC || (LIST && EVF16 && (EVW == 0 || EVW == 3)), "from records: the kept list, the 16-bit family's records");
  uint32_t *__restrict__ n_active = st.n_active;
  // A finished group's launches return at once.  With EVW the count can also reach zero INSIDE this launch -- the
  // bookkeeping waves below subtract the codewords they latch -- and a wave that starts after the last subtraction must
  // still take its share of the rebuild of those codewords' L-free posteriors: it goes on to the EVW block (where a group
  // that had finished BEFORE the launch has no `fresh` codeword and costs a few loads) and returns behind it.
  const bool idle = *n_active == 0;
  if (EVW == 0 && idle) return;
  const TablePtr col_ptr = table_ptr(LIST ? g.list_ptr : g.col_ptr);
  // (col_edge and msg here, row_bytes and lane_off below: what only one form's main loop needs belongs in that form's branch.
  // These four stay where each form has always computed them -- moved, every instantiation comes out with the same
  // instructions in another order and other registers, and they are to stay identical: tools/kernel_digest.py.)
  TablePtr col_edge = nullptr;
  if constexpr (!REC) col_edge = table_ptr(LIST ? g.list_edge : g.col_edge);
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
    if (idle && (!has_records(ev.rec) || unsat_in == nullptr || st.slice_state == nullptr || st.slice_state[chunk] == 2u)) return;
  }
  const size_t off = size_t(b0) + lane * VEC;
  const size_t G = tile;
  chan += tile_base(b0, g.n_cols, sc) + lane * VEC;
  post += tile_base(b0, g.n_cols, sc) + lane * VEC;
  const T *__restrict__ msg = nullptr;
  if constexpr (!REC) msg = from.msg + tile_base(b0, g.n_edges, sc) + lane * VEC;
  uint32_t row_bytes = 0, lane_off = 0;
  if constexpr (REC) {
    row_bytes = tile * uint32_t(sizeof(T));
    lane_off = lane * uint32_t(VEC * sizeof(T));
  }
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
    if (has_records(ev.rec) && unsat_in != nullptr && st.slice_state != nullptr && st.slice_state[chunk] != 2u) {
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
        if constexpr (!REC) {
          row_bytes = tile * uint32_t(sizeof(T));
          lane_off = lane * uint32_t(VEC * sizeof(T));
        }
        const RecBuf<EVF16> b_rec = rec_buf<T, EVW>(ev.rec, b0, g.n_rows, sc, row_bytes);
        // (the L-free rebuild loop: vn_free_rec_kernel has the other copy)
        for (uint32_t i = v_first; i < ev.n_free; i += waves_per_chunk) {
          const uint32_t fv = free_var[i], a = free_rs[2 * i], b = free_rs[2 * i + 1];
          const Pack<T, VEC> ch = load_pack<T, VEC>(chan + size_t(fv) * G);
          typedef RowRec<T, VEC, EVW, RecFlagWord<T, EVF16, EVF8>> Rec;
          Rec ra, rb;
          if (a != kAuxNone) ra.load(b_rec, lane_off, (a >> 6) * Rec::kRows * row_bytes, row_bytes);
          if (b != kAuxNone) rb.load(b_rec, lane_off, (b >> 6) * Rec::kRows * row_bytes, row_bytes);
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

  if constexpr (!REC) {  // the sum of the per-edge messages
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
  } else {  // the same sum, each message taken out of its row's record
    typedef RowRec<T, VEC, 3, RecFlagWord<T, true, EVF8>> Rec;
    const TablePtr keep_rs = table_ptr(from.keep_rs);
    const RecBuf<true> b_rec = rec_buf<T, 3>(from.rec, b0, g.n_rows, sc, row_bytes);
    const uint32_t rec_bytes = Rec::kRows * row_bytes;
    // (keep_rs is padded by kTablePad words: the block fetch of a variable's first U indices stays in bounds)
    uint32_t v = v_first, s0 = 0, s1 = 0, rs[U], var = v_first;
    [[maybe_unused]] VnChainWalk walk{};
    [[maybe_unused]] VnCarry<Rec, T, VEC, RecFlagWord<T, true, EVF8>> carry = {};
    if constexpr (CHAIN) {
      static_assert(U >= int(kChainEdges), "the marked edges of an entry are in flight together");
      walk = VnChainWalk{v_first / from.chain.mates, v_first % from.chain.mates, 0u, v_first % from.chain.mates};
      v = uniform(walk.settle(from.chain, n_cols));
    }
    if (v < n_cols) {
      s0 = col_ptr[v];
      s1 = col_ptr[v + 1];
      var = table_ptr(g.list_var)[v];
    }
#pragma unroll
    for (int u = 0; u < U; u++) rs[u] = keep_rs[s0 + u];

    while (v < n_cols) {
      T sum[VEC];
#pragma unroll
      for (int k = 0; k < VEC; k++) sum[k] = -T(0.0);
      const Pack<T, VEC> ch = load_msg<T, VEC, NT>(chan + size_t(var) * G);
      uint32_t vn = v + waves_per_chunk;
      if constexpr (CHAIN) {
        walk.t++;
        vn = uniform(walk.settle(from.chain, n_cols));
      }
      uint32_t ns0 = 0, ns1 = 0, nvar = vn;
      if (vn < n_cols) {
        ns0 = col_ptr[vn];
        ns1 = col_ptr[vn + 1];
        nvar = table_ptr(g.list_var)[vn];
      }
      uint32_t nrs[U];
      for (uint32_t j0 = s0; j0 < s1; j0 += U) {
        Rec rv[U];
        uint32_t w[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          w[u] = 0;
          if (j0 + u < s1) {  // wave-uniform
            w[u] = (j0 == s0) ? rs[u] : keep_rs[j0 + u];
            if constexpr (CHAIN) {
              // (no branch around a load: the compiler then waits for each record where it is loaded.  The edge that takes
              // the carry asks for its neighbour's record again instead, which the wave is fetching anyway, and drops what
              // arrives; what that second request costs beyond the CU is in profiles/vn_chains.txt, section 6.
              // Two properties of build_vn_chains' tables are relied on: a marked entry has a neighbour edge -- the kept
              // list holds variables of degree 3 and more only (graph_tables.h, build_lfree_tables: degree 1 and 2 are
              // L-free), so rs[1] is an edge of the same entry at u == 0 -- and the marks lie on an entry's first
              // kChainEdges edges, the round j0 == s0.)
              uint32_t row = w[u];
              if (w[u] & kChainFrom) row = u == 0 ? ((j0 == s0) ? rs[1] : keep_rs[j0 + 1]) : w[u - 1];
              rv[u].load(b_rec, lane_off, ((row & kChainRsMask) >> 6) * rec_bytes, row_bytes);
            } else {
              rv[u].load(b_rec, lane_off, (w[u] >> 6) * rec_bytes, row_bytes);
            }
          }
        }
        if (j0 == s0) {
#pragma unroll
          for (int u = 0; u < U; u++) nrs[u] = keep_rs[ns0 + u];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
          if (j0 + u < s1) {
            if constexpr (CHAIN) {
              if (w[u] & kChainFrom) {  // wave-uniform; nothing but arithmetic behind this branch
#pragma unroll
                for (int k = 0; k < VEC; k++) sum[k] = sum[k] + carry.value(w[u] & 63u, k);
                continue;
              }
            }
#pragma unroll
            for (int k = 0; k < VEC; k++) sum[k] = sum[k] + rv[u].value(w[u] & 63u, k);
          }
        }
        if constexpr (CHAIN) {
          // (behind the sums: the carry has been read; an edge with both marks leaves the carry as it is)
#pragma unroll
          for (int u = 0; u < U; u++)
            if (j0 + u < s1 && (w[u] & (kChainFrom | kChainLeave)) == kChainLeave) carry.keep(rv[u]);
        }
      }
      if (s0 == s1) {
#pragma unroll
        for (int u = 0; u < U; u++) nrs[u] = keep_rs[ns0 + u];
      }
      Pack<T, VEC> o;
#pragma unroll
      for (int k = 0; k < VEC; k++) o.v[k] = ch.v[k] + sum[k];
      T *dst = post + size_t(var) * G;
      if (all) {
        store_pack<T, VEC>(dst, o);
      } else {
#pragma unroll
        for (int k = 0; k < VEC; k++)
          if (!skip[k]) dst[k] = o.v[k];
      }
      v = vn;
      var = nvar;
      s0 = ns0;
      s1 = ns1;
#pragma unroll
      for (int u = 0; u < U; u++) rs[u] = nrs[u];
    }
  }
}
// ---------------------------------------------------------------------------------------
// The check-node kernels min-sum can take: cn_minsum (streaming), cn_minsum_lfree, cn_minsum_rec (row records), cn_staged
// (LDS-staged, every rule).  Each ends in `typename... MC` / `MC... mc` (kernels_common.hip.h, MinsumCorr): with the pack
// empty it is the kernel of plain min-sum (and of the other rules); x_kernel<..., MinsumCorr<T>> is its normalized / offset
// form, with the correction where a magnitude leaves the fold.
// ---------------------------------------------------------------------------------------

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
template <typename T, int VEC, typename MASK, int U, bool FIRST, bool NT, typename... MC>
__global__ __launch_bounds__(256) void cn_minsum_kernel(
    Graph g, Sched sc, State st, const T *__restrict__ L, T *__restrict__ msg,
    uint32_t *__restrict__ unsat_out, MC... mc) {
  constexpr bool CORR = sizeof...(MC) != 0;  // normalized / offset min-sum
  static_assert(is_corr_pack<T, MC...>, "mc: nothing, or one MinsumCorr<T>");
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
    if constexpr (CORR) {
      // once per row: every message of the row is one of these two magnitudes
#pragma unroll
      for (int k = 0; k < VEC; k++) {
        min1[k] = minsum_corrected(min1[k], mc...);
        min2[k] = minsum_corrected(min2[k], mc...);
      }
    }
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
template <typename T, int VEC, typename MASK, int U, bool FIRST, bool NT, bool NT_IN, typename... MC>
__global__ __launch_bounds__(256) void cn_minsum_lfree_kernel(
    Graph g, Sched sc, State st, const T *__restrict__ chan, T *__restrict__ post,
    const T *__restrict__ msg_in, T *__restrict__ msg, uint32_t *__restrict__ unsat_out, MC... mc) {
  constexpr bool CORR = sizeof...(MC) != 0;  // normalized / offset min-sum
  static_assert(is_corr_pack<T, MC...>, "mc: nothing, or one MinsumCorr<T>");
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
    if constexpr (CORR) {
      // once per row: every message of the row is one of these two magnitudes
#pragma unroll
      for (int k = 0; k < VEC; k++) {
        min1[k] = minsum_corrected(min1[k], mc...);
        min2[k] = minsum_corrected(min2[k], mc...);
      }
    }
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
// F16: the records' flags are 16-bit words in an array of their own (RecRef / RowRec above): rows of at most 12 edges.
// SEND = false: no per-edge messages are stored -- the variable-node launch rebuilds them from the records this launch
// writes (vn_kernel's record form); the record already holds the corrected pair, so the normalized / offset forms need nothing more.
// F8: the 16-bit family's records stored with byte flags (rows of at most 7 edges: record_flags8.h); short rows only, and
// U = 7: a row is one round of seven loads (the tables' padding, graph_tables.h kTablePad, covers any U up to 16).  The byte
// form also holds the signs and the running argmin of a row in ONE register per codeword (`sa`), folds the minima with
// selects instead of branches, and keeps a loaded record's argmins in one register (RowRec8Once): 91 VGPRs and 2929 vector
// instructions in the steady-state f32 pack-of-4 kernel, where decoding per value had 96 and 4804
// (profiles/cn_flags8_decode.txt).
// SHAPE = kCnShapePN / kCnShapeNP ("cn_row_shape"; the byte form without per-edge messages, not the first iteration): a run
// of the walk whose rows all have the graph's dominant shape -- graph_tables.h, build_row_shapes: kRowShapeKept kept slots,
// then the variable shared with the row before and the one shared with the row after (PN: DVB-S2 1/2 from its alist), or those
// two the other way round (NP), the peers' slots and the writer where that shape puts them -- takes a row step that knows all this:
// straight-line code per walk direction, no peer words, no `carry_var` / `carry_slot` compares, no far path and no tests of
// the row's length.  The other message of the slot shared with the row ahead comes from `nxt`; the variable shared with the
// row behind arrives through the LDS hand-off as its new posterior, which that row formed a step ago from the same three
// values.  Only the run's first row, whose neighbour behind belongs to another run, has that neighbour's record fetched (as
// the generic step does) and the shared channel row loaded.  Whether a run conforms is one word of the peer table (the
// row-shape counts behind the peer words), loaded beside the run's first row_ptr word; every other run -- the graph's first
// and last rows, anything odd -- takes the generic step below, in the same launch.  The same operations on the same values
// in the same slot order: results do not change, NaNs and infinities included (tests/test_cn_row_shape_gpu.py).
// profiles/cn_row_shape.txt.
enum : int { kCnShapeNone = 0, kCnShapePN = 1, kCnShapeNP = 2 };
static_assert(kCnShapePN == int(kRowShapePN) && kCnShapeNP == int(kRowShapeNP), "the kinds of graph_tables.h, build_row_shapes");
template <typename T, int VEC, int RECW, bool F16, int U, bool FIRST, bool NT, bool STREAM = false, bool LONG = true, bool SEND = true,
          bool F8 = false, int SHAPE = kCnShapeNone, typename... MC>
__global__ __launch_bounds__(256) void cn_minsum_rec_kernel(
    Graph g, Sched sc, State st, const T *__restrict__ chan, T *__restrict__ post, typename RecRef<T, F16, F8>::in rec_in,
    typename RecRef<T, F16, F8>::out rec_out, T *__restrict__ msg, uint32_t *__restrict__ unsat_out, uint32_t run, MC... mc) {
  static_assert(!F8 || (F16 && !LONG), "byte flags: rows of at most 7 edges");
  static_assert(!F8 || U == int(kRecFlags8MaxRow), "byte flags: a row is one round of 7 loads");
  static_assert(SHAPE == kCnShapeNone || ((SHAPE == kCnShapePN || SHAPE == kCnShapeNP) && F8 && !SEND && !FIRST && !STREAM),
                "row shapes: the byte form without per-edge messages, behind the first iteration");
  static_assert(kRowShapeKept + 2 <= kRecFlags8MaxRow, "the dominant shape is a row of the byte form");
  typedef std::conditional_t<F8, RowRec8Once<T, VEC>, RowRec<T, VEC, RECW, RecFlagWord<T, F16, F8>>> Rec;
  constexpr bool CORR = sizeof...(MC) != 0;  // normalized / offset min-sum
  static_assert(is_corr_pack<T, MC...>, "mc: nothing, or one MinsumCorr<T>");
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
  // (the one-array form spells out what rec_buf<T, RECW>(const T *, ...) does, with the in_tile above: through rec_buf the
  // compiler schedules the 40 instantiations that existed before the 16-bit form differently, and they are to stay
  // instruction-identical, tools/kernel_digest.py)
  RecBuf<F16> b_rin, b_rout;
  if constexpr (F16) {
    b_rin = rec_buf<T, RECW>(rec_in, b0, g.n_rows, sc, row_bytes);
    b_rout = rec_buf<T, RECW>(rec_out, b0, g.n_rows, sc, row_bytes);
  } else {
    b_rin.b = row_buf(rec_in + tile_base(b0, g.n_rows * RECW, sc), uint64_t(g.n_rows) * RECW * row_bytes - in_tile);
    b_rout.b = row_buf(rec_out + tile_base(b0, g.n_rows * RECW, sc), uint64_t(g.n_rows) * RECW * row_bytes - in_tile);
  }
  const uint32_t rec_bytes = Rec::kRows * row_bytes;
  // What a row hands to the next row of its walk, for the variable the two share (below): a pack per lane, private to the
  // lane -- written and read by the same thread in program order, so no barrier -- and double-buffered by the parity of the
  // step (`ph`): a long row may write its own hand-off in an early round and read the previous row's in a later one.
  // In LDS and not in registers: held in registers across the step, the two packs cost the steady-state f32 pack-of-4
  // kernel 8 VGPRs (96 -> 104) and with them the fifth wave per SIMD.  16 KiB per workgroup at most.
  __shared__ Pack<T, VEC> carry_chan[2][256], carry_msg[2][256];
  static_assert(sizeof(Pack<T, VEC>) * 256 * 4 <= 16384, "the hand-off arrays: 16 KiB per workgroup at most");
  uint64_t odd_m[VEC];  // lane masks (SGPR pairs): codeword k of the lane has seen an odd row
#pragma unroll
  for (int k = 0; k < VEC; k++) odd_m[k] = 0;

  for (uint32_t r = node0; r * run < n_rows; r += waves_per_chunk) {
    const uint32_t lo = r * run, hi = min(lo + run, n_rows);
    const uint32_t dir = (r & 1u) ? 0xFFFFFFFFu : 1u;  // +1 / -1 (row numbers wrap: an invalid row is >= n_rows)
    uint32_t c = (r & 1u) ? hi - 1 : lo;
    if constexpr (SHAPE != kCnShapeNone) {
      // the fitting rows from c on in the walk's direction (graph_tables.h, row_shape_run_conforms)
      const uint32_t span = edge_peer[g.n_edges + kTablePad + c];
      if (((r & 1u) ? span >> 16 : span & 0xFFFFu) >= hi - lo) {
        // UP: the walk's direction.  AHEAD / BEHIND: the slots shared with the next / the previous row of the walk
        auto shape_run = [&](auto UP) {
          constexpr bool kUp = decltype(UP)::value;
          constexpr uint32_t K = kRowShapeKept, D = K + 2;
          constexpr uint32_t NEXT = SHAPE == kCnShapePN ? K + 1 : K, PREV = SHAPE == kCnShapePN ? K : K + 1;  // in row order
          constexpr uint32_t AHEAD = kUp ? NEXT : PREV, BEHIND = kUp ? PREV : NEXT;
          constexpr uint32_t kSgnMask8 = (1u << kRecFlags8MaxRow) - 1;
          uint32_t cc = c, e0 = row_ptr[cc], cols[D];
#pragma unroll
          for (uint32_t u = 0; u < D; u++) cols[u] = edge_col[e0 + u];
          Rec recA, recB;
          {
            // The hand-off the run's first row finds: the row behind it belongs to another run, so that row's record is fetched
            // (the generic step's far fetch) and the shared channel row loaded, and the shared variable's new posterior goes
            // where a row of this run would have left it.  (Both neighbours of a fitting row exist.)  The neighbour's record
            // as memory holds it, asked for before the first row's own: the three answers come back together, where a
            // record decoded at its load (RowRec8Once) is waited for before the next request goes out.
            const uint32_t far_off = (kUp ? cc - 1 : cc + 1) * rec_bytes;
            const Pack<T, VEC> far_min1 = buf_load<T, VEC, false>(b_rin.b, lane_off, far_off);
            const Pack<T, VEC> far_min2 = buf_load<T, VEC, false>(b_rin.b, lane_off, far_off + row_bytes);
            const Pack<uint8_t, VEC> far_fl =
                flags_load<uint8_t, VEC, false>(b_rin.f, lane_off / uint32_t(sizeof(T)), far_off / uint32_t(2 * sizeof(T)));
            const Pack<T, VEC> chan_behind = buf_load<T, VEC, false>(b_chan, lane_off, cols[BEHIND] * row_bytes);
            recA.load(b_rin, lane_off, cc * rec_bytes, row_bytes);
            Pack<T, VEC> l_behind;
#pragma unroll
            for (int k = 0; k < VEC; k++) {
              const T m_far = __builtin_bit_cast(T, record_flags8_value<W>(__builtin_bit_cast(W, far_min1.v[k]),
                                                                              __builtin_bit_cast(W, far_min2.v[k]), far_fl.v[k], AHEAD));
              l_behind.v[k] = chan_behind.v[k] + (recA.value(BEHIND, k) + m_far);
            }
            carry_chan[1][threadIdx.x] = l_behind;
          }
          auto step = [&](Rec &own, Rec &nxt, uint32_t ph) {
            const uint32_t cn = kUp ? cc + 1 : cc - 1;
            nxt.load(b_rin, lane_off, cn * rec_bytes, row_bytes);
            Pack<T, VEC> lv[D];
#pragma unroll
            for (uint32_t u = 0; u < K; u++) lv[u] = buf_load<T, VEC, false>(b_post, lane_off, cols[u] * row_bytes);
            lv[AHEAD] = buf_load<T, VEC, false>(b_chan, lane_off, cols[AHEAD] * row_bytes);
            // The variable shared with the row behind: its new posterior L = chan + (m_a + m_b) as that row formed it a step ago,
            // from the same channel row and the same two messages -- there with this row's message second, and neither
            // message is ever a NaN, so the sum is the same bits either way.  A message is a stored minimum of magnitudes
            // (RowRec::value; the fold ignores NaNs) or, with the corrected rules, minsum_corrected of one, whose closing
            // select `c > 0 ? c : 0` turns a NaN (alpha = 0 on an infinite minimum) into 0: true for every alpha and beta
            lv[BEHIND] = carry_chan[ph ^ 1u][threadIdx.x];
            // the next row's columns.  Every row of the run has D edges; the row beyond the run's last one may be shorter (its
            // columns are read and not used: upwards the tables' padding covers them, downwards the offset stops at 0)
            const uint32_t ne0 = kUp ? e0 + D : e0 - min(e0, D);
            const TablePtr next_col = edge_col + ne0;  // (one address, D constant offsets)
            uint32_t ncols[D];
#pragma unroll
            for (uint32_t u = 0; u < D; u++) ncols[u] = next_col[u];
            T min1[VEC], min2[VEC];
            uint32_t sa[VEC];
            uint64_t par_m[VEC];
#pragma unroll
            for (int k = 0; k < VEC; k++) {
              min1[k] = Limits<T>::inf();
              min2[k] = Limits<T>::inf();
              sa[k] = 0;
              par_m[k] = 0;
            }
            Pack<T, VEC> lnew;  // the new posterior of the variable this row stores: the one shared with the next row in row order
#pragma unroll
            for (uint32_t u = 0; u < D; u++) {
              // A slot is a basic block of its own, behind a branch that is always taken and that the compiler cannot see
              // through.  As one block, the compiler fills the wait for the loads with everything the D slots can do ahead of
              // time and holds the results: 120 VGPRs and four waves per SIMD, or scratch under a bound of 96; in blocks: 94
              // (96 with the corrected rules).  The build checks it: `make` ends in tools/kernel_resources.py --gate.
              uint32_t always = 1;
              asm volatile("" : "+s"(always));
              if (always)
#pragma unroll
              for (int k = 0; k < VEC; k++) {
                T l = lv[u].v[k];
                const T m_own = own.value(u, k);
                if (u == AHEAD) {
                  l = l + (m_own + nxt.value(BEHIND, k));  // chan + (m_a + m_b)
                  lv[u].v[k] = l;
                }
                if (u == NEXT) lnew.v[k] = l;
                const T x = l - m_own;
                const T a = m_abs(x);
                if (x < T(0.0)) sa[k] |= 1u << u;
                par_m[k] ^= __builtin_amdgcn_ballot_w64(l <= T(0.0));
                const bool lt1 = a < min1[k], lt2 = a < min2[k];
                min2[k] = lt1 ? min1[k] : (lt2 ? a : min2[k]);
                min1[k] = lt1 ? a : min1[k];
                sa[k] = lt1 ? ((sa[k] & kSgnMask8) | (u << kArgShift16)) : sa[k];
              }
              if (u == AHEAD) carry_chan[ph][threadIdx.x] = lv[u];
            }
            if (write_post) {
              if (all_live) {
                buf_store<T, VEC, false>(b_post, lane_off, cols[NEXT] * row_bytes, lnew);
              } else {
#pragma unroll
                for (int k = 0; k < VEC; k++)
                  // (codeword k's word through the scalar offset: no lane offset per codeword held in registers)
                  if (live[k]) row_store<T, false>(b_post, lane_off, cols[NEXT] * row_bytes + k * uint32_t(sizeof(T)), lnew.v[k]);
              }
            }
            typename Rec::New out;
            if constexpr (CORR) {
              // (each magnitude on its own, fenced: see the generic step)
#pragma unroll
              for (int k = 0; k < VEC; k++) {
                asm("" : "+v"(min1[k]));
                asm("" : "+v"(min2[k]));
                min1[k] = minsum_corrected(min1[k], mc...);
                min2[k] = minsum_corrected(min2[k], mc...);
                asm("" : "+v"(min1[k]));
                asm("" : "+v"(min2[k]));
              }
            }
#pragma unroll
            for (int k = 0; k < VEC; k++) {
              const uint32_t tot = __popc(sa[k] & kSgnMask8) & 1u;
              odd_m[k] |= par_m[k];
              out.min1.v[k] = min1[k];
              out.min2.v[k] = min2[k];
              out.flip.v[k] = uint16_t(tot ? sa[k] ^ kSgnMask8 : sa[k]);
            }
            out.template store<NT>(b_rout, lane_off, cc * rec_bytes, row_bytes);
            cc = cn;
            e0 = ne0;
#pragma unroll
            for (uint32_t u = 0; u < D; u++) cols[u] = ncols[u];
          };
          for (uint32_t i = lo; i < hi; i += 2) {
            step(recA, recB, 0);
            if (i + 1 < hi) step(recB, recA, 1);
          }
        };
        if (r & 1u)
          shape_run(std::false_type{});
        else
          shape_run(std::true_type{});
        continue;
      }
    }
    // own = record of the current row, nxt = record of the row the walk reaches next (this row's peer now, `own`
    // one step later); carry_msg = the message the PREVIOUS row of the walk sent to the variable it shares with this
    // one (it had that value in hand as its own message: the previous row's record need not be kept); carry_chan = that
    // variable's channel row as the previous row loaded it: this row does not fetch it again (the second fetch, a whole
    // row step later, found it in no cache).  Both start empty with every run, in either direction.
    Rec recA, recB;
    uint32_t carry_slot = kAuxNone;  // slot of the previous row whose old message carry_msg holds
    // the variable whose channel row carry_chan holds (wave-uniform).  Matched by variable, not by slot: two degree-2
    // variables may join the same pair of rows; one is carried, the other loads.  Never a degree-1 variable or one whose
    // peer is a far row: only an edge with `prow == cn` hands anything on.
    uint32_t carry_var = kAuxNone;
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

    auto row_step = [&](Rec &own, Rec &nxt, uint32_t ph) {
      const uint32_t d = e1 - e0, cn = c + dir, cp = c - dir;
      if (!FIRST && cn < n_rows) nxt.load(b_rin, lane_off, cn * rec_bytes, row_bytes);
      Pack<T, VEC> lv[U];
#pragma unroll
      for (int u = 0; u < U; u++)
        if (uint32_t(u) < d && cols[u] != carry_var)  // (wave-uniform; the carried row: `edge` takes it from carry_chan)
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
      // F8: both in one register, the 16-bit flags word as it grows -- the signs of at most 7 edges below the running argmin
      uint32_t sa[VEC];
      constexpr uint32_t kSgnMask8 = (1u << kRecFlags8MaxRow) - 1;
      uint64_t par_m[VEC];
#pragma unroll
      for (int k = 0; k < VEC; k++) {
        min1[k] = Limits<T>::inf();
        min2[k] = Limits<T>::inf();
        arg[k] = 0;
        sgn[k] = 0;
        sa[k] = 0;
        par_m[k] = 0;
      }
      uint32_t next_carry_slot = kAuxNone;
      uint32_t next_carry_var = kAuxNone;
      // one edge: slot, variable, peer word, the loaded soft value (posterior, or channel LLR for an L-free variable);
      // `have`: `loaded` is valid also for the carried variable (the later rounds of a long row)
      auto edge = [&](uint32_t slot, uint32_t var, uint32_t peer, const Pack<T, VEC> loaded, bool have) {
        const bool lfree = !(peer & kPeerKeep);
        Pack<T, VEC> lvu = loaded;
        if (!have && var == carry_var) lvu = carry_chan[ph ^ 1u][threadIdx.x];
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
            for (int k = 0; k < VEC; k++) m_other[k] = carry_msg[ph ^ 1u][threadIdx.x].v[k];
          } else {
            Rec far;  // not a neighbour inside the run: fetch the peer's record
            far.load(b_rin, lane_off, prow * rec_bytes, row_bytes);
#pragma unroll
            for (int k = 0; k < VEC; k++) m_other[k] = far.value(pslot, k);
          }
          if constexpr (STREAM) {
#pragma unroll
            for (int k = 0; k < VEC; k++) m_other[k] = fresh[k] ? T(0.0) : m_other[k];
          }
        }
        Pack<T, VEC> lnew, sent;
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
          sent.v[k] = m_own;
          const T x = FIRST ? l : (l - m_own);
          const T a = m_abs(x);
          if constexpr (F8) {
            if (x < T(0.0)) sa[k] |= 1u << slot;
          } else {
            if (x < T(0.0)) sgn[k] |= W(1) << slot;
          }
          par_m[k] ^= __builtin_amdgcn_ballot_w64(l <= T(0.0));
          if constexpr (F8) {
            // the same fold as selects: no branch, no change of the exec mask per edge and codeword
            const bool lt1 = a < min1[k], lt2 = a < min2[k];
            min2[k] = lt1 ? min1[k] : (lt2 ? a : min2[k]);
            min1[k] = lt1 ? a : min1[k];
            sa[k] = lt1 ? ((sa[k] & kSgnMask8) | (slot << kArgShift16)) : sa[k];
          } else if (a < min1[k]) {
            min2[k] = min1[k];
            min1[k] = a;
            arg[k] = slot;
          } else if (a < min2[k]) {
            min2[k] = a;
          }
        }
        if (lfree && !FIRST && prow == cn) {
          next_carry_slot = slot;
          carry_msg[ph][threadIdx.x] = sent;
        }
        if (lfree && !single && prow == cn) {  // the next row of the walk reads the same channel row
          next_carry_var = var;
          carry_chan[ph][threadIdx.x] = lvu;
        }
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
        if (uint32_t(u) < d) edge(u, cols[u], peers[u], lv[u], false);
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
          if (i0 + u < d) {
            if (cv[u] == carry_var)
              lw[u] = carry_chan[ph ^ 1u][threadIdx.x];
            else
              lw[u] = buf_load<T, VEC, false>((pv[u] & kPeerKeep) ? b_post : b_chan, lane_off, cv[u] * row_bytes);
          }
#pragma unroll
        for (int u = 0; u < U; u++)
          if (i0 + u < d) edge(i0 + u, cv[u], pv[u], lw[u], true);
      }
      carry_slot = next_carry_slot;
      carry_var = next_carry_var;
      if (d != 0) {
        // the new record: flip[slot] = (parity of all signs) ^ (x_slot < 0)
        typename Rec::New out;
        if constexpr (CORR && F8) {
          // The byte form corrects each magnitude on its own, fenced from its neighbours: left to itself the compiler pairs the
          // eight corrections into packed f32 math, whose operands want aligned register pairs and copies of alpha and beta
          // in vector registers -- 99 VGPRs in the f32 pack-of-4 kernel without per-edge messages, where this has 91.
#pragma unroll
          for (int k = 0; k < VEC; k++) {
            asm("" : "+v"(min1[k]));
            asm("" : "+v"(min2[k]));
            min1[k] = minsum_corrected(min1[k], mc...);
            min2[k] = minsum_corrected(min2[k], mc...);
            asm("" : "+v"(min1[k]));
            asm("" : "+v"(min2[k]));
          }
        }
#pragma unroll
        for (int k = 0; k < VEC; k++) {
          const uint32_t tot =
              F8 ? __popc(sa[k] & kSgnMask8) & 1u : (sizeof(W) == 8 ? __popcll(sgn[k]) : __popc(uint32_t(sgn[k]))) & 1u;
          odd_m[k] |= par_m[k];
          if constexpr (CORR && !F8) {
            // the record holds the corrected pair, so every reader of the record (value()) sees corrected messages
            out.min1.v[k] = minsum_corrected(min1[k], mc...);
            out.min2.v[k] = minsum_corrected(min2[k], mc...);
          } else {
            out.min1.v[k] = min1[k];
            out.min2.v[k] = min2[k];
          }
          const W fl = tot ? ~sgn[k] : sgn[k];
          if constexpr (F8) {
            out.flip.v[k] = uint16_t(tot ? sa[k] ^ kSgnMask8 : sa[k]);  // (pack_flags: the word is packed already)
          } else if constexpr (RECW == 4) {
            out.flip.v[k] = fl;
            out.arg.v[k] = W(arg[k]);
          } else {
            out.flip.v[k] = Rec::pack_flags(fl, arg[k]);
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
        if constexpr (SEND) {
#pragma unroll
          for (int u = 0; u < U; u++)
            if (uint32_t(u) < d) send(u, peers[u]);
          if constexpr (LONG)
            for (uint32_t i = U; i < d; i++) send(i, edge_peer[e0 + i]);
        }
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
      row_step(recA, recB, 0);
      if (i + 1 < hi) row_step(recB, recA, 1);
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
template <int RULE, typename T, bool FIRST, bool SCRATCH = false, typename... MC>
__global__ void cn_staged_kernel(Graph g, Sched sc, State st, const T *__restrict__ L, T *__restrict__ msg,
                                 uint32_t *__restrict__ unsat_out, uint32_t dmax, T *__restrict__ scratch = nullptr,
                                 MC... mc) {
  static_assert(is_corr_pack<T, MC...> && (sizeof...(MC) == 1) == (RULE == kRuleMinsumCorr), "mc goes with kRuleMinsumCorr");
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
    const T *out = rule_check_node<RULE, T>(A, B, d, S, mc...);
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

}  // namespace dev
}  // namespace ldpc
