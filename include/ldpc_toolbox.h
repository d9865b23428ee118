/*
 * C ABI of the MI355X-native LDPC decoder library (libldpc_toolbox.so).
 *
 * PART 1 re-exports, symbol for symbol, the C API of daniestevez/ldpc-toolbox v0.12.0
 * (reference header: /root/reference/include/ldpc_toolbox.h:12-29; Rust side:
 * /root/reference/src/c_api/decoder.rs:75-137 and src/c_api/encoder.rs:55-97), so that a
 * program linked against the reference's cdylib can link against this library unchanged.
 * Decoding runs on the GPU (hand-written HIP kernels for gfx950); there is NO CPU
 * fallback: constructors return NULL (with a message on stderr / ldpc_toolbox_last_error)
 * when no HIP device is usable.
 *
 * PART 2 is the batched extension the GPU path needs (the reference decodes one codeword
 * per call).  Per codeword the semantics are exactly those of the scalar call.
 *
 * Numerical contract.  Hard decisions, iteration counts and posterior LLRs are bit-identical to
 * the reference decoder for every implementation name -- for the rules that call transcendental
 * functions (Phi, Tanh, Minstarapprox, Aminstar; /root/reference/src/decoder/arithmetic.rs:184,
 * 357, 376, 510, 965-966) this means: identical to a reference whose Rust f32/f64::{exp, ln,
 * ln_1p, tanh} resolve to the glibc libm generation with the Szabolcs-Nagy expf/logf/exp/log and
 * the fdlibm log1pf/expm1f/tanhf (and double versions) -- glibc 2.28 through 2.40, checked
 * exhaustively against 2.35.  A libm that rounds these functions correctly (the CORE-MATH
 * routines of newer glibc releases) differs from it in rare last ulps, and so would a reference
 * built there; tests/test_libm_contract.py names that situation on a host where it applies.
 * Min-sum and the 8-bit rules use no libm function and carry no such condition.
 */
#ifndef _LDPC_TOOLBOX_H
#define _LDPC_TOOLBOX_H

#ifdef __cplusplus
extern "C" {
#endif

#include <stdint.h>
#include <stddef.h>

/* ===================================================================================
 * PART 1 -- the reference's nine symbols
 * =================================================================================== */

/* Replaces ldpc_toolbox_decoder_ctor (reference include/ldpc_toolbox.h:12-13,
 * src/c_api/decoder.rs:75-88).  alist_file_path: alist text file; implementation: a decoder
 * implementation name (src/decoder/factory.rs:240-277: all 36 are accepted, plus the added
 * Minsumf32/Minsumf64/HLMinsumf32/HLMinsumf64 -- all 40 bit-identical to the reference decoder;
 * "Tanhf32@fast", "HLTanhf32@fast", "Phif32@fast", "HLPhif32@fast" are opt-in approximate variants on the
 * GPU's native exp2 / log2 / rcp, NOT bit-identical and never chosen unless named;
 * [HL]NormMinsum{f32,f64}[:alpha] and [HL]OffsetMinsum{f32,f64}[:beta] are normalized and offset min-sum: the Minsum
 * decoder, both schedules, except that the magnitude m a check row sends on an edge (the minimum of the other edges' |x|)
 * becomes alpha * m (0 < alpha <= 1, default 0.75) or max(m - beta, 0) (beta >= 0, default 0.5), in the decoder's type,
 * each result rounded once; the sign is plain min-sum's, so a magnitude clamped to zero sends +0.0 or -0.0.  The value
 * is digits[.digits] (no sign, no exponent): "NormMinsumf32", "HLOffsetMinsumf64:0.3", "NormMinsumf32:0.8125@hip:1".
 * "NormMinsumf32:1" and "OffsetMinsumf32:0" decode exactly as "Minsumf32"; there is no "@fast" form, and the 8-bit
 * forms are spelled differently:
 * [HL]Minsumi8[Norm|Offset][Jones][PartialHardLimit][Deg1Clip][:value] is 8-bit min-sum: Minstarapproxi8's quantised
 * arithmetic (8 steps per LLR unit, clip at +-127), options and schedules -- with HL only PartialHardLimit -- with the
 * check-node fold step reduced to min.  The magnitude m (0..127) becomes (a * m + 8) >> 4 with a = 16 * value in 1..16
 * (Norm, default value 0.75) or max(m - b, 0) with b = 8 * value in 0..127 (Offset, default value 0.5), both products
 * integers; the hard limit, if named, follows the correction.  A value is allowed only after Norm or Offset:
 * "Minsumi8", "Minsumi8NormJones:0.8125", "HLMinsumi8OffsetPartialHardLimit".  "Minsumi8Norm:1" and "Minsumi8Offset:0"
 * decode exactly as "Minsumi8"; "NormMinsumi8" and its like are invalid;
 * an optional "@hip:N" suffix, last, selects GPU N); puncturing: "" or a pattern such as "1,1,1,0"
 * (src/cli/ber.rs:219-229).  Returns an opaque handle, or NULL on any error. */
void *ldpc_toolbox_decoder_ctor(const char *alist_file_path, const char *implementation,
                                const char *puncturing);

/* Replaces ldpc_toolbox_decoder_ctor_alist_string (reference header :14-15,
 * src/c_api/decoder.rs:90-102): same, with the alist text passed directly. */
void *ldpc_toolbox_decoder_ctor_alist_string(const char *alist, const char *implementation,
                                             const char *puncturing);

/* Replaces ldpc_toolbox_decoder_dtor (reference header :16, src/c_api/decoder.rs:104-107). */
void ldpc_toolbox_decoder_dtor(void *decoder);

/* Replaces ldpc_toolbox_decoder_decode_f64 (reference header :17-20,
 * src/c_api/decoder.rs:109-122 -> :50-67).  llrs: llrs_len channel LLRs (the punctured
 * length when a puncturing pattern was given, else exactly n); output: receives the first
 * output_len hard decisions, one byte per bit; returns the number of iterations (0 = the
 * input was already a codeword) or -1 when max_iterations were used without reaching a
 * codeword -- output is filled in both cases.  Where the reference would panic (length
 * mismatch) or when the GPU call itself fails, this returns a value BELOW -1 (one of the
 * LDPC_TOOLBOX_ERR_* codes) and writes nothing: a caller that counts -1 as a decoding failure
 * must treat < -1 as a fault (message: ldpc_toolbox_last_error). */
#define LDPC_TOOLBOX_ERR_DEVICE (-2)      /* HIP failure */
#define LDPC_TOOLBOX_ERR_UNSUPPORTED (-3) /* graph / rule combination the kernels do not take */
#define LDPC_TOOLBOX_ERR_ARGUMENT (-4)    /* null handle, LLR or output length not matching the code */
int32_t ldpc_toolbox_decoder_decode_f64(void *decoder,
                                        uint8_t *output, size_t output_len,
                                        const double *llrs, size_t llrs_len,
                                        uint32_t max_iterations);

/* Replaces ldpc_toolbox_decoder_decode_f32 (reference header :21-24,
 * src/c_api/decoder.rs:124-137 -> :69-73). */
int32_t ldpc_toolbox_decoder_decode_f32(void *decoder,
                                        uint8_t *output, size_t output_len,
                                        const float *llrs, size_t llrs_len,
                                        uint32_t max_iterations);

/* Replace ldpc_toolbox_encoder_{ctor,ctor_alist_string,dtor,encode} (reference header
 * :26-32, src/c_api/encoder.rs:55-97).  Host-side systematic encoder (+ puncturer).
 * encode: input = k message bytes (value 1 = one, anything else = zero), output =
 * the (punctured) codeword, one byte per bit; output_len must equal its length. */
void *ldpc_toolbox_encoder_ctor(const char *alist_file_path, const char *puncturing);
void *ldpc_toolbox_encoder_ctor_alist_string(const char *alist, const char *puncturing);
void ldpc_toolbox_encoder_dtor(void *encoder);
void ldpc_toolbox_encoder_encode(void *encoder,
                                 uint8_t *output, size_t output_len,
                                 const uint8_t *input, size_t input_len);

/* ===================================================================================
 * PART 2 -- batched extension (new symbols, same handles)
 * =================================================================================== */

/* Constructor with an explicit GPU index (the "@hip:N" suffix does the same). */
void *ldpc_toolbox_decoder_ctor_alist_string_on_device(const char *alist, const char *implementation,
                                                       const char *puncturing, int32_t device);

/* Batch decode, host buffers.  Semantically a loop of ldpc_toolbox_decoder_decode_f32 over
 * `batch` frames (replaces that loop: src/simulation/ber.rs:462-466 calls decode once per
 * frame):
 *   llrs        [batch][llrs_len]   one row per frame
 *   output      [batch][output_len] first output_len hard decisions of every frame
 *   iterations  [batch]             iterations used, -1 = failed (may be NULL)
 *   posterior   [batch][n]          final soft LLRs of the decoder (may be NULL)
 * returns 0, or one of the LDPC_TOOLBOX_ERR_* codes above -- the same vocabulary as the scalar entries (bad
 * handle / lengths: LDPC_TOOLBOX_ERR_ARGUMENT, HIP failure: _DEVICE, unsupported graph / rule: _UNSUPPORTED). */
int32_t ldpc_toolbox_decoder_decode_batch_f32(void *decoder, uint8_t *output, size_t output_len,
                                              const float *llrs, size_t llrs_len, size_t batch,
                                              uint32_t max_iterations, int32_t *iterations,
                                              float *posterior);
int32_t ldpc_toolbox_decoder_decode_batch_f64(void *decoder, uint8_t *output, size_t output_len,
                                              const double *llrs, size_t llrs_len, size_t batch,
                                              uint32_t max_iterations, int32_t *iterations,
                                              double *posterior);

/* Batch decode, buffers already resident in the decoder's GPU memory (all four pointers are
 * device pointers).  hip_stream: a hipStream_t to launch on (the call returns without
 * synchronising; the caller orders it after the producers of llrs), or NULL: the library uses the
 * handle's own stream, ordered after everything queued on the legacy default stream (handle 0) at
 * the time of the call, and synchronises before returning.  NULL is also what a framework's
 * "default stream" handle looks like (torch.cuda.default_stream().cuda_stream == 0): pass a real
 * stream to get the asynchronous form.  (Returning without synchronising is not returning at once: a call returns when
 * its last launch is enqueued, and a layered-schedule call large enough for two execution lanes enqueues from two
 * threads that follow their groups' progress one iteration behind, so it returns shortly before its work completes.) */
int32_t ldpc_toolbox_decoder_decode_batch_f32_device(void *decoder, uint8_t *output, size_t output_len,
                                                     const float *llrs, size_t llrs_len, size_t batch,
                                                     uint32_t max_iterations, int32_t *iterations,
                                                     float *posterior, void *hip_stream);
int32_t ldpc_toolbox_decoder_decode_batch_f64_device(void *decoder, uint8_t *output, size_t output_len,
                                                     const double *llrs, size_t llrs_len, size_t batch,
                                                     uint32_t max_iterations, int32_t *iterations,
                                                     double *posterior, void *hip_stream);

/* Batched encoder on the GPU (the transmit side of the batched decode entries).  Same handle as the scalar encoder: a
 * handle from ldpc_toolbox_encoder_ctor / ..._ctor_alist_string needs no GPU until its first batched call, which builds
 * the device tables on the GPU LDPC_TOOLBOX_DEVICE names (default 0); the constructor below builds them at once on GPU
 * `device` and returns NULL when it cannot (no GPU, bad alist or pattern; message: ldpc_toolbox_last_error). */
void *ldpc_toolbox_encoder_ctor_alist_string_on_device(const char *alist, const char *puncturing, int32_t device);

/* A loop of ldpc_toolbox_encoder_encode over `batch` messages, run on the GPU -- byte for byte the same codewords.
 *   input  [batch][input_len]   input_len == k; a byte equal to 1 is a one, anything else a zero
 *   output [batch][output_len]  output_len == n, or the punctured length when a pattern was given; bytes 0/1
 * Host pointers (pageable is fine).  returns 0 or an LDPC_TOOLBOX_ERR_* code: a null handle, a length that does not
 * match the code or a pattern that does not divide n: _ARGUMENT, found before the GPU is touched; no usable GPU or a HIP
 * failure: _DEVICE (message: ldpc_toolbox_last_error) -- there is no CPU fallback.  On an error nothing is written.
 * batch == 0 returns 0.  One batched call at a time per handle (the work buffers belong to the handle). */
int32_t ldpc_toolbox_encoder_encode_batch(void *encoder, uint8_t *output, size_t output_len,
                                          const uint8_t *input, size_t input_len, size_t batch);

/* The same on buffers resident in the encoder's GPU memory (both are device pointers, and they do not overlap).
 * hip_stream: as for the ..._decode_batch_*_device entries -- a hipStream_t: enqueue and return (the caller orders the
 * call after the producers of `input`); NULL: the handle's own stream, ordered after everything queued on the legacy
 * default stream at the time of the call, and synchronised before returning.  The work buffers belong to the handle:
 * calls on one handle on different streams are to be ordered by the caller. */
int32_t ldpc_toolbox_encoder_encode_batch_device(void *encoder, uint8_t *output, size_t output_len,
                                                 const uint8_t *input, size_t input_len, size_t batch,
                                                 void *hip_stream);

/* Integer properties of an encoder: "k", "n", "output_len" (n, or the punctured length), "staircase" (1: the
 * accumulator encoder of the DVB-S2 family, 0: the dense generator), "staircase_form" (how the batched entries encode
 * a staircase code, a function of k alone that needs no device: 0 = 32 frames per word staged in LDS, 1 = 16 frames
 * per word staged in LDS, 2 = gathered from global memory; -1 for every other code), "device" (GPU of the batched
 * entries; -1 while no device state exists).  returns 0 or -1 (unknown key). */
int32_t ldpc_toolbox_encoder_get(void *encoder, const char *key, int64_t *value);

/* The syndrome test of the reference's decoders (src/decoder.rs:157-164, check_llrs: the parity
 * of the hard decisions over every row of H) as an operator that returns the parities instead of
 * only "all zero?".  bits: [batch][bits_len] hard decisions, one byte per bit (what the decode
 * entries write with output_len = n); bits_len must equal n.  syndrome: [batch][m], 1 = check
 * unsatisfied (may be NULL).  weight: [batch] number of unsatisfied checks (may be NULL).  A frame
 * the decoder reported as converged (iterations >= 0) has weight 0; a failed one does not.
 * Host pointers; the _device form takes device pointers and a hipStream_t (NULL = the handle's own
 * stream, synchronised on return), at most 65535 codewords per call.  returns 0 or an LDPC_TOOLBOX_ERR_* code. */
int32_t ldpc_toolbox_decoder_syndrome(void *decoder, const uint8_t *bits, size_t bits_len, size_t batch,
                                      uint8_t *syndrome, uint32_t *weight);
int32_t ldpc_toolbox_decoder_syndrome_device(void *decoder, const uint8_t *bits, size_t bits_len, size_t batch,
                                             uint8_t *syndrome, uint32_t *weight, void *hip_stream);

/* Integer properties: "n", "m", "k", "edges", "input_len", "device", "group_size",
 * "max_check_degree", "max_variable_degree", "layers" (dependency levels of the layered schedule),
 * "last_lanes" / "last_group" (execution lanes and codewords per group of the last decode call),
 * "preferred_group" (codewords per group of a large call: "group_size" if set, else 4096, more for small graphs),
 * "row_records" (words per check-row record when flooding min-sum keeps a row's messages as
 * {min1, min2, flip bits, argmin}; 0 = per-edge messages), "record_flag_bits" (read-only: bits of the word that holds a
 * record's flip bits and argmin in memory -- 16 where every row has at most 12 edges, then kept in an array of its own
 * beside the two magnitudes, else 32 or 64, the decoder's own word; 0 without records.  "row_records" stays the record
 * family, 3 or 4, whatever the width), "last_vn_records" (1: the last decode call's variable-node launches read the row
 * records, the "vn_records" form; 0: per-edge messages), "last_vn_bundles" (1: those launches walked the kept variables in
 * bundles, the "vn_bundles" order), "vn_bundle_saved_permille" (what that order spares in the last decode call: thousandths
 * of the variable-node launch's record fetches that coincide inside a workgroup's step; 0 when off), "last_vn_chains" (1:
 * they walked that order in chains, "vn_chains": a record two consecutive entries of a wave share stays in its registers),
 * "vn_chain_saved_permille" (thousandths of the record fetches the chained walk does not issue; 0 when off), "flags8" (the tunable
 * below, as set), "cn_row_shape" (the tunable below, as set), "last_cn_row_shape" (1: the last decode call's check-node
 * launches behind the first iteration took the row-shape form -- a straight-line row step in the runs of the walk whose rows
 * all have the graph's dominant shape), "cn_row_shape_runs" / "cn_row_shape_rows" (the runs of the walk that conformed at that
 * call's "rec_run", and the check rows in them; 0 when the form did not run), "last_record_flag_bytes"
 * (bytes of a record's flags word in memory in the last decode call: 1 with "flags8" on rows of at most 7 edges, else 2, 4
 * or 8 = "record_flag_bits" / 8; 0: that call kept no flooding row records), "call_edges" (the tunable below, as set),
 * "last_call_edges" (read-only bit mask: which of that tunable's shortcuts the last decode call took -- 1: the ingest launch
 * stored the input once, with no copy in the posterior array; 2: the last hard-decision pack covered the rows the
 * variable-node launch writes and the closing launch packed the other variables' decisions without storing their
 * posteriors; 4: the final output launch read the packed decisions instead of posterior rows; 8: a re-packing checkpoint was
 * enqueued as two launches behind its plan instead of four; 1, 2 and 4 only on the flooding row-record path of a call that
 * asks for no posterior), "minsum_correction" (0: none, 1: normalized min-sum,
 * 2: offset min-sum), "minsum_correction_int" (the 8-bit min-sum names: the integer the kernels use, 16 * alpha or
 * 8 * beta; 0 for every other name).  returns 0 or -1 (unknown key). */
int32_t ldpc_toolbox_decoder_get(void *decoder, const char *key, int64_t *value);
/* Tunables: "group_size" (codewords decoded together; 0 = automatic), "profiling" (0/1:
 * bracket the check/variable/layer launches with hipEvents), and 33 launch / execution choices -- "waves", "vec", "tile",
 * "lfree", "records", "rec_run", "rec_quiet", "rec_long", "call_edges" (0/1, default 1: the launches around a call's iterations trimmed to what
 * its result needs, see "last_call_edges" above; 0: as they were), "vn_event", "vn_records", "vn_bundles", "vn_chains", "vn_chain_len", "flags8", "cn_row_shape", "staged_minsum", "cn_reg", "hl_reg", "hl_records",
 * "serial_levels", "latency", "latency_edge", "compact", "compact_first", "compact_every", "lanes", "lane_threads",
 * "lane_pace", "lead", "poll", "throttle", "pooling" (ldpc_toolbox_amd/csrc/device_decoder.h says what each selects; results never
 * depend on them: each chooses between forms the test suite compares bit for bit).  "throttle" (0/1, default 0):
 * a ..._device call on the CALLER's stream may pace its launches on the groups' progress words, i.e. return when the
 * work is within two iterations of its end instead of as soon as it is enqueued (fewer launches past convergence;
 * calls on the library's own stream always may).  The same switch governs the layered schedule's lane threads ("lane_pace",
 * one iteration ahead of their group): without it a call on the caller's stream returns as soon as everything is
 * enqueued.  A paced call that sees no progress for 200 ms (a stream gated behind something the caller releases later)
 * stops pacing and enqueues the rest at once.  Flooding schedule (round 5): a ..._device call with "throttle" (or on the library's
 * own stream) follows its groups two iterations ahead -- with two execution lanes through a host thread per lane -- and, once the first codewords have converged, ends every iteration with a re-packing
 * checkpoint instead of every second one (DVB-S2 1/2 at +2 dB: +2 %; a call in which nothing converges launches nothing
 * extra).
 * "pooling" (0/1, default 0): straggler pooling inside the batch entries.  A call of several chunks of frames learns from
 * its first chunk how many iterations its frames take; later chunks run a reduced iteration budget (2 x average + 8) and the
 * frames that have not converged by then are decoded again, together, with max_iterations -- per frame the outcome of one
 * full-budget decode, so outputs do not depend on the option.  It spares every chunk the nearly empty iterations its few slow
 * or failing frames would drag it through (the waterfall with the reference's default of 100 iterations).  The call
 * synchronises between chunks: host-buffer entries always may; a ..._device entry takes it on the library's own stream or
 * with "throttle".  ldpc_toolbox_decoder_get "last_pooled": frames of the last call that took the second pass.
 * returns 0 or -1. */
int32_t ldpc_toolbox_decoder_set(void *decoder, const char *key, int64_t value);
/* hipEvent statistics collected while "profiling" is 1.  kind: 0 = check-node kernel,
 * 1 = variable-node phase (vn_kernel and, with row records, the small vn_free_rec_kernel launch behind it: one bracket
 * per iteration), 2 = layered level kernel.  reset != 0 clears the counters
 * after reading. */
int32_t ldpc_toolbox_decoder_kernel_stats(void *decoder, int32_t kind, uint64_t *launches,
                                          double *total_ms, int32_t reset);

/* ===================================================================================
 * PART 3 -- GPU-resident simulation step (the frame pipeline either side of the decode path:
 * reference src/simulation/ber.rs:436-481 Worker::simulate, one frame per call there)
 * =================================================================================== */

/* Decoder + host encoder + a pool of `pool_size` pre-encoded random messages (seeded by
 * pool_seed) on GPU `device`.  BPSK over AWGN.  NULL on error. */
void *ldpc_toolbox_sim_ctor(const char *alist, const char *implementation, const char *puncturing,
                            int32_t device, uint32_t pool_size, uint64_t pool_seed);
void ldpc_toolbox_sim_dtor(void *sim);
/* Generates frames [first_frame, first_frame + frames) at ebn0_db on the device (noise is a pure
 * function of (seed, frame index, position): Philox4x32-10 + polar method), decodes them and counts
 * errors.  counters[6] = frames, bit errors (first k bits), frame errors, false decodes, total
 * iterations, iterations of the correct frames (the fields of ber.rs:113-138).  returns 0 or < 0. */
int32_t ldpc_toolbox_sim_run(void *sim, double ebn0_db, uint64_t seed, uint64_t first_frame,
                             size_t frames, uint32_t max_iterations, uint64_t *counters);
/* The same with the reference driver's outer-BCH accounting (src/simulation/ber.rs:328-337,
 * `ber --bch-max-errors`): a frame with at most bch_max_errors bit errors after LDPC decoding counts
 * as corrected.  counters[9] = the six above, then BCH bit errors, BCH frame errors, iterations of
 * the frames the BCH code corrects. */
int32_t ldpc_toolbox_sim_run_bch(void *sim, double ebn0_db, uint64_t seed, uint64_t first_frame,
                                 size_t frames, uint32_t max_iterations, uint64_t bch_max_errors,
                                 uint64_t *counters);
/* The LLRs of the same frames ([frames][n_tx]; a host buffer, or a buffer in the simulator's GPU memory, which is then
 * filled in place) and which pooled codeword each frame carries (host array, may be NULL): lets a CPU decoder be run on
 * identical frames, and a benchmark fill its device-resident batch from the library's own generator. */
int32_t ldpc_toolbox_sim_generate(void *sim, double ebn0_db, uint64_t seed, uint64_t first_frame,
                                  size_t frames, float *llrs, uint32_t *pool_index);
/* The pool: messages [pool][k] and transmitted (punctured) codewords [pool][n_tx]; either may be NULL. */
int32_t ldpc_toolbox_sim_pool(void *sim, uint8_t *messages, uint8_t *tx_bits);
/* "k", "n", "n_tx", "pool", "modulation" (bits per symbol of what generates the frames: of the constellation while one
 * is set), "interleaving", "constellation" (read-only, 0/1: ldpc_toolbox_sim_set_constellation is in force), "max_log"
 * (read-only, 0/1: its fold step); "preferred_batch" (frames per run call that fill one
 * group of the decoder: 4096, more for small graphs); of the last run call: "pooled_frames" (frames that went
 * through the straggler pool, below); "streamed_frames" and "stream_iterations" are accepted and read 0.
 * returns 0 or -1. */
int32_t ldpc_toolbox_sim_get(void *sim, const char *key, int64_t *value);
/* "modulation": bits per symbol, 1 = BPSK (default), 3 = 8PSK with the DVB-S2 Gray mapping and the
 * exact max* demodulator (src/simulation/modulation.rs:144-288; n_tx must be a multiple of 3).
 * "interleaving": columns of the DVB-S2 bit interleaver applied before modulation and undone after
 * demodulation (src/simulation/interleaving.rs; negative = rows read backwards, 0 = none (default);
 * must divide n_tx), as the reference's `ber --modulation 8PSK --interleaving N` (src/cli/ber.rs:52-59).
 * "pooling" (0/1, default 1): once a run call has seen how many iterations its frames take, its later chunks run a
 * reduced iteration budget and the frames that have not converged by then are pooled and decoded together with the
 * full budget -- per frame the result of one full-budget decode, so the counters do not depend on it; it spares every
 * chunk the nearly empty iterations its few slow frames would otherwise drag it through.
 * "streaming" is accepted and has no effect (continuous batching measured slower than drained chunks and was removed).
 * Any other key is forwarded to the simulator's decoder (see ldpc_toolbox_decoder_set).
 * returns 0, or -1 (unknown key / unusable value, message via ldpc_toolbox_last_error). */
int32_t ldpc_toolbox_sim_set(void *sim, const char *key, int64_t value);
/* Any constellation of PART 4 as the simulator's modulation.  demod: a handle of ldpc_toolbox_demod_ctor[_table]; its
 * constellation is copied, the handle may be destroyed afterwards.  NULL returns to what the "modulation" key selects
 * (which ldpc_toolbox_sim_set keeps recording while a constellation is in force).  A "BPSK" handle selects the BPSK
 * generator of "modulation" = 1.  Any other: n_tx must be a multiple of bits_per_symbol, and the table's mean energy
 * sum_V |p_V|^2 / 2^m must lie within 1e-6 of 1 -- noise_sigma stays sqrt(0.5 / (rate * m * EbN0))
 * (src/simulation/ber.rs:299-302), which presumes unit symbol energy; a table of another energy is refused rather than
 * simulated on a shifted Eb/N0 axis.  max_log != 0: the demapper's max-log fold step instead of max*.
 * DEFINED RESULT: for either fold step the LLRs of frame f are what ldpc_toolbox_mod_run_f64 (the frame's pooled
 * codeword, the simulator's "interleaving"), then ldpc_toolbox_awgn_run_f64 (the run's seed, frame f, noise_sigma),
 * then ldpc_toolbox_demod_run_f64 (the same noise_sigma, interleaving and max_log; the handle's energy term) give, each
 * value rounded once to float.  With the "8PSK" handle and max_log = 0 that is bit for bit what "modulation" = 3
 * produces.  One fused kernel computes it, one thread per symbol; the symbols are never stored.
 * Resets the straggler-pooling budget, as "modulation" does.  returns 0, or -1 with a message and nothing changed. */
int32_t ldpc_toolbox_sim_set_constellation(void *sim, void *demod, int32_t max_log);

/* ===================================================================================
 * PART 4 -- batched soft demapper, modulator and AWGN channel on the GPU (reference: trait Demodulator,
 * src/simulation/modulation.rs:109-281, and the LLR deinterleaver, src/simulation/interleaving.rs:65-86; trait Modulator,
 * modulation.rs:40-62 with the bit interleaver, interleaving.rs:40-58; AwgnChannel::add_noise, src/simulation/channel.rs:60-81;
 * one frame per call there)
 * =================================================================================== */

/* A demodulator handle turns [batch][symbols_len] received symbols into [batch][llrs_len] channel LLRs in codeword
 * order (deinterleaved): exactly the `llrs` of ldpc_toolbox_decoder_decode_batch_f32_device / _f64_device, so the two
 * calls chain on one stream without a host round trip.  A positive LLR means bit 0.
 *
 * modulation: "BPSK" (real symbols, llr = -2 / sigma^2 * x), "QPSK" or "8PSK" (the DVB-S2 mappings; symbols are
 * (re, im) pairs).  The _table constructor takes any constellation of m = bits_per_symbol (1..5) bits: 2^m (re, im)
 * doubles, point p_V at index V = sum_j b_j << (m-1-j) (b0, the first bit of the symbol, most significant).
 * With scale = 1 / sigma^2:   d_V = (re * scale) * p_V.re + (im * scale) * p_V.im   [ - (0.5 * scale) * |p_V|^2
 * when energy_term != 0: needed for points of unequal energy ],
 *   llr_j = F({d_V : bit j of V = 0}) - F({d_V : bit j of V = 1}),  F a left fold over ascending V with the step
 *   max*(a, b) = max(a, b) + log1p(exp(-|a - b|))  (exact; with "8PSK" the reference's Psk8Demodulator bit for bit), or
 *   max(a, b) with a NaN operand ignored, -0 < +0  (max_log != 0: IEEE 754-2019 maximumNumber).
 * The constructors need no GPU (`device` is used by the first run; -1 = LDPC_TOOLBOX_DEVICE, default 0).  NULL for an
 * unknown name, bits_per_symbol outside 1..5, or a point that is not finite (message via ldpc_toolbox_last_error). */
void *ldpc_toolbox_demod_ctor(const char *modulation, int32_t device);
void *ldpc_toolbox_demod_ctor_table(const double *points_re_im, uint32_t bits_per_symbol, int32_t energy_term,
                                    int32_t device);
void ldpc_toolbox_demod_dtor(void *demod);
/* symbols [batch][symbols_len] -- (re, im) pairs, reals for "BPSK" -- to llrs [batch][llrs_len], host pointers, staged
 * through device buffers of the handle.  _f64: all arithmetic in double.  _f32: exact = symbols widened to double, the
 * double arithmetic, each LLR rounded once; max_log = the same formulas in float throughout.
 * interleaving: signed columns of the DVB-S2 bit interleaver as in ldpc_toolbox_sim_set (0 = none, negative = rows read
 * backwards); the LLR of interleaved position i = m * symbol + j is written to its codeword position.
 * llrs_len must be bits_per_symbol * symbols_len and a multiple of |interleaving|, noise_sigma finite and > 0: else
 * LDPC_TOOLBOX_ERR_ARGUMENT, before the GPU is touched and with nothing written.  Without a GPU: LDPC_TOOLBOX_ERR_DEVICE
 * (there is no CPU path).  batch == 0 returns 0.  One call at a time per handle.  returns 0 or an LDPC_TOOLBOX_ERR_* code. */
int32_t ldpc_toolbox_demod_run_f32(void *demod, float *llrs, size_t llrs_len, const float *symbols, size_t symbols_len,
                                   size_t batch, double noise_sigma, int32_t interleaving, int32_t max_log);
int32_t ldpc_toolbox_demod_run_f64(void *demod, double *llrs, size_t llrs_len, const double *symbols, size_t symbols_len,
                                   size_t batch, double noise_sigma, int32_t interleaving, int32_t max_log);
/* The same on device pointers.  hip_stream as in the decode entries: a stream = enqueue and return; NULL = the handle's
 * own stream, ordered after what the legacy default stream holds at the call, synchronised on return. */
int32_t ldpc_toolbox_demod_run_f32_device(void *demod, float *llrs, size_t llrs_len, const float *symbols,
                                          size_t symbols_len, size_t batch, double noise_sigma, int32_t interleaving,
                                          int32_t max_log, void *hip_stream);
int32_t ldpc_toolbox_demod_run_f64_device(void *demod, double *llrs, size_t llrs_len, const double *symbols,
                                          size_t symbols_len, size_t batch, double noise_sigma, int32_t interleaving,
                                          int32_t max_log, void *hip_stream);
/* The handle is a constellation: it maps as well as demaps.  bits [batch][bits_len], one byte per bit with the encoder's
 * convention (a byte equal to 1 is a one, anything else a zero) -> symbols [batch][symbols_len], (re, im) pairs.
 * Interleaved position i = m * symbol + j carries the bit of codeword position
 * deinterleaved_position(i) = c * rows + r, with columns = |interleaving|, rows = bits_len / columns, r = i / columns,
 * c' = i % columns, c = interleaving < 0 ? columns - 1 - c' : c'  (i itself for interleaving == 0): the bit interleaver of
 * src/simulation/interleaving.rs:40-58, the inverse of what ldpc_toolbox_demod_run_* undoes.  V = sum_j b_j << (m-1-j),
 * and the symbol is (p_V.re, p_V.im): the handle's doubles for _f64, each rounded once to float for _f32.  A "BPSK"
 * handle writes reals: +1 for a one, -1 for a zero (modulation.rs:87-95).
 * A null handle, bits_len != bits_per_symbol * symbols_len, bits_len > 0x7fffffff or |interleaving| not dividing bits_len:
 * LDPC_TOOLBOX_ERR_ARGUMENT before the GPU is touched, nothing written.  Without a GPU LDPC_TOOLBOX_ERR_DEVICE; batch == 0
 * returns 0.  Host pointers (staged through the handle's buffers) or, _device, device pointers and a hipStream_t as in
 * ldpc_toolbox_demod_run_*_device.  returns 0 or an LDPC_TOOLBOX_ERR_* code. */
int32_t ldpc_toolbox_mod_run_f32(void *demod, float *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len,
                                 size_t batch, int32_t interleaving);
int32_t ldpc_toolbox_mod_run_f64(void *demod, double *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len,
                                 size_t batch, int32_t interleaving);
int32_t ldpc_toolbox_mod_run_f32_device(void *demod, float *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len,
                                        size_t batch, int32_t interleaving, void *hip_stream);
int32_t ldpc_toolbox_mod_run_f64_device(void *demod, double *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len,
                                        size_t batch, int32_t interleaving, void *hip_stream);
/* AWGN in place on symbols [batch][symbols_len] (src/simulation/channel.rs:60-81); row r is frame first_frame + r.  The
 * noise is the simulator's: Philox4x32-10 with key (seed low word, seed high word) and counter (attempt, pair, frame low
 * word, frame high word), and the polar method in float over the block's two candidate points (v = (w >> 8) * 2^-23 - 1;
 * the first with 0 < s = v1^2 + v2^2 < 1 gives f = sqrt(-2 * logf(s) / s), z0 = v1 * f, z1 = v2 * f; else the next attempt).
 * Complex handles: symbol s uses pair s, re += sigma * z0, im += sigma * z1.  "BPSK" handle (real symbols): position j
 * uses pair j / 2, z0 for even j, z1 for odd j -- the simulator's BPSK keying.  _f64: x + sigma * (double)z.
 * _f32: x + (float)sigma * z.  Each product and each sum is rounded once.
 * noise_sigma must be finite and >= 0 (channel.rs:52-53) and symbols_len <= 0x7fffffff, else LDPC_TOOLBOX_ERR_ARGUMENT with
 * nothing written.  Other behaviour as ldpc_toolbox_mod_run_*. */
int32_t ldpc_toolbox_awgn_run_f32(void *demod, float *symbols, size_t symbols_len, size_t batch, double noise_sigma,
                                  uint64_t seed, uint64_t first_frame);
int32_t ldpc_toolbox_awgn_run_f64(void *demod, double *symbols, size_t symbols_len, size_t batch, double noise_sigma,
                                  uint64_t seed, uint64_t first_frame);
int32_t ldpc_toolbox_awgn_run_f32_device(void *demod, float *symbols, size_t symbols_len, size_t batch, double noise_sigma,
                                         uint64_t seed, uint64_t first_frame, void *hip_stream);
int32_t ldpc_toolbox_awgn_run_f64_device(void *demod, double *symbols, size_t symbols_len, size_t batch, double noise_sigma,
                                         uint64_t seed, uint64_t first_frame, void *hip_stream);
/* Rayleigh block fading with perfect CSI behind a one-tap equaliser, in place on symbols [batch][symbols_len], writing scale
 * [batch][symbols_len]: what ldpc_toolbox_nr_demap_csi_* (PART 10) takes.  Row r is frame first_frame + r.  The received
 * h x + sigma z, divided by h, is x + sigma z / h; the phase of h does not change the law of z / h, so only a = |h| is drawn.
 * Per frame f and symbol s, with q = s / block:
 *   (w0, w1) = the normal pair above with key seed ^ 0x9E3779B97F4A7C15, frame f, pair q: one gain per `block` consecutive
 *     symbols of a frame, from another stream than the noise's; block >= symbols_len is quasi-static fading;
 *   gf = 0.5f * (w0 * w0 + w1 * w1), af = sqrtf(gf), in float, each operation rounded once (af > 0: w0^2 + w1^2 = -2 ln s
 *     with 0 < s < 1; the mean of af^2 is 1, so noise_sigma keeps its meaning as the average Eb/N0);
 *   sigma_e = noise_sigma / (double)af, scale_s = 1.0 / (sigma_e * sigma_e), in double, each operation rounded once (no f64
 *     square root);
 *   (z0, z1) = the AWGN channel's pair: key seed, frame f, pair s.
 *   _f64: re += sigma_e * (double)z0, im += sigma_e * (double)z1, scale[s] = scale_s.
 *   _f32: re += (float)sigma_e * z0, im += (float)sigma_e * z1, scale[s] = (float)scale_s.
 * Complex handles only: a "BPSK" handle, noise_sigma not finite or not > 0, block == 0, symbols_len > 0x7fffffff, a null
 * handle or buffer: LDPC_TOOLBOX_ERR_ARGUMENT before the GPU is touched, nothing written.  A device symbol buffer is aligned
 * to one (re, im) pair, a device scale buffer to its element.  Other behaviour as ldpc_toolbox_awgn_run_*. */
int32_t ldpc_toolbox_fading_run_f32(void *demod, float *symbols, float *scale, size_t symbols_len, size_t batch, double noise_sigma,
                                    uint32_t block, uint64_t seed, uint64_t first_frame);
int32_t ldpc_toolbox_fading_run_f64(void *demod, double *symbols, double *scale, size_t symbols_len, size_t batch, double noise_sigma,
                                    uint32_t block, uint64_t seed, uint64_t first_frame);
int32_t ldpc_toolbox_fading_run_f32_device(void *demod, float *symbols, float *scale, size_t symbols_len, size_t batch,
                                           double noise_sigma, uint32_t block, uint64_t seed, uint64_t first_frame, void *hip_stream);
int32_t ldpc_toolbox_fading_run_f64_device(void *demod, double *symbols, double *scale, size_t symbols_len, size_t batch,
                                           double noise_sigma, uint32_t block, uint64_t seed, uint64_t first_frame, void *hip_stream);
/* key: "bits_per_symbol", "points", "energy_term", "device" (-1 until the first run made the device state).
 * returns 0, or -1 for an unknown key. */
int32_t ldpc_toolbox_demod_get(void *demod, const char *key, int64_t *value);

/* ===================================================================================
 * PART 5 -- batched BCH outer code on the GPU: the DVB-S2 outer code (EN 302 307-1 5.3.1) and any narrow-sense binary
 * BCH code over GF(2^4)..GF(2^16).  The reference has no BCH code; its simulation counts "a frame with at most
 * bch_max_errors bit errors" as corrected (src/simulation/ber.rs:328-337).
 * =================================================================================== */

/* spec: "dvbs2:NAME" with the names of ldpc_toolbox_code_alist ("R1_2", "R8_9short", ...): (n, k, t) of the standard,
 * GF(2^16) with P = 1 + x^2 + x^3 + x^5 + x^16 for normal frames, GF(2^14) with P = 1 + x + x^3 + x^5 + x^14 for short
 * ones -- or "bch:M:P:T:N": GF(2^M) built from the primitive polynomial P (hex, bit i = coefficient of x^i, alpha = x),
 * T errors corrected, shortened length N.  g(x) = lcm of the minimal polynomials of alpha^1, alpha^3, ..., alpha^(2T-1),
 * derived from P; parity = deg g, k = n - parity.
 * NULL (message via ldpc_toolbox_last_error) for an unknown name, M outside 4..16, a P of another degree or not primitive,
 * T < 1, 2T >= 2^M - 1, T > 12, N > 2^M - 1 or N - deg g < 1.
 * n is the LDPC code's k, so the handles chain -- except for "dvbs2:R3_4short": the library's LDPC code of that name
 * follows the reference's m() and has k = 1080, the BCH handle follows the standard (n = 11880); the length checks of
 * the entries refuse that chain by themselves.
 * The constructor needs no GPU (`device` is used by the first batched call; -1 = LDPC_TOOLBOX_DEVICE, default 0). */
void *ldpc_toolbox_bch_ctor(const char *spec, int32_t device);
void ldpc_toolbox_bch_dtor(void *bch);
/* key: "n", "k", "t", "m", "parity", "primitive" (P), "pass_frames" (frames per pass of a batched call),
 * "stage_frames" (frames a host entry stages on the device at a time), "device" (-1
 * until the first batched call made the device state).  returns 0, or -1 for an unknown key. */
int32_t ldpc_toolbox_bch_get(void *bch, const char *key, int64_t *value);
/* g_0 .. g_parity, one byte each, when len >= parity + 1; returns parity + 1. */
size_t ldpc_toolbox_bch_generator(void *bch, uint8_t *coefficients, size_t len);
/* Bytes hold one bit each; on input a byte equal to 1 is a one and anything else a zero (the encoder's convention),
 * outputs are 0 or 1.  Byte i of a row of length n is the coefficient of x^(n-1-i): the first message bit is the highest
 * power.  input [batch][k] -> output [batch][n], c(x) = x^parity m(x) + (x^parity m(x) mod g(x)): the first k bytes are
 * the normalised message, the last `parity` the remainder -- exactly the `input` of
 * ldpc_toolbox_encoder_encode_batch_device.
 * input_len != k, output_len != n or a null handle: LDPC_TOOLBOX_ERR_ARGUMENT before the GPU is touched, nothing written.
 * Without a GPU LDPC_TOOLBOX_ERR_DEVICE (there is no CPU path).  batch == 0 returns 0; batch is otherwise unlimited.
 * Input and output do not overlap.  One call at a time per handle.  Host pointers (staged through the handle's buffers)
 * or, _device, device pointers and a hipStream_t: a stream = enqueue and return; NULL = the handle's own stream, ordered
 * after what the legacy default stream holds at the call, synchronised on return.  The decoder's list, count and
 * syndrome buffers belong to the handle: calls on one handle on different streams are to be ordered by the caller. */
int32_t ldpc_toolbox_bch_encode_batch(void *bch, uint8_t *output, size_t output_len, const uint8_t *input, size_t input_len,
                                      size_t batch);
int32_t ldpc_toolbox_bch_encode_batch_device(void *bch, uint8_t *output, size_t output_len, const uint8_t *input,
                                             size_t input_len, size_t batch, void *hip_stream);
/* Bounded-distance decoder.  input [batch][n] (the LDPC decode entries' `output` with output_len = k_ldpc) -> output
 * [batch][output_len], output_len = k (the message) or n (the whole word); errors [batch] may be NULL.
 * If a codeword c within Hamming distance t of the input exists (it is unique), the output is c (its first output_len
 * bytes) and errors = the distance, corrected parity bits included.  Otherwise the output is the normalised input
 * unchanged and errors = -1.  Other behaviour as ldpc_toolbox_bch_encode_batch. */
int32_t ldpc_toolbox_bch_decode_batch(void *bch, uint8_t *output, size_t output_len, const uint8_t *input, size_t input_len,
                                      size_t batch, int32_t *errors);
int32_t ldpc_toolbox_bch_decode_batch_device(void *bch, uint8_t *output, size_t output_len, const uint8_t *input,
                                             size_t input_len, size_t batch, int32_t *errors, void *hip_stream);
/* The simulator's option to run the real code instead of the genie of ldpc_toolbox_sim_run_bch.  The code is copied
 * (the handle may be destroyed afterwards); returns -1 with a message and changes nothing unless the code's n equals the
 * simulator's k -- which also refuses "dvbs2:R3_4short" on the library's LDPC code of that name.  NULL returns to the
 * genie.  Resets the straggler-pooling budget, as "modulation" does.  "bch" of ldpc_toolbox_sim_get is 1 while a code is set.
 * With a code set, ldpc_toolbox_sim_run_bch requires bch_max_errors == t (else LDPC_TOOLBOX_ERR_ARGUMENT); counters 0..5
 * are what they are without it, and counters 6..8 come from the real decoder.  Per frame: e = the XOR of the frame's k
 * hard decisions with its pooled message; the bounded-distance decoder runs on e -- by linearity that is the outcome for
 * EVERY transmitted BCH codeword, so the pool's messages are not BCH codewords and need not be; residual = the weight of
 * the first k_bch bits of the decoder's output; [6] += residual, [7] += (residual > 0), [8] += the frame's iterations
 * when residual == 0.  This differs from the genie where it should: a miscorrection adds errors, parity bits are not
 * payload, and a frame whose more-than-t errors all lie in the parity is correct.  The counters do not depend on "pooling". */
int32_t ldpc_toolbox_sim_set_bch(void *sim, void *bch);

/* ===================================================================================
 * PART 6 -- batched 5G NR rate matching and rate recovery on the GPU (3GPP TS 38.212 5.4.2: bit selection from the
 * circular buffer and the bit interleaver; on receive, soft combining of repeats and retransmissions).  The reference
 * has no rate matcher: its block puncturing pattern can only leave out the first 2 Zc columns.
 * =================================================================================== */

/* The handle is a code block configuration (BG, Zc, F, Ncb); a transmission (E, rv, Qm) is given per call, because HARQ
 * changes rv between calls on one soft buffer.
 *   n = 68 Zc (BG 1) or 52 Zc (BG 2), the columns of "nr5g:BG:ZC";  K = 22 Zc or 10 Zc;  N = n - 2 Zc.
 *   Column c of the codeword is buffer bit d = c - 2 Zc; the columns c < 2 Zc are never transmitted.
 *   Fillers: the F columns K-F .. K-1 (buffer bits K-2Zc-F .. K-2Zc-1) are NULL; 0 <= F <= K - 2 Zc.
 *   Ncb: 1 <= Ncb <= N (default N: no limited-buffer rate matching).  L = the number of non-NULL bits among buffer bits
 *   0 .. Ncb-1; L >= 1.
 *   k0 = floor(a Ncb / N) Zc with a = 0, 17, 33, 56 (BG 1) or 0, 13, 25, 43 (BG 2) for rv 0..3.
 *   Bit selection:  k = j = 0; while k < E: d = (k0 + j) mod Ncb; if d is not NULL: e[k++] = d; j++.
 *   Interleaver:    f[i + q Qm] = e[i (E / Qm) + q] for i < Qm, q < E / Qm.  Qm in 1..8 divides E; E <= 0x7fffffff.
 *   f is the transmitted order: the `output` of match and the `rx` of recover.
 * spec: "nr5g:BG:ZC[:F[:NCB]]", decimal.  NULL (message via ldpc_toolbox_last_error) for another spelling, a BG other than
 * 1 or 2, a Zc that is none of the 51 lifting sizes, or F, Ncb, L outside the ranges above.
 * The constructor needs no GPU (`device` is used by the first batched call; -1 = LDPC_TOOLBOX_DEVICE, default 0). */
void *ldpc_toolbox_nr_rm_ctor(const char *spec, int32_t device);
void ldpc_toolbox_nr_rm_dtor(void *rm);
/* key: "n", "k" (K), "zc", "base_graph", "fillers", "n_cb", "buffer_len" (L), "k0_0" .. "k0_3", "pass_elements" (a
 * batched call runs in passes of floor(pass_elements / row) frames, at least one; row = e for match, max(n, e) for
 * recover), "stage_bytes" (a host entry stages floor(stage_bytes / (max(n, e) * element size)) frames on the device at a
 * time, at least one), "device" (-1 until the first batched call made the device state).  returns 0, or -1 for an
 * unknown key. */
int32_t ldpc_toolbox_nr_rm_get(void *rm, const char *key, int64_t *value);
/* codewords [batch][n] -- exactly the output of ldpc_toolbox_encoder_encode_batch_device; a byte equal to 1 is a one,
 * anything else a zero -- to output [batch][e], bytes 0 or 1 in transmitted order.
 * A null handle, n other than the code's, rv > 3, qm outside 1..8, e == 0, e > 0x7fffffff or qm not dividing e:
 * LDPC_TOOLBOX_ERR_ARGUMENT before the GPU is touched, nothing written.  Without a GPU LDPC_TOOLBOX_ERR_DEVICE (there is
 * no CPU path).  batch == 0 returns 0; batch is otherwise unlimited.  Input and output do not overlap.  One call at a
 * time per handle.  Host pointers (staged through the handle's buffers) or, _device, device pointers and a hipStream_t:
 * a stream = enqueue and return; NULL = the handle's own stream, ordered after what the legacy default stream holds at
 * the call, synchronised on return. */
int32_t ldpc_toolbox_nr_rm_match(void *rm, uint8_t *output, size_t e, const uint8_t *codewords, size_t n, size_t batch,
                                 uint32_t rv, uint32_t qm);
int32_t ldpc_toolbox_nr_rm_match_device(void *rm, uint8_t *output, size_t e, const uint8_t *codewords, size_t n, size_t batch,
                                        uint32_t rv, uint32_t qm, void *hip_stream);
/* rx [batch][e], received values in transmitted order (the demapper's LLRs), to llrs [batch][n] -- exactly the `llrs` of
 * ldpc_toolbox_decoder_decode_batch_f32_device / _f64_device on a decoder built with puncturing "".  Per frame and
 * column c: let p_0 < p_1 < ... < p_(R-1) be the selection indices k (before interleaving) that carry c, and t_i the
 * received value at the interleaved position of p_i; S = t_0 + t_1 + ... + t_(R-1), added left to right in the element
 * type, each sum rounded once.  The output is
 *   a filler column:  filler_llr rounded once to the type, whatever `combine` is;
 *   R = 0:            +0.0, or the old value when combine != 0;
 *   otherwise:        S, or old + S when combine != 0.
 * No atomics and no reassociation: the result is a pure function of the inputs, bit for bit.  combine != 0 is HARQ soft
 * combining: call once per transmission on one buffer, the first with combine = 0.
 * filler_llr must be positive (+inf is allowed; a NaN is not): else, and for what ldpc_toolbox_nr_rm_match refuses,
 * LDPC_TOOLBOX_ERR_ARGUMENT with nothing written.  rx and llrs do not overlap.  Other behaviour as ldpc_toolbox_nr_rm_match. */
int32_t ldpc_toolbox_nr_rm_recover_f32(void *rm, float *llrs, size_t n, const float *rx, size_t e, size_t batch, uint32_t rv,
                                       uint32_t qm, double filler_llr, int32_t combine);
int32_t ldpc_toolbox_nr_rm_recover_f64(void *rm, double *llrs, size_t n, const double *rx, size_t e, size_t batch, uint32_t rv,
                                       uint32_t qm, double filler_llr, int32_t combine);
int32_t ldpc_toolbox_nr_rm_recover_f32_device(void *rm, float *llrs, size_t n, const float *rx, size_t e, size_t batch,
                                              uint32_t rv, uint32_t qm, double filler_llr, int32_t combine, void *hip_stream);
int32_t ldpc_toolbox_nr_rm_recover_f64_device(void *rm, double *llrs, size_t n, const double *rx, size_t e, size_t batch,
                                              uint32_t rv, uint32_t qm, double filler_llr, int32_t combine, void *hip_stream);
/* The simulator's option to rate-match what it transmits.  The configuration is copied (the handle may be destroyed
 * afterwards); rm == NULL returns to none.  returns -1 with a message and changes nothing unless the simulator was built
 * with puncturing "", its n equals the handle's n, the handle's F is 0 (the pool's messages are random in all k
 * positions), (e, rv, qm) is a transmission as above, and e is a multiple of the modulation's bits per symbol and of
 * |interleaving|.  While a rate matcher is set: "n_tx" is e and the rate k / e; the pool's transmitted rows
 * (ldpc_toolbox_sim_pool) are the rate-matched pooled codewords, [pool][e]; the LLRs of frame f are what the generator
 * produces for that transmitted row with the same keys, and ldpc_toolbox_sim_generate returns these [frames][e] values;
 * they are recovered with combine = 0 into the [frames][n] rows the decoder and the straggler pool see.  The counters do
 * not depend on "pooling".  "rate_match" of ldpc_toolbox_sim_get is 1 while one is set.  Setting or clearing resets the
 * straggler-pooling budget, as "modulation" does. */
int32_t ldpc_toolbox_sim_set_rate_match(void *sim, void *rm, size_t e, uint32_t rv, uint32_t qm);

/* HARQ with incremental-redundancy soft combining: a sequence of `transmissions` = T transmissions (e[t], rv[t]), t < T,
 * 1 <= T <= 8, of one qm.
 *   Configuration.  Each (e[t], rv[t], qm) is a transmission as above, each e[t] a multiple of the modulation's bits per
 *   symbol, and sum e[t] <= 0x7fffffff.  The modulation is the BPSK generator or an NR modulation
 *   (ldpc_toolbox_sim_set_nr_qam) and the interleaving 0: while "8PSK" or a table constellation is in force the sequence is
 *   refused.  The first transmission must be one that ldpc_toolbox_sim_set_rate_match accepts.
 *   ldpc_toolbox_sim_set_harq puts the simulator into the state of ldpc_toolbox_sim_set_rate_match(sim, rm, e[0], rv[0], qm)
 *   -- ldpc_toolbox_sim_run, _run_bch, _generate and _pool behave exactly as after that call -- and keeps the further
 *   transmissions.  rm == NULL, and every ldpc_toolbox_sim_set_rate_match call, clears them.  A refusal returns -1 with a
 *   message and changes nothing.  ldpc_toolbox_sim_get: "harq" (T, or 0), "harq_e0" .. "harq_e7", "harq_rv0" .. "harq_rv7".
 *   Noise.  n_tx = e[0] and the rate k / e[0]: sigma is computed from them as for every run and is the same for all T
 *   transmissions, so Es/N0 is constant and an Eb/N0 refers to the first transmission.
 *   LLRs.  A frame's HARQ process is one long transmitted row: the T rate-matched rows of its pooled codeword, concatenated,
 *   with the noise the channel puts on that row for (seed, frame).  P_t = e[0] + ... + e[t-1].  BPSK: position j of
 *   transmission t takes the normal of pair (P_t + j) >> 1, the pair's first normal when P_t + j is even and its second
 *   when odd.  NR modulation of QM bits: symbol s of transmission t takes pair P_t / QM + s.  Everything else is the
 *   generator's arithmetic; transmission 0 is bit for bit what ldpc_toolbox_sim_generate returns.
 *   ldpc_toolbox_sim_generate_harq: llrs [frames][e[transmission]] (host) and the frames' pool indices (may be NULL).
 *   Soft buffer, attempts, stopping.  After transmission 0 the soft buffer [n] of a frame is what
 *   ldpc_toolbox_nr_rm_recover_f32 gives with combine = 0, after each later one with combine = 1 into the same row.  After
 *   every transmission the frame is decoded with the full max_iterations (the straggler budget has no part in a HARQ run).
 *   A frame stops at the first attempt that converges (iteration count >= 0, right or wrong), or after transmission T-1.
 *   ldpc_toolbox_sim_run_harq: counters[6] = the fields of ldpc_toolbox_sim_run for each frame's final attempt -- frames,
 *   bit errors, frame errors, false decodes (the final attempt converged with bit errors), iterations over all attempts of
 *   the frame (a failed attempt counts max_iterations), and that sum for the frames that end with no bit error.
 *   per_tx[T][4], for each transmission: attempts, frames that stopped because the attempt converged, of those how many
 *   have bit errors, iterations of this transmission's attempts.  (Delivered after t: the sum over s <= t of
 *   per_tx[s][1] - per_tx[s][2]; transmitted bits: the sum of per_tx[t][0] * e[t].)  With T = 1 counters equals what
 *   ldpc_toolbox_sim_run returns.  A frame's result depends on (seed, frame, configuration) alone: not on the chunks a
 *   call is cut into, nor on "pooling".  "pooling" 1: the frames that need transmission t wait in a pool of that stage and
 *   are decoded thousands at a time ("pooled_frames": the retransmission attempts of the last call); 0: every chunk's
 *   failures go through all stages before the next chunk ("pooled_frames" 0).  "harq_flushes_t1" .. "harq_flushes_t7" and
 *   "harq_rows_t1" .. "harq_rows_t7": how often the last call flushed the pool of transmission t, and the rows it decoded.
 *   Without a sequence, with a BCH code set (ldpc_toolbox_sim_set_bch), or when the modulation has changed to one the
 *   sequence does not fit: LDPC_TOOLBOX_ERR_ARGUMENT, counters zeroed.  A null argument: -1, nothing written. */
int32_t ldpc_toolbox_sim_set_harq(void *sim, void *rm, const uint64_t *e, const uint32_t *rv, uint32_t transmissions, uint32_t qm);
int32_t ldpc_toolbox_sim_run_harq(void *sim, double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames,
                                  uint32_t max_iterations, uint64_t *counters /*6*/, uint64_t *per_tx /*[T][4]*/);
int32_t ldpc_toolbox_sim_generate_harq(void *sim, double ebn0_db, uint64_t seed, uint64_t first_frame, size_t frames,
                                       uint32_t transmission, float *llrs /*[frames][E_t]*/, uint32_t *pool_index);

/* ===================================================================================
 * PART 7 -- batched 5G NR transport block processing on the GPU (3GPP TS 38.212 5.1, 6.2.1, 7.2.1: CRC attachment;
 * 5.2.2: code block segmentation with CRC24B and filler bits; 5.5 with the E_r of 5.4.2.1: code block concatenation).
 * It takes payload bits to the batched encoder's input and the decoder's hard decisions back to a payload with the
 * CRC verdicts, and it produces the F of PART 6.  The reference has none of it.
 * =================================================================================== */

/* The handle is (BG, A): base graph and payload size in bits, 1 <= A <= 1277992.  Everything else follows TS 38.212:
 *   L_tb = 24 (gCRC24A) if A > 3824, else 16 (gCRC16);  B = A + L_tb;  Kcb = 8448 (BG 1) or 3840 (BG 2).
 *   B <= Kcb: C = 1, L_cb = 0, B' = B.  Otherwise L_cb = 24 (gCRC24B), C = ceil(B / (Kcb - 24)), B' = B + 24 C.
 *   K' = B' / C.  Kb = 22 (BG 1); BG 2: 10 if B > 640, 9 if B > 560, 8 if B > 192, else 6.
 *   Zc = the smallest of the 51 lifting sizes with Kb Zc >= K';  K = 22 Zc or 10 Zc;  F = K - K';  n = 68 Zc or 52 Zc.
 * The code blocks are codewords of "nr5g:BG:ZC" and are rate-matched by a PART 6 handle "nr5g:BG:ZC:F".
 * spec: "nr5g-tb:BG:A", decimal.  NULL (message via ldpc_toolbox_last_error) for another spelling, a BG other than 1 or
 * 2, an A outside the range, and a pair for which C does not divide B': the transport block sizes of TS 38.214 never
 * produce one, and the standard has no padding rule for it.
 * The constructor needs no GPU (`device` is used by the first batched call; -1 = LDPC_TOOLBOX_DEVICE, default 0). */
void *ldpc_toolbox_nr_tb_ctor(const char *spec, int32_t device);
void ldpc_toolbox_nr_tb_dtor(void *tb);
/* key: "a", "base_graph", "tb_crc" (L_tb), "b", "c", "cb_crc" (L_cb), "k_prime", "k_b", "zc", "k", "fillers" (F), "n",
 * "pass_rows" (segment and desegment run in passes of floor(pass_rows / C) transport blocks, at least one),
 * "pass_elements" (concatenate and split in passes of floor(pass_elements / G), at least one), "stage_bytes" (a host
 * entry stages floor(stage_bytes / bytes of a transport block's longest side) transport blocks on the device at a time,
 * at least one: C K bytes for segment and desegment, G elements for concatenate and split), "device" (-1 until the first
 * batched call made the device state).  returns 0, or -1 for an unknown key. */
int32_t ldpc_toolbox_nr_tb_get(void *tb, const char *key, int64_t *value);
/* TS 38.212 7.2.2: the base graph for payload size a and target code rate `rate`: 2 if a <= 292, or a <= 3824 and
 * rate <= 0.67, or rate <= 0.25; otherwise 1. */
int32_t ldpc_toolbox_nr_base_graph(uint64_t a, double rate);
/* TS 38.212 5.4.2.1, host only: the rate matching output lengths E_r of G coded bits, q = N_L Qm.  The first
 * *c_lo = C - (G/q mod C) blocks get *e_lo = q floor(G / (q C)), the others *e_hi = q ceil(G / (q C)); they sum to G.
 * A null argument, q == 0, G == 0, G > 0x7fffffff, q not dividing G or G / q < C: LDPC_TOOLBOX_ERR_ARGUMENT. */
int32_t ldpc_toolbox_nr_tb_block_lengths(void *tb, uint64_t g, uint64_t q, uint64_t *e_lo, uint64_t *e_hi, uint64_t *c_lo);
/* Conventions of every batched entry below.  Bytes hold one bit each; on input a byte equal to 1 is a one and anything
 * else a zero, outputs are 0 or 1.  Code block rows are block-major: row r * batch + b is block r of transport block b,
 * so the blocks that share one E are one contiguous batch for the rate matcher.
 * A null handle or buffer, or a length that is not the handle's: LDPC_TOOLBOX_ERR_ARGUMENT before the GPU is touched,
 * nothing written.  Without a GPU LDPC_TOOLBOX_ERR_DEVICE (there is no CPU path).  batch == 0 returns 0; batch is
 * otherwise unlimited.  Input and output do not overlap.  One call at a time per handle.  Host pointers (staged through
 * the handle's buffers) or, _device, device pointers and a hipStream_t: a stream = enqueue and return; NULL = the
 * handle's own stream, ordered after what the legacy default stream holds at the call, synchronised on return.  The
 * CRC parts of a call live in a buffer of the handle: calls on one handle on different streams are to be ordered by the
 * caller.
 *
 * Segmentation: payload [batch][a], a = A, to rows [C * batch][k], k = K -- exactly the `input` of
 * ldpc_toolbox_encoder_encode_batch_device on "nr5g:BG:ZC".  Bytes 0 .. K'-L_cb-1 of block r are bits r (K'-L_cb) .. of
 * the normalised payload followed by its L_tb CRC bits; then, when C > 1, the 24 CRC24B bits over those bytes; then F
 * zeros.  Parity bit p_0 is the coefficient of the highest power (5.1). */
int32_t ldpc_toolbox_nr_tb_segment(void *tb, uint8_t *rows, size_t k, const uint8_t *payload, size_t a, size_t batch);
int32_t ldpc_toolbox_nr_tb_segment_device(void *tb, uint8_t *rows, size_t k, const uint8_t *payload, size_t a, size_t batch,
                                          void *hip_stream);
/* The inverse with the verdicts: rows [C * batch][k] (the decode entries' `output` with output_len = K) to payload
 * [batch][a], tb_ok [batch] and cb_ok [batch][C] (may be NULL), bytes 0 or 1.
 *   cb_ok[b][r] = 1 exactly when the CRC24B remainder of the first K' bits of block r is zero;
 *   tb_ok[b]    = 1 exactly when the CRC remainder of the reassembled B bits is zero;  with C = 1, cb_ok[b][0] = tb_ok[b].
 * The filler columns are not read.  The payload is written whatever the flags say.
 * An all-zero block passes every CRC: all three are plain polynomial remainders without an initial value, and the
 * standard relies on scrambling to keep an all-zero transport block from occurring.  A receiver that may see all-zero
 * hard decisions (an erased slot) has to test for them itself. */
int32_t ldpc_toolbox_nr_tb_desegment(void *tb, uint8_t *payload, size_t a, uint8_t *tb_ok, uint8_t *cb_ok, const uint8_t *rows, size_t k,
                                     size_t batch);
int32_t ldpc_toolbox_nr_tb_desegment_device(void *tb, uint8_t *payload, size_t a, uint8_t *tb_ok, uint8_t *cb_ok, const uint8_t *rows,
                                            size_t k, size_t batch, void *hip_stream);
/* Code block concatenation (5.5).  With (e_lo, e_hi, c_lo) of the block lengths entry for (g, q): `packed` is c_lo * batch
 * rows of e_lo bytes directly followed by (C - c_lo) * batch rows of e_hi bytes, both block-major -- what two
 * ldpc_toolbox_nr_rm_match_device calls leave, the second writing behind the first -- and output is [batch][g] with block
 * 0 first, bytes normalised.  (g, q) refused by the block lengths entry: LDPC_TOOLBOX_ERR_ARGUMENT. */
int32_t ldpc_toolbox_nr_tb_concatenate(void *tb, uint8_t *output, size_t g, const uint8_t *packed, size_t q, size_t batch);
int32_t ldpc_toolbox_nr_tb_concatenate_device(void *tb, uint8_t *output, size_t g, const uint8_t *packed, size_t q, size_t batch,
                                              void *hip_stream);
/* The inverse on received values: rx [batch][g] to `packed` in the layout above, the `rx` of two recover calls.  Values
 * are copied bit for bit. */
int32_t ldpc_toolbox_nr_tb_split_f32(void *tb, float *packed, const float *rx, size_t g, size_t q, size_t batch);
int32_t ldpc_toolbox_nr_tb_split_f64(void *tb, double *packed, const double *rx, size_t g, size_t q, size_t batch);
int32_t ldpc_toolbox_nr_tb_split_f32_device(void *tb, float *packed, const float *rx, size_t g, size_t q, size_t batch, void *hip_stream);
int32_t ldpc_toolbox_nr_tb_split_f64_device(void *tb, double *packed, const double *rx, size_t g, size_t q, size_t batch, void *hip_stream);

/* ===================================================================================
 * PART 8 -- batched 5G NR modulation mapper, soft demapper and scrambling on the GPU (3GPP TS 38.211 5.1.3-5.1.6: QPSK,
 * 16QAM, 64QAM, 256QAM; 5.2.1: the length-31 Gold sequence; 6.3.1.1 / 7.3.1.1: scrambling).  It sits between PART 6 / 7
 * and the decoder: bits and LLRs here are in TRANSMITTED order -- the `output` of ldpc_toolbox_nr_rm_match /
 * ldpc_toolbox_nr_tb_concatenate and the `rx` of ldpc_toolbox_nr_rm_recover / ldpc_toolbox_nr_tb_split.  There is no
 * `interleaving` argument: NR's bit interleaver is the rate matcher's.  The reference has none of it.
 * =================================================================================== */

/* spec: "nr5g-qam:QM", QM = 2, 4, 6 or 8 bits per symbol; anything else: NULL (message via ldpc_toolbox_last_error).
 * The constructor needs no GPU (`device` is used by the first run; -1 = LDPC_TOOLBOX_DEVICE, default 0).
 * With h = QM / 2 and norm = 2, 10, 42, 170:
 *   Levels.  A level index u = sum_t a_t << (h-1-t) (a_0 the most significant bit) has the integer level
 *     L_u = (1 - 2 a_0) [2^(h-1) - (1 - 2 a_1) [2^(h-2) - ... (1 - 2 a_(h-1)) [1]]]       (38.211's nested form:
 *     h = 2: 1, 3, -1, -3;  h = 3: 3, 1, 5, 7, -3, -1, -5, -7;  h = 4: 5, 7, 3, 1, 11, 9, 13, 15 and their negatives)
 *   Amplitudes.  a = sqrt(1.0 / norm) and A_u = L_u * a in double, each rounded once.  QM = 2 is the "QPSK" of PART 4
 *     bit for bit.
 *   Symbol bits.  Of the bits b_0 .. b_(QM-1) of a symbol the I axis takes a_t = b_(2t), the Q axis a_t = b_(2t+1); the
 *     point is (A_uI, A_uQ).  Mean symbol energy 1.
 *   Scrambling sequence.  c(n) = x1(n + 1600) ^ x2(n + 1600),  x1(n + 31) = x1(n + 3) ^ x1(n),
 *     x2(n + 31) = x2(n + 3) ^ x2(n + 2) ^ x2(n + 1) ^ x2(n);  x1 starts 1, 0, ..., 0 and x2(i) = bit i of c_init, i < 31.
 *     An int64_t c_init of 0 .. 2^31 - 1 selects scrambling, -1 none; anything else is LDPC_TOOLBOX_ERR_ARGUMENT.  Every row
 *     of a batch uses the same sequence, position i of a row c(i).  The handle keeps the sequence of the last
 *     (c_init, row length) on the device: a call with another pair generates it first, on the call's stream.  The handle
 *     orders this cache across streams itself, with events and without waiting on the host: a call that reads the
 *     sequence runs after the launch that generated it, and a call that generates another runs after every earlier
 *     launch that reads the one it replaces, whatever streams those calls were given.
 *   Mapper.  bits [batch][bits_len] (a byte equal to 1 is a one, anything else a zero) -> symbols [batch][bits_len / QM],
 *     (re, im) pairs.  Bit i of a row is XORed with c(i) first.  The symbol is (A_uI, A_uQ): the doubles for _f64, each
 *     rounded once to float for _f32.
 *   Demapper.  Per axis, with coordinate x:  scale = 1 / sigma^2,  sx = x * scale,
 *       d_u = sx * A_u - K_u,   K_u = (0.5 * scale) * (A_u * A_u) made on the host in double,
 *       llr_t = F({d_u : a_t = 0}) - F({d_u : a_t = 1}),  F a left fold over ascending u starting at its first element,
 *     with the fold step of PART 4: max* (exact) or the maximum that ignores a NaN operand and orders -0 < +0 (max_log).
 *     Every product and sum is rounded once.  Bit 2t of the symbol gets the I axis's llr_t, bit 2t + 1 the Q axis's; the
 *     LLR at row position i is negated when c(i) = 1.  A positive LLR means bit 0.  The bit-j sum over the 2^QM points
 *     factorises over the axes and the other axis cancels in the LLR: this is the demapper of the whole constellation,
 *     up to rounding (tests/test_nr_qam_reference.py compares the two).
 *     _f64: all arithmetic in double.  _f32: exact = symbols widened to double, the double arithmetic, each LLR rounded
 *     once; max_log = float throughout, with scale, A_u and K_u each rounded to float once.
 * A null handle, llrs_len / bits_len != QM * symbols_len, a length above 0x7fffffff, a noise_sigma that is not finite or
 * not > 0, a c_init out of range: LDPC_TOOLBOX_ERR_ARGUMENT before the GPU is touched, nothing written.  Without a GPU
 * LDPC_TOOLBOX_ERR_DEVICE (there is no CPU path).  batch == 0 returns 0.  One call at a time per handle.
 * The AWGN channel of PART 4 works on these symbols through any complex demodulator handle, e.g. "QPSK":
 * ldpc_toolbox_awgn_run_* reads nothing of the handle's table. */
void *ldpc_toolbox_nr_qam_ctor(const char *spec, int32_t device);
void ldpc_toolbox_nr_qam_dtor(void *qam);
/* key: "bits_per_symbol" (QM), "points" (2^QM), "levels" (2^h), "device" (-1 until the first run made the device state),
 * "sequence_launches" (how often the Gold kernel has run: a repeated (c_init, length) does not run it again).
 * returns 0, or -1 for an unknown key. */
int32_t ldpc_toolbox_nr_qam_get(void *qam, const char *key, int64_t *value);
/* The 2^QM points as (re, im) doubles, point V = sum_j b_j << (QM-1-j) at index V (the indexing of PART 4's tables).
 * Written when re_im is not NULL and len (in doubles) >= 2 * 2^QM.  returns 2^QM, 0 for a null handle.  Host only. */
size_t ldpc_toolbox_nr_qam_points(void *qam, double *re_im, size_t len);
/* c(0) .. c(len - 1) of c_init (0 .. 2^31 - 1), one byte per bit, as the GPU generated them: the kernel writes the
 * sequence bit-packed, one thread per run of 1024 bits, reaching the register states at the start of its run by
 * jump-ahead (x^offset modulo each feedback polynomial), so nothing is serial in len.  len <= 0x7fffffff. */
int32_t ldpc_toolbox_nr_qam_sequence(void *qam, uint8_t *c, size_t len, int64_t c_init);
/* The argument order of ldpc_toolbox_mod_run_* / ldpc_toolbox_demod_run_* without `interleaving`, c_init last.  Host
 * pointers (staged through the handle's buffers) or, _device, device pointers and a hipStream_t: a stream = enqueue and
 * return; NULL = the handle's own stream, ordered after what the legacy default stream holds at the call, synchronised
 * on return.  The kernels move a symbol and its QM LLRs as vectors: a device symbol buffer must be aligned to one
 * (re, im) pair and a device LLR buffer to 16 bytes, else LDPC_TOOLBOX_ERR_ARGUMENT. */
int32_t ldpc_toolbox_nr_qam_mod_f32(void *qam, float *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len, size_t batch,
                                    int64_t c_init);
int32_t ldpc_toolbox_nr_qam_mod_f64(void *qam, double *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len, size_t batch,
                                    int64_t c_init);
int32_t ldpc_toolbox_nr_qam_mod_f32_device(void *qam, float *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len,
                                           size_t batch, int64_t c_init, void *hip_stream);
int32_t ldpc_toolbox_nr_qam_mod_f64_device(void *qam, double *symbols, size_t symbols_len, const uint8_t *bits, size_t bits_len,
                                           size_t batch, int64_t c_init, void *hip_stream);
int32_t ldpc_toolbox_nr_qam_demod_f32(void *qam, float *llrs, size_t llrs_len, const float *symbols, size_t symbols_len, size_t batch,
                                      double noise_sigma, int32_t max_log, int64_t c_init);
int32_t ldpc_toolbox_nr_qam_demod_f64(void *qam, double *llrs, size_t llrs_len, const double *symbols, size_t symbols_len, size_t batch,
                                      double noise_sigma, int32_t max_log, int64_t c_init);
int32_t ldpc_toolbox_nr_qam_demod_f32_device(void *qam, float *llrs, size_t llrs_len, const float *symbols, size_t symbols_len,
                                             size_t batch, double noise_sigma, int32_t max_log, int64_t c_init, void *hip_stream);
int32_t ldpc_toolbox_nr_qam_demod_f64_device(void *qam, double *llrs, size_t llrs_len, const double *symbols, size_t symbols_len,
                                             size_t batch, double noise_sigma, int32_t max_log, int64_t c_init, void *hip_stream);
/* An NR modulation as the simulator's (PART 3).  qam: a handle of ldpc_toolbox_nr_qam_ctor; its configuration is copied,
 * the handle may be destroyed afterwards.  NULL returns to what the "modulation" key selects.  Refused (-1 with a message,
 * nothing changed) unless n_tx is a multiple of QM and the simulator's "interleaving" is 0; while it is set a non-zero
 * "interleaving" is refused, and so is clearing a rate matcher when n is no multiple of QM.  With a rate matcher set
 * (ldpc_toolbox_sim_set_rate_match) its qm need not equal QM: it is the interleaver's row count and nothing here depends
 * on it, so the two are not compared -- a standard-conformant chain passes the same value to both.
 * Setting it clears a constellation of ldpc_toolbox_sim_set_constellation, and setting one of those clears it.
 * noise_sigma uses m = QM; "modulation" of ldpc_toolbox_sim_get reports QM, "nr_qam" 1 while one is set, "max_log" the
 * fold step.  Resets the straggler-pooling budget, as "modulation" does.
 * DEFINED RESULT: the LLRs of frame f are what ldpc_toolbox_nr_qam_mod_f64 (c_init -1) of the frame's pooled transmitted
 * row, then ldpc_toolbox_awgn_run_f64 (the run's seed, frame f, noise_sigma), then ldpc_toolbox_nr_qam_demod_f64 (the same
 * noise_sigma and max_log, c_init -1) give, each value rounded once to float, in transmitted order.  One fused kernel
 * computes it, one thread per symbol; the symbols are never stored. */
int32_t ldpc_toolbox_sim_set_nr_qam(void *sim, void *qam, int32_t max_log);

/* ===================================================================================
 * PART 9 -- the 8-bit soft-bit receive path: NR demapper -> rate recovery / HARQ combining -> decoder input, one byte per
 * soft bit throughout.  It ends in one of the 50 8-bit implementations (Minstarapproxi8*, Aminstari8*, Minsumi8*, either
 * schedule), whose quantiser it shares.  The reference has none of it.
 *   Unit.  One step is 1/8 of an LLR unit.  A soft bit is an int8_t in -127..127; a positive value means bit 0.
 *   clip(v) = min(max(v, -127), 127), symmetric: an input byte of -128 is read as -127 everywhere.  (Inside the decoders
 *     sums saturate to -128..127; the soft-bit path stays symmetric because the decoders are symmetric in the transmitted
 *     codeword.)
 *   Q(x) = the quantiser of the 8-bit decoders: clamp(round-half-away(8 x)) to +-127, NaN -> 0.
 * Each entry has a host form and a _device form with a trailing hipStream_t; streams and synchronisation are those of the
 * neighbouring _f32 entries.
 * =================================================================================== */

/* Batch decode of 8-bit soft bits: llrs [batch][llrs_len] int8_t.  Only a decoder whose implementation is one of the 8-bit
 * names takes it, with or without a puncturing pattern; any other returns LDPC_TOOLBOX_ERR_UNSUPPORTED before the GPU is
 * touched and writes nothing.  The other argument checks and error codes are those of the _f32 entry.
 * RESULT: `output` and `iterations` are exactly those of ldpc_toolbox_decoder_decode_batch_f32 / _f32_device on the rows
 * (float)clip(v) / 8.0f -- Q of that value is clip(v) for all 256 bytes.  posterior [batch][n] (may be NULL) is int16_t: the
 * integer that the _f32 entry converts to float.  The call takes the path the _f32 entry would take for that batch, stream
 * and option set -- groups, two lanes, the straggler pool ("pooling"), the single-launch path of small synchronised calls
 * -- with the rows moved as bytes: no float row exists anywhere, and the ingest reads a quarter of the _f32 entry's bytes.
 * A device `llrs` may be any byte address and `posterior` any int16_t address. */
int32_t ldpc_toolbox_decoder_decode_batch_i8(void *decoder, uint8_t *output, size_t output_len, const int8_t *llrs, size_t llrs_len,
                                             size_t batch, uint32_t max_iterations, int32_t *iterations, int16_t *posterior);
int32_t ldpc_toolbox_decoder_decode_batch_i8_device(void *decoder, uint8_t *output, size_t output_len, const int8_t *llrs,
                                                    size_t llrs_len, size_t batch, uint32_t max_iterations, int32_t *iterations,
                                                    int16_t *posterior, void *hip_stream);

/* The NR demapper of PART 8 (qam: a handle of ldpc_toolbox_nr_qam_ctor) with 8-bit output: llrs[i] = Q(the float that
 * ldpc_toolbox_nr_qam_demod_f32 writes at i with the same arguments, descrambling included).  One kernel, one byte out per
 * LLR; the float row is never stored.  Float symbols only.  The refusals are those of the _f32 entry, except that a device
 * `llrs` buffer needs no alignment: any byte address is valid (the QM bytes of a symbol leave as 4- or 2-byte pieces where
 * the buffer's address allows, as single bytes otherwise).  A device symbol buffer is aligned to one (re, im) pair. */
int32_t ldpc_toolbox_nr_demap_i8(void *qam, int8_t *llrs, size_t llrs_len, const float *symbols, size_t symbols_len, size_t batch,
                                 double noise_sigma, int32_t max_log, int64_t c_init);
int32_t ldpc_toolbox_nr_demap_i8_device(void *qam, int8_t *llrs, size_t llrs_len, const float *symbols, size_t symbols_len, size_t batch,
                                        double noise_sigma, int32_t max_log, int64_t c_init, void *hip_stream);

/* Rate recovery and HARQ combining of PART 6 (rm: a handle of ldpc_toolbox_nr_rm_ctor) on 8-bit soft bits, with the p_i /
 * t_i notation of ldpc_toolbox_nr_rm_recover_f32.  Per frame and column c:
 *   t_i = clip(the received byte at the interleaved position of p_i);
 *   S = t_0, then S = clip(S + t_i) for i = 1 .. R-1 in ascending selection index;
 *   the output is `filler` in a filler column, whatever `combine` is; with R = 0: 0, or clip(old) when combine != 0;
 *   otherwise S, or clip(clip(old) + S) when combine != 0.
 * Saturating sums are not associative: the order is part of the definition, and no atomics are used.  filler outside
 * 1..127 is LDPC_TOOLBOX_ERR_ARGUMENT; the other refusals are those of the _f32 entry.  It runs in passes and stages like
 * the _f32 entry, with 1-byte elements ("pass_elements", "stage_bytes").  Any byte address is a valid device `llrs` / `rx`. */
int32_t ldpc_toolbox_nr_rm_recover_i8(void *rm, int8_t *llrs, size_t n, const int8_t *rx, size_t e, size_t batch, uint32_t rv, uint32_t qm,
                                      int32_t filler, int32_t combine);
int32_t ldpc_toolbox_nr_rm_recover_i8_device(void *rm, int8_t *llrs, size_t n, const int8_t *rx, size_t e, size_t batch, uint32_t rv,
                                             uint32_t qm, int32_t filler, int32_t combine, void *hip_stream);

/* The simulator's soft buffers: the key "soft_bits" of ldpc_toolbox_sim_set takes 8 or 32 (default 32; ldpc_toolbox_sim_get
 * reports it).  8 is accepted only when the simulator's implementation is one of the 8-bit names; a refusal returns -1 with
 * a message and changes nothing.  It changes ldpc_toolbox_sim_run_harq only -- run, run_bch, generate and generate_harq stay
 * as they are.  With 8 a frame's attempt after transmission t is defined by composition: the float row that
 * ldpc_toolbox_sim_generate_harq returns for t, taken through Q; then the 8-bit rate recovery above into the frame's int8
 * soft row, with combine = (t > 0) and the plan of transmission t; then the 8-bit decode entry with the full max_iterations.
 * The stopping rule, counters[6], per_tx[T][4], their independence of chunking and of "pooling", and the harq_flushes_t /
 * harq_rows_t keys are those of the float run.  The stage pools hold [capacity][n] bytes, a quarter of the float ones; the
 * generators still write floats, which a pass of its own quantises into the int8 receive buffer recovery reads.  With 32
 * every launch and result is what it was. */

/* ===================================================================================
 * PART 10 -- the NR demapper with a scale per symbol (channel state information, CSI), and the simulator over the Rayleigh
 * block-fading channel of PART 4.  After the one-tap equaliser of an OFDM receiver every resource element has its own
 * noise variance; the demapper weights each symbol by it in the one pass it makes.  The reference has none of it.
 * Each entry has a host form and a _device form with a trailing hipStream_t; streams and synchronisation are those of the
 * PART 8 / PART 9 entries.
 * =================================================================================== */

/* The demapper of PART 8 (qam: a handle of ldpc_toolbox_nr_qam_ctor) with scale [batch][symbols_len] in place of noise_sigma:
 * one value per symbol, 1 / sigma_s^2 with sigma_s^2 that symbol's noise variance per real coordinate after equalisation.
 * Everything is PART 8's arithmetic with the symbol's own s (its scale value converted to the arithmetic type A) where
 * PART 8 has the call's scale:  sx = x * s,  K_u = (0.5 * s) * Q_u,  d_u = sx * A_u - K_u,  with Q_u = A_u * A_u made on the
 * host in double and rounded once to A, as the A_u are.  0.5 * s is exact; every other product and difference is rounded
 * once; K_u is the same for both axes.  The folds, the bit order, the descrambling sign and the arithmetic types are PART
 * 8's: _f64 double throughout; _f32 exact = symbol and scale widened to double, each LLR rounded once; _f32 max_log = float
 * throughout; _i8 = Q (PART 9) of the float that the _f32 entry writes, the float row never stored.
 * Where A is double and every s equals the double 1.0 / (sigma * sigma), the output is bit for bit that of the PART 8 entry
 * with noise_sigma = sigma -- (0.5 * scale) * (A_u * A_u) is the expression that entry's table is made of: _f64 with either
 * fold step, and exact _f32 when that double is also a float.  For max_log _f32 the K_u are float products, not rounded
 * doubles, and no such identity holds.
 * The scale values are used as given and are not checked, on the host or on the device: with finite symbols s = 0 gives
 * LLRs of magnitude 0 (an erased symbol); a negative, infinite or NaN scale gives what the arithmetic gives.
 * The refusals are PART 8's (PART 9's for _i8) without the sigma test, and a null scale: LDPC_TOOLBOX_ERR_ARGUMENT before the
 * GPU is touched, nothing written.  Device buffers: the symbol and LLR rules of those entries; scale needs the alignment of
 * its element only. */
int32_t ldpc_toolbox_nr_demap_csi_f32(void *qam, float *llrs, size_t llrs_len, const float *symbols, const float *scale, size_t symbols_len,
                                      size_t batch, int32_t max_log, int64_t c_init);
int32_t ldpc_toolbox_nr_demap_csi_f64(void *qam, double *llrs, size_t llrs_len, const double *symbols, const double *scale,
                                      size_t symbols_len, size_t batch, int32_t max_log, int64_t c_init);
int32_t ldpc_toolbox_nr_demap_csi_i8(void *qam, int8_t *llrs, size_t llrs_len, const float *symbols, const float *scale, size_t symbols_len,
                                     size_t batch, int32_t max_log, int64_t c_init);
int32_t ldpc_toolbox_nr_demap_csi_f32_device(void *qam, float *llrs, size_t llrs_len, const float *symbols, const float *scale,
                                             size_t symbols_len, size_t batch, int32_t max_log, int64_t c_init, void *hip_stream);
int32_t ldpc_toolbox_nr_demap_csi_f64_device(void *qam, double *llrs, size_t llrs_len, const double *symbols, const double *scale,
                                             size_t symbols_len, size_t batch, int32_t max_log, int64_t c_init, void *hip_stream);
int32_t ldpc_toolbox_nr_demap_csi_i8_device(void *qam, int8_t *llrs, size_t llrs_len, const float *symbols, const float *scale,
                                            size_t symbols_len, size_t batch, int32_t max_log, int64_t c_init, void *hip_stream);

/* The simulator's channel: the key "fading_block" of ldpc_toolbox_sim_set takes 0 (none, the default) up to 0x7fffffff, the
 * symbols per gain; ldpc_toolbox_sim_get reports it.  Within that range the setter always succeeds (outside it: -1 with a
 * message, nothing changed), and it resets the straggler-pooling budget as "modulation" does.  While it is not 0, a call to
 * run, run_bch, generate, run_harq or generate_harq without an NR modulation in force (ldpc_toolbox_sim_set_nr_qam) is
 * refused: -1 with a message, the counters untouched -- the run, not the setter.
 * DEFINED RESULT with fading_block B != 0: the LLRs of frame f are what ldpc_toolbox_nr_qam_mod_f64 (c_init -1) of the frame's
 * pooled transmitted row, then ldpc_toolbox_fading_run_f64 (the run's seed, frame f, noise_sigma, block B), then
 * ldpc_toolbox_nr_demap_csi_f64 on those symbols and that scale (the simulator's max_log, c_init -1) give, each value rounded
 * once to float, in transmitted order.  A HARQ process's concatenated row goes through the same channel: symbol s of
 * transmission t has index first_symbol + s, as in PART 6's simulator, and takes noise pair first_symbol + s and gain pair
 * (first_symbol + s) / B.  One fused kernel per generator, one thread per symbol; symbols and scales are never stored.
 * With "soft_bits" 8, run_harq stays the composition PART 9 defines over generate_harq; the counters stay independent of
 * chunking and of "pooling".  With 0 every launch and result is what it was. */

/* ===================================================================================
 * PART 11 -- the 5G NR link handle: one shared-channel configuration, transport blocks in one call each way, and HARQ
 * soft buffers that stay on the GPU.  It owns one handle of every stage above -- PART 7, the encoder and decoder of PART 2,
 * PART 6, PART 8 / PART 10 -- and is DEFINED BY THEIR COMPOSITION; what it adds is the bookkeeping a caller of the twelve
 * stage calls does by hand, a fused kernel for code block de-concatenation and rate recovery, and a decoder that runs only on
 * the code blocks that have not passed their CRC yet.  The reference has none of it.
 * =================================================================================== */

/* spec: "nr5g-link:BG:A:G:QM[:NL]", decimal.  BG and A as in "nr5g-tb:BG:A" (PART 7): C, K', Zc, K, F and n follow from them.
 * G = coded bits per transmission; QM = 2, 4, 6 or 8 bits per symbol; NL = 1 .. 4 layers (default 1); q = QM NL.  The blocks'
 * lengths (e_lo, e_hi, c_lo) are those of ldpc_toolbox_nr_tb_block_lengths for (G, q); a transmission is G / QM symbols.
 * implementation: a decoder implementation name as PART 2 takes it, without a device suffix; the link decodes float LLRs.
 * slots: the HARQ slots, each the state of one transport block: per code block a soft row of n floats, the K hard decisions
 * and the iteration count of its last decode, and a done flag.
 * NULL (message via ldpc_toolbox_last_error) for whatever the PART 7 constructor, the block lengths entry, the PART 6
 * constructor "nr5g:BG:ZC:F" with a transmission of e_lo or e_hi bits, or the PART 8 constructor would refuse; for slots == 0
 * or slots * C > 0x7fffffff; and for an unknown implementation name.
 * The constructor needs no GPU: the device state, the slots included, is made by the first batched call (`device`: -1 =
 * LDPC_TOOLBOX_DEVICE, default 0), and a slot reads as zeros until something is received into it. */
void *ldpc_toolbox_nr_link_ctor(const char *spec, const char *implementation, uint32_t slots, int32_t device);
void ldpc_toolbox_nr_link_dtor(void *link);
/* key: the keys of ldpc_toolbox_nr_tb_get for (BG, A) except its pass and stage sizes; "g", "qm", "layers", "q", "e_lo",
 * "e_hi", "c_lo", "symbols" (G / QM), "slots"; "max_log"; "pass_elements" (the fused recover kernel runs in launches of at
 * most this many elements (transport block, block, column); a launch may begin and end inside a transport block),
 * "stage_bytes" (a transmit call takes floor(stage_bytes / (C n)) transport blocks, at least one, through the handle's
 * buffers at a time), "device" (-1 until the first batched call made the device state); "decoded_rows" and "skipped_rows":
 * the code blocks the last receive call gave to the decoder and the ones it left alone, 0 before the first.
 * returns 0, or -1 for an unknown key. */
int32_t ldpc_toolbox_nr_link_get(void *link, const char *key, int64_t *value);
/* key: "max_log" (0, the default: the exact demapper; 1: max-log), "pass_elements" (1 .. 2^30, the default).  Results never
 * depend on "pass_elements".  returns 0, or LDPC_TOOLBOX_ERR_ARGUMENT with a message and nothing changed. */
int32_t ldpc_toolbox_nr_link_set(void *link, const char *key, int64_t value);
/* The LLR of the filler columns in the soft rows, converted to float: positive, +inf allowed (the default, as PART 6's
 * recover entries are usually called); 0, a negative value or NaN: LDPC_TOOLBOX_ERR_ARGUMENT, nothing changed. */
int32_t ldpc_toolbox_nr_link_set_filler_llr(void *link, double filler_llr);
/* Conventions: those of PART 7 and PART 8.  Bytes hold one bit each (1 is a one on input, outputs are 0 or 1); symbols are
 * (re, im) float pairs; c_init is the scrambling seed 0 .. 2^31 - 1, or -1 for no scrambling; a = A and symbols_len = G / QM.
 * A null handle or buffer, a length that is not the handle's, rv > 3, a c_init out of range: LDPC_TOOLBOX_ERR_ARGUMENT
 * before the GPU is touched, nothing written.  Without a GPU LDPC_TOOLBOX_ERR_DEVICE (there is no CPU path).  batch == 0
 * returns 0.  One call at a time per handle.  Host pointers (symbols staged in, results staged out; the soft rows never
 * leave the device) or, _device, device pointers and a hipStream_t: a stream = enqueue and return, NULL = the handle's own
 * stream, ordered after what the legacy default stream holds at the call, synchronised on return.  Device symbol buffers
 * are aligned to one (re, im) pair, scale and iterations to their element.
 *
 * Transmit: payload [batch][a] to symbols [batch][symbols_len].  Bit for bit what this chain gives: ldpc_toolbox_nr_tb_segment;
 * ldpc_toolbox_encoder_encode_batch on "nr5g:BG:ZC"; ldpc_toolbox_nr_rm_match on "nr5g:BG:ZC:F" with (rv, QM), the first
 * c_lo * batch rows at e_lo bits and, written behind them, the other rows at e_hi; ldpc_toolbox_nr_tb_concatenate for (G, q);
 * ldpc_toolbox_nr_qam_mod_f32 on "nr5g-qam:QM" with c_init.  batch is unlimited. */
int32_t ldpc_toolbox_nr_link_transmit_f32(void *link, float *symbols, size_t symbols_len, const uint8_t *payload, size_t a, size_t batch,
                                          uint32_t rv, int64_t c_init);
int32_t ldpc_toolbox_nr_link_transmit_f32_device(void *link, float *symbols, size_t symbols_len, const uint8_t *payload, size_t a,
                                                 size_t batch, uint32_t rv, int64_t c_init, void *hip_stream);
/* Receive: symbols [batch][symbols_len] to payload [batch][a], tb_ok [batch], and cb_ok and iterations [batch][C] (either
 * may be NULL), through the slots first_slot .. first_slot + batch - 1: transport block b of the call lives in slot
 * first_slot + b.  scale == NULL: the PART 8 demapper with noise_sigma (finite and positive); otherwise scale
 * [batch][symbols_len] and the PART 10 demapper, and noise_sigma is not read.  Further refusals: first_slot + batch > slots;
 * combine != 0 with a slot in the range that has never been received into (the handle knows this per slot).
 *
 * combine == 0, a first transmission, resets the slots of the range -- no block of them is done -- and is then bit for bit
 * this chain: ldpc_toolbox_nr_qam_demod_f32 (or ldpc_toolbox_nr_demap_csi_f32), exact or max-log per "max_log", with c_init;
 * ldpc_toolbox_nr_tb_split_f32 for (G, q); ldpc_toolbox_nr_rm_recover_f32 with (rv, QM), combine 0 and the handle's filler
 * LLR, at e_lo and at e_hi, into the slots' soft rows; ldpc_toolbox_decoder_decode_batch_f32 with max_iterations on all
 * C * batch rows, output_len = K; ldpc_toolbox_nr_tb_desegment.  The slots keep the soft rows, the hard decisions, the
 * iteration counts and the done flags: a block is DONE when its cb_ok is 1 (with C = 1: when tb_ok is 1).
 * combine != 0, a retransmission.  A block that is not done: its soft row becomes what ldpc_toolbox_nr_rm_recover_f32 with
 * combine 1 makes of the row the slot holds; it is decoded with the full max_iterations, and its hard decisions and
 * iteration count replace the slot's.  A block that is done: its soft row, hard decisions and iteration count stay as they
 * are, bit for bit, and the decoder does not see it.  Then ldpc_toolbox_nr_tb_desegment runs over the slots' hard decisions as
 * they stand, and iterations reports the slots' counts.  The rows to decode are listed and counted on the device; the count
 * reaches the host in one 4-byte copy, which is the one time a _device call with combine != 0 waits for its stream before it
 * returns (a combine == 0 call on a caller's stream does not wait).  With no row to decode the decoder is not called.
 * Per block the outcome is that of decoding it alone: the decoder is deterministic per codeword whatever batch surrounds it.
 * A transport block whose blocks all pass CRC24B while the transport block CRC fails -- a block has converged to another
 * codeword that happens to pass -- has nothing left to decode: it stays failed until a combine == 0 call.  And as in PART 7
 * an all-zero block passes every CRC: a receiver that may see all-zero hard decisions has to test for them itself. */
int32_t ldpc_toolbox_nr_link_receive_f32(void *link, uint8_t *payload, size_t a, uint8_t *tb_ok, uint8_t *cb_ok, int32_t *iterations,
                                         const float *symbols, const float *scale, size_t symbols_len, size_t batch, double noise_sigma,
                                         uint32_t rv, int64_t c_init, uint32_t first_slot, int32_t combine, uint32_t max_iterations);
int32_t ldpc_toolbox_nr_link_receive_f32_device(void *link, uint8_t *payload, size_t a, uint8_t *tb_ok, uint8_t *cb_ok,
                                                int32_t *iterations, const float *symbols, const float *scale, size_t symbols_len,
                                                size_t batch, double noise_sigma, uint32_t rv, int64_t c_init, uint32_t first_slot,
                                                int32_t combine, uint32_t max_iterations, void *hip_stream);
/* The rate recovery step of receive alone, for a receiver with a demapper of its own: rx [batch][g], g = G, device LLRs in
 * transmitted order (what the demapper entries write) into the soft rows of the slots, by the fused kernel: combine == 0
 * resets the slots of the range as above, combine != 0 adds to the rows of the blocks that are not done.  Nothing is decoded
 * and no verdict changes.  The refusals are receive's; the stream rules those of the _device entries. */
int32_t ldpc_toolbox_nr_link_recover_f32_device(void *link, const float *rx, size_t g, size_t batch, uint32_t rv, uint32_t first_slot,
                                                int32_t combine, void *hip_stream);
/* Host copies of the state of the slots first_slot .. first_slot + batch - 1, for tests and for a receiver that migrates a
 * HARQ process: soft [C * batch][n] floats, done [batch][C], rows [C * batch][K] hard decisions; soft and rows block-major
 * as in PART 7 (row r * batch + b is block r of slot first_slot + b).  Any of the three may be NULL.  Synchronous, on the
 * handle's own stream: a _device call on a caller's stream has to be complete.  first_slot + batch > slots:
 * LDPC_TOOLBOX_ERR_ARGUMENT. */
int32_t ldpc_toolbox_nr_link_slot_state(void *link, float *soft, uint8_t *done, uint8_t *rows, uint32_t first_slot, size_t batch);

/* ===================================================================================
 * PART 12 -- 8-bit HARQ soft buffers in the link handle of PART 11: one byte per soft bit (PART 9) from the demapper through
 * the slots to the decoder input.  DEFINED BY THE COMPOSITION of the _i8 stage entries of PART 9 and PART 10, as PART 11 is by
 * the float ones.  No float LLR row exists in this mode: the demapper output is batch * G bytes, the slots' soft rows are
 * [C * slots][n] int8_t, and so is the decoder's input.
 * =================================================================================== */

/* The mode is the key "soft_bits" of ldpc_toolbox_nr_link_set: 32 (the default: PART 11 as it stands) or 8;
 * ldpc_toolbox_nr_link_get reports it, and "soft_bytes", the bytes of the slots' soft rows, C * slots * n * (soft_bits / 8),
 * which follows from the configuration and needs no GPU.  The setter returns LDPC_TOOLBOX_ERR_ARGUMENT, with a message and
 * nothing changed: for a value other than 8 or 32; for 8 when the handle's implementation is not one of the 8-bit names of
 * PART 9; for 8 when the filler LLR quantises to the soft bit 0; and for a value other than the current one once the device
 * state exists ("device" is not -1) -- the slots are allocated by the first batched call, so the mode is chosen before it.
 * Setting the current value always returns 0.  The mode never follows from the implementation name: an 8-bit implementation
 * on float slots sums and then quantises, this mode quantises and then sums with saturation.
 * The filler soft bit of an 8-bit handle is Q(filler_llr), PART 9's quantiser: 127 for the default +inf and for every LLR
 * from 15.8125 on.  On an 8-bit handle ldpc_toolbox_nr_link_set_filler_llr also refuses a value with Q(filler_llr) == 0.
 *
 * Receive with soft_bits 8 -- ldpc_toolbox_nr_link_receive_f32[_device], signatures unchanged, symbols and scale floats.
 * combine == 0 resets the slots of the range and is then byte for byte this chain: ldpc_toolbox_nr_demap_i8 (or
 * ldpc_toolbox_nr_demap_csi_i8 when scale != NULL) per "max_log", with c_init; the bytes of block r of transport block b are
 * positions start(r) .. start(r) + E_r - 1 of row b, start(r) = r e_lo + max(r - c_lo, 0) (e_hi - e_lo) -- what
 * ldpc_toolbox_nr_tb_split_f32 does to floats, a copy; ldpc_toolbox_nr_rm_recover_i8 with (rv, QM), combine 0 and filler
 * Q(filler_llr), at e_lo and at e_hi, into the slots' soft rows; ldpc_toolbox_decoder_decode_batch_i8 with max_iterations on
 * all C * batch rows, output_len = K; ldpc_toolbox_nr_tb_desegment.
 * combine != 0 is PART 11's rule with these entries: a block that is not done gets ldpc_toolbox_nr_rm_recover_i8 with combine 1
 * on the row its slot holds -- saturating, in the fixed order of PART 9 -- and is decoded with the full budget; a done block's
 * row, hard decisions and iteration count stay as they are, byte for byte, and the decoder does not see it.  The done rule,
 * the one 4-byte count copy, "decoded_rows" / "skipped_rows", the refusals and the stream rules are PART 11's.
 * The fused recover kernel owns four columns and one dword of a soft row per thread, so its launches are whole dwords:
 * "pass_elements" rounded down to a multiple of 4, and 4 below that; results never depend on it. */

/* ldpc_toolbox_nr_link_recover_f32_device for a receiver with an 8-bit demapper of its own: rx [batch][g], g = G, device soft
 * bits in transmitted order at any byte address, -128 read as -127, into the slots' int8 soft rows by the fused kernel;
 * nothing is decoded and no verdict changes.  On a float handle LDPC_TOOLBOX_ERR_UNSUPPORTED, as
 * ldpc_toolbox_nr_link_recover_f32_device on an 8-bit handle; both before the GPU is touched.  Otherwise the refusals and the
 * stream rules are those of the float entry. */
int32_t ldpc_toolbox_nr_harq_slots_recover_i8_device(void *link, const int8_t *rx, size_t g, size_t batch, uint32_t rv,
                                                     uint32_t first_slot, int32_t combine, void *hip_stream);
/* ldpc_toolbox_nr_link_slot_state with the soft rows as the bytes an 8-bit handle's slots hold: soft [C * batch][n] int8_t.  On
 * a float handle with soft != NULL LDPC_TOOLBOX_ERR_UNSUPPORTED, as ldpc_toolbox_nr_link_slot_state with soft != NULL on an
 * 8-bit handle; with soft == NULL either entry works on either handle. */
int32_t ldpc_toolbox_nr_harq_slots_state_i8(void *link, int8_t *soft, uint8_t *done, uint8_t *rows, uint32_t first_slot, size_t batch);

/* Standard-code generator (what the reference's `dvbs2` / `5g` / `ccsds` / `ccsds-c2` CLI
 * sub-commands print, src/cli/dvbs2.rs:91, src/cli/nr5g.rs:46, src/cli/ccsds.rs:70): writes the
 * padded alist text of `spec` ("dvbs2:R1_2", "nr5g:1:384", "ar4ja:1/2:1024", "c2") into
 * buffer (NUL-terminated when it fits) and returns the number of bytes needed excluding the
 * NUL; 0 for an unknown spec. */
size_t ldpc_toolbox_code_alist(const char *spec, char *buffer, size_t buffer_len);

/* alist parser + writer of the host library on their own (reference: SparseMatrix::from_alist
 * src/sparse.rs:352-389 then alist() / alist_no_padding() :301-341): parses `alist` and writes it
 * back (padding != 0: MacKay zero padding).  Same buffer convention as ldpc_toolbox_code_alist;
 * returns 0 when `alist` is malformed (message via ldpc_toolbox_last_error). */
size_t ldpc_toolbox_alist_normalize(const char *alist, int32_t padding, char *buffer, size_t buffer_len);

/* Number of usable HIP devices (0 when the HIP runtime finds none). */
int32_t ldpc_toolbox_device_count(void);

/* Message of the last failed call on this thread ("" if none). */
const char *ldpc_toolbox_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* _LDPC_TOOLBOX_H */
