"""Python mirror of the reference's decoder boundary, over the C ABI of libldpc_toolbox.so.

Names and argument meaning follow the reference so that tests read like its own:
  * `LdpcDecoder.decode(llrs, max_iterations)`  ~ trait LdpcDecoder::decode
    (/root/reference/src/decoder.rs:19-35): returns (ok, DecoderOutput) where ok=True is the
    trait's Ok(..) and ok=False its Err(..);
  * `DecoderOutput(codeword, iterations)`       ~ decoder.rs:38-48 (iterations ==
    max_iterations on failure);
  * `DecoderImplementation(name)`               ~ decoder/factory.rs:31-277, with
    `build_decoder(h)` as in trait DecoderFactory (factory.rs:19-25).
The batched calls (`decode_batch`, `decode_batch_device`) are the extension the GPU needs.
"""
import ctypes as C
import math
import re
from dataclasses import dataclass

import numpy as np

from . import _capi
from .sparse import SparseMatrix

# implementation names accepted by the HIP path (factory.rs:240-277 float rows + Minsum)
_RULES = ("Phi", "Tanh", "Minstarapprox", "Aminstar", "Minsum")
IMPLEMENTATIONS = tuple(p + r + s for p in ("", "HL") for r in _RULES for s in ("f64", "f32"))
# the reference's 8-bit quantised names (factory.rs:246-263, 270-275)
I8_IMPLEMENTATIONS = tuple(b + j + h + d for b in ("Minstarapproxi8", "Aminstari8") for j in ("", "Jones")
                           for h in ("", "PartialHardLimit") for d in ("", "Deg1Clip")) + (
    "HLMinstarapproxi8", "HLMinstarapproxi8PartialHardLimit", "HLAminstari8", "HLAminstari8PartialHardLimit")
ALL_IMPLEMENTATIONS = IMPLEMENTATIONS + I8_IMPLEMENTATIONS
# opt-in approximate variants (native exp2 / log2 / rcp instead of the glibc-identical functions): NOT bit-identical to
# the reference, never chosen unless asked for by name
FAST_IMPLEMENTATIONS = ("Tanhf32@fast", "HLTanhf32@fast", "Phif32@fast", "HLPhif32@fast")
# normalized and offset min-sum with their default values (alpha = 0.75, beta = 0.5): the Minsum decoder whose check
# rows send alpha * m or max(m - beta, 0) instead of the magnitude m.  Any of them also takes ":value" -- digits[.digits],
# 0 < alpha <= 1, beta >= 0 -- as in "NormMinsumf32:0.8125".  Not the reference's, so not part of ALL_IMPLEMENTATIONS.
CORRECTED_MINSUM_IMPLEMENTATIONS = tuple(p + r + s for p in ("", "HL") for r in ("NormMinsum", "OffsetMinsum")
                                         for s in ("f64", "f32"))
_CORRECTED = re.compile(r"(?:HL)?(Norm|Offset)Minsumf(?:32|64)(?::([0-9]+(?:\.[0-9]+)?))?", re.ASCII)


def corrected_minsum(name: str):
    """("Norm" | "Offset", value) for a valid normalized / offset min-sum name, None for anything else (the rules of
    csrc/implementation.cpp: the value is digits[.digits], 0 < alpha <= 1, beta >= 0 and finite)."""
    m = _CORRECTED.fullmatch(name)
    if not m:
        return None
    kind = m.group(1)
    value = float(m.group(2)) if m.group(2) is not None else (0.75 if kind == "Norm" else 0.5)
    if not math.isfinite(value) or (kind == "Norm" and not 0.0 < value <= 1.0):
        return None
    return kind, value

# 8-bit min-sum with the default values (alpha = 0.75, beta = 0.5): Minstarapproxi8's quantised arithmetic and options with
# the check-node fold reduced to min, and the magnitude m (quantiser units) corrected in integers -- (a * m + 8) >> 4 with
# a = 16 alpha, or max(m - b, 0) with b = 8 beta.  The names with Norm / Offset also take ":value" (digits[.digits]; 16 alpha
# an integer in 1..16, 8 beta an integer in 0..127), as in "Minsumi8NormJones:0.8125".  Not part of ALL_IMPLEMENTATIONS.
MINSUM_I8_IMPLEMENTATIONS = tuple(
    n for b in ("Minsumi8", "Minsumi8Norm", "Minsumi8Offset")
    for n in tuple(b + j + h + d for j in ("", "Jones") for h in ("", "PartialHardLimit") for d in ("", "Deg1Clip"))
    + ("HL" + b, "HL" + b + "PartialHardLimit"))
_MINSUM_I8 = re.compile(r"(HL)?Minsumi8(Norm|Offset)?(Jones)?(PartialHardLimit)?(Deg1Clip)?(?::([0-9]+(?:\.[0-9]+)?))?", re.ASCII)


def minsum_i8(name: str):
    """(None | "Norm" | "Offset", the kernels' integer a = 16 alpha or b = 8 beta, 0 for the plain rule) for a valid 8-bit
    min-sum name, None for anything else (the rules of csrc/implementation.cpp)."""
    m = _MINSUM_I8.fullmatch(name)
    if not m:
        return None
    layered, kind, jones, _, deg1, value = m.groups()
    if (layered and (jones or deg1)) or (value is not None and kind is None):
        return None
    if kind is None:
        return None, 0
    scaled = (float(value) if value is not None else (0.75 if kind == "Norm" else 0.5)) * (16.0 if kind == "Norm" else 8.0)
    if scaled != math.floor(scaled) or not (1.0 if kind == "Norm" else 0.0) <= scaled <= (16.0 if kind == "Norm" else 127.0):
        return None
    return kind, int(scaled)


class DecoderUnavailable(RuntimeError):
    """ctor returned NULL (no GPU, bad alist, unknown implementation, bad pattern)."""


@dataclass
class DecoderOutput:
    codeword: np.ndarray  # u8, one byte per bit, all n bits
    iterations: int


class LdpcDecoder:
    """One Tanner graph + rule + schedule on one GPU."""

    def __init__(self, alist: str, implementation: str, puncturing: str = "", device=None):
        L = _capi.lib()
        if device is None:
            h = L.ldpc_toolbox_decoder_ctor_alist_string(alist.encode(), implementation.encode(),
                                                         puncturing.encode())
        else:
            h = L.ldpc_toolbox_decoder_ctor_alist_string_on_device(
                alist.encode(), implementation.encode(), puncturing.encode(), int(device))
        if not h:
            raise DecoderUnavailable(_capi.last_error() or "decoder constructor returned NULL")
        self._h = h
        self.implementation = implementation
        self.n = self.get("n")
        self.m = self.get("m")
        self.k = self.get("k")
        self.edges = self.get("edges")
        self.input_len = self.get("input_len")
        self.device = self.get("device")

    # -- properties / tunables ---------------------------------------------------------
    def get(self, key: str) -> int:
        v = C.c_int64(0)
        if _capi.lib().ldpc_toolbox_decoder_get(self._h, key.encode(), C.byref(v)) != 0:
            raise KeyError(key)
        return int(v.value)

    def set(self, key: str, value: int):
        if _capi.lib().ldpc_toolbox_decoder_set(self._h, key.encode(), int(value)) != 0:
            raise KeyError(key)

    def kernel_stats(self, kind: int, reset=False):
        n = C.c_uint64(0)
        ms = C.c_double(0.0)
        _capi.lib().ldpc_toolbox_decoder_kernel_stats(self._h, kind, C.byref(n), C.byref(ms), int(reset))
        return int(n.value), float(ms.value)

    # -- the reference's scalar contract ------------------------------------------------
    def decode(self, llrs, max_iterations: int):
        """trait LdpcDecoder::decode: llrs are f64 (f32 arrays go through the _f32 entry)."""
        llrs = np.ascontiguousarray(llrs)
        if llrs.dtype != np.float32:
            llrs = llrs.astype(np.float64, copy=False)
        if llrs.shape != (self.input_len,):
            raise ValueError("LLR length does not match the code")  # the reference asserts
        out = np.zeros(self.n, dtype=np.uint8)
        L = _capi.lib()
        fn = L.ldpc_toolbox_decoder_decode_f32 if llrs.dtype == np.float32 else L.ldpc_toolbox_decoder_decode_f64
        it = fn(self._h, out.ctypes.data, self.n, llrs.ctypes.data, llrs.shape[0], max_iterations)
        if it >= 0:
            return True, DecoderOutput(out, it)
        if it < -1:  # LDPC_TOOLBOX_ERR_*: the call failed (the reference would have panicked), nothing decoded
            raise RuntimeError(_capi.last_error() or f"decode failed with error {it}")
        return False, DecoderOutput(out, max_iterations)

    # -- batched extension ----------------------------------------------------------------
    def decode_batch(self, llrs, max_iterations: int, output_len=None, want_posterior=False, out=None):
        """llrs [B][input_len] f32/f64 host array -> (bits [B][output_len] u8,
        iterations [B] i32 with -1 = failed, posterior [B][n] or None).
        An int8 array holds 8-bit soft bits (1/8 of an LLR unit per step, -128 read as -127; the 8-bit implementations
        only): the results are those of the rows clip(v) / 8 as float32, and the posterior is int16.
        out: (bits, iterations[, posterior]) arrays of those shapes to fill instead of fresh ones (a
        caller that decodes batch after batch reuses its buffers, as a C caller would)."""
        llrs = np.ascontiguousarray(llrs)
        if llrs.dtype not in (np.float32, np.float64, np.int8):
            llrs = llrs.astype(np.float64)
        post_dtype = np.int16 if llrs.dtype == np.int8 else llrs.dtype
        B, ln = llrs.shape
        output_len = self.n if output_len is None else output_len
        if out is not None:
            bits, its = out[0], out[1]
            post = out[2] if want_posterior else None
            ok = (bits.shape == (B, output_len) and bits.dtype == np.uint8 and bits.flags.c_contiguous
                  and its.shape == (B,) and its.dtype == np.int32 and its.flags.c_contiguous
                  and (post is None or (post.shape == (B, self.n) and post.dtype == post_dtype and post.flags.c_contiguous)))
            if not ok:
                raise ValueError("out arrays do not match the batch")
        else:
            bits = np.zeros((B, output_len), dtype=np.uint8)
            its = np.zeros(B, dtype=np.int32)
            post = np.zeros((B, self.n), dtype=post_dtype) if want_posterior else None
        L = _capi.lib()
        fn = {np.dtype(np.float32): L.ldpc_toolbox_decoder_decode_batch_f32, np.dtype(np.float64): L.ldpc_toolbox_decoder_decode_batch_f64,
              np.dtype(np.int8): L.ldpc_toolbox_decoder_decode_batch_i8}[llrs.dtype]
        rc = fn(self._h, bits.ctypes.data, output_len, llrs.ctypes.data, ln, B, max_iterations,
                its.ctypes.data, post.ctypes.data if want_posterior else None)
        if rc != 0:
            raise RuntimeError(f"decode_batch failed ({rc}): {_capi.last_error()}")
        return bits, its, post

    def decode_batch_device(self, llrs_ptr: int, f64: bool, batch: int, max_iterations: int,
                            bits_ptr: int, output_len: int, iterations_ptr: int = 0,
                            posterior_ptr: int = 0, stream: int = 0, i8: bool = False):
        """Raw device pointers (e.g. torch tensors' data_ptr()); stream = hipStream_t handle or 0.  i8: the rows are 8-bit
        soft bits (int8, any byte address) and the posterior int16; the 8-bit implementations only."""
        L = _capi.lib()
        fn = (L.ldpc_toolbox_decoder_decode_batch_i8_device if i8 else L.ldpc_toolbox_decoder_decode_batch_f64_device if f64
              else L.ldpc_toolbox_decoder_decode_batch_f32_device)
        rc = fn(self._h, bits_ptr, output_len, llrs_ptr, self.input_len, batch, max_iterations,
                iterations_ptr or None, posterior_ptr or None, stream or None)
        if rc != 0:
            raise RuntimeError(f"decode_batch_device failed ({rc}): {_capi.last_error()}")

    def syndrome(self, bits):
        """Syndrome of hard decisions (the reference's check_llrs, src/decoder.rs:157-164, with the
        parities returned): bits [B][n] u8 -> (syndrome [B][m] u8, weight [B] u32)."""
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        if bits.ndim != 2:
            raise ValueError("bits must be [batch][n]")
        B = bits.shape[0]
        syn = np.zeros((B, self.m), dtype=np.uint8)
        weight = np.zeros(B, dtype=np.uint32)
        rc = _capi.lib().ldpc_toolbox_decoder_syndrome(self._h, bits.ctypes.data, bits.shape[1], B,
                                                       syn.ctypes.data, weight.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"syndrome failed ({rc}): {_capi.last_error()}")
        return syn, weight

    def close(self):
        if getattr(self, "_h", None):
            _capi.lib().ldpc_toolbox_decoder_dtor(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DecoderImplementation:
    """FromStr / Display / DecoderFactory of the reference's enum (factory.rs:211-236)."""

    def __init__(self, name: str):
        if name not in ALL_IMPLEMENTATIONS and corrected_minsum(name) is None and minsum_i8(name) is None:
            raise ValueError("invalid decoder implementation")  # factory.rs:221
        self.name = name

    def __str__(self):
        return self.name

    def build_decoder(self, h, puncturing: str = "", device=None) -> LdpcDecoder:
        alist = h.alist() if isinstance(h, SparseMatrix) else str(h)
        return LdpcDecoder(alist, self.name, puncturing, device)


class Encoder:
    """C ABI encoder (/root/reference/src/c_api/encoder.rs:14-53), and its batched form on the GPU.

    device=None: the handle needs no GPU until the first batched call (which then uses GPU LDPC_TOOLBOX_DEVICE,
    default 0); device=N: the device tables are built at once on GPU N (DecoderUnavailable without one)."""

    def __init__(self, alist: str, puncturing: str = "", device=None):
        L = _capi.lib()
        if device is None:
            h = L.ldpc_toolbox_encoder_ctor_alist_string(alist.encode(), puncturing.encode())
            if not h:
                raise ValueError(_capi.last_error() or "encoder constructor returned NULL")
        else:
            h = L.ldpc_toolbox_encoder_ctor_alist_string_on_device(alist.encode(), puncturing.encode(), int(device))
            if not h:
                msg = _capi.last_error() or "encoder constructor returned NULL"
                raise (DecoderUnavailable if "HIP" in msg or "device" in msg else ValueError)(msg)
        self._h = h

    def get(self, key: str) -> int:
        v = C.c_int64(0)
        if _capi.lib().ldpc_toolbox_encoder_get(self._h, key.encode(), C.byref(v)) != 0:
            raise KeyError(key)
        return int(v.value)

    k = property(lambda self: self.get("k"))
    n = property(lambda self: self.get("n"))
    output_len = property(lambda self: self.get("output_len"))
    staircase = property(lambda self: bool(self.get("staircase")))
    # which form of the staircase kernels a batched call takes: 0 = 32 frames per word staged in LDS, 1 = 16 frames per
    # word staged in LDS, 2 = gathered from global memory; -1 = not a staircase code
    staircase_form = property(lambda self: self.get("staircase_form"))
    device = property(lambda self: self.get("device"))

    def encode(self, message, output_len: int):
        message = np.ascontiguousarray(message, dtype=np.uint8)
        out = np.zeros(output_len, dtype=np.uint8)
        _capi.lib().ldpc_toolbox_encoder_encode(self._h, out.ctypes.data, output_len,
                                                message.ctypes.data, message.shape[0])
        if _capi.last_error():
            raise ValueError(_capi.last_error())
        return out

    # -- batched extension (GPU; there is no CPU fallback) -----------------------------------
    def encode_batch(self, messages):
        """messages [B][k] u8 host array (a byte equal to 1 is a one) -> codewords [B][output_len] u8:
        what a loop of `encode` gives, computed on the GPU."""
        messages = np.ascontiguousarray(messages, dtype=np.uint8)
        if messages.ndim != 2:
            raise ValueError("messages must be [batch][k]")
        B, k = messages.shape
        output_len = self.output_len
        out = np.zeros((B, max(output_len, 0)), dtype=np.uint8)
        rc = _capi.lib().ldpc_toolbox_encoder_encode_batch(self._h, out.ctypes.data, output_len,
                                                           messages.ctypes.data, k, B)
        if rc != 0:
            raise RuntimeError(f"encode_batch failed ({rc}): {_capi.last_error()}")
        return out

    def encode_batch_device(self, in_ptr: int, out_ptr: int, batch: int, stream: int = 0):
        """Raw device pointers (e.g. torch uint8 tensors' data_ptr()): in [batch][k] -> out [batch][output_len];
        stream = hipStream_t handle (enqueue and return) or 0 (the handle's own stream, synchronous)."""
        rc = _capi.lib().ldpc_toolbox_encoder_encode_batch_device(self._h, out_ptr, self.output_len, in_ptr, self.k,
                                                                  batch, stream or None)
        if rc != 0:
            raise RuntimeError(f"encode_batch_device failed ({rc}): {_capi.last_error()}")

    def close(self):
        if getattr(self, "_h", None):
            _capi.lib().ldpc_toolbox_encoder_dtor(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Simulator:
    """GPU-resident simulation step over the C ABI (include/ldpc_toolbox.h part 3): frames are
    generated, decoded and scored on the device; only six counters come back."""

    def __init__(self, alist: str, implementation: str, puncturing: str = "", device: int = 0, pool_size: int = 64,
                 pool_seed: int = 1, modulation="BPSK", interleaving: int = 0, max_log: bool = False):
        """modulation: "BPSK" or "8PSK" (factory.rs:53-73), "QPSK", or a `Demodulator` -- any constellation of up to 32
        points with unit mean energy (its table is copied; the instance may be closed afterwards).  max_log: the max-log
        demapper instead of the exact one ("QPSK" or a `Demodulator` only).  interleaving: columns of the DVB-S2 bit
        interleaver, negative = rows read backwards, 0 = none (ber.rs:250-252)."""
        constellation = owned = None
        if isinstance(modulation, str):
            bits_per_symbol = {"BPSK": 1, "8PSK": 3, "QPSK": 1}.get(modulation)
            if bits_per_symbol is None:
                raise ValueError(f"invalid modulation {modulation}")
            if max_log and modulation != "QPSK":
                raise ValueError('max_log needs a constellation: "QPSK" or a Demodulator instance')
            if modulation == "QPSK":
                from .demodulator import Demodulator
                constellation = owned = Demodulator("QPSK", device=device)
        elif hasattr(modulation, "_h") and hasattr(modulation, "bits_per_symbol"):
            constellation, bits_per_symbol = modulation, 1
            modulation = f"constellation:{constellation.points}"
        else:
            raise ValueError(f"invalid modulation {modulation!r}")
        h = _capi.lib().ldpc_toolbox_sim_ctor(alist.encode(), implementation.encode(), puncturing.encode(),
                                              int(device), int(pool_size), int(pool_seed))
        if not h:
            raise DecoderUnavailable(_capi.last_error() or "simulator constructor returned NULL")
        self._h = h
        self.k, self.n, self.n_tx, self.pool = (self.get(x) for x in ("k", "n", "n_tx", "pool"))
        self.rate = self.k / self.n_tx
        self.modulation, self.interleaving, self.max_log = modulation, int(interleaving), bool(max_log)
        try:
            for key, value in (("modulation", bits_per_symbol), ("interleaving", int(interleaving))):
                if _capi.lib().ldpc_toolbox_sim_set(self._h, key.encode(), value) != 0:
                    msg = _capi.last_error() or f"cannot set {key}"
                    self.close()
                    raise ValueError(msg)
            if constellation is not None:
                try:
                    self.set_constellation(constellation, max_log)
                except ValueError:
                    self.close()
                    raise
        finally:
            if owned is not None:
                owned.close()
        self.bits_per_symbol = self.get("modulation")

    def set_constellation(self, demodulator, max_log=False):
        """`demodulator`: a `Demodulator` whose constellation generates the frames from now on, or None for what the
        "modulation" key selects.  ValueError (nothing changed) when the simulator refuses it."""
        h = None if demodulator is None else demodulator._h
        if _capi.lib().ldpc_toolbox_sim_set_constellation(self._h, h, int(bool(max_log))) != 0:
            raise ValueError(_capi.last_error() or "cannot set the constellation")

    def set_nr_qam(self, qam, max_log=False):
        """`qam`: an `NrQam` whose 5G NR modulation (no scrambling) generates the frames from now on, in place of any
        constellation of `set_constellation`, or None for what the "modulation" key selects.  ValueError (nothing changed)
        unless n_tx is a multiple of its bits per symbol and the interleaving is 0."""
        h = None if qam is None else qam._h
        if _capi.lib().ldpc_toolbox_sim_set_nr_qam(self._h, h, int(bool(max_log))) != 0:
            raise ValueError(_capi.last_error() or "cannot set the NR modulation")
        self.bits_per_symbol = self.get("modulation")

    def set_bch(self, code):
        """`code`: a `BchCode` whose bounded-distance decoder gives the outer-BCH counters of `run(..., bch_max_errors=t)`
        from now on, or None for the genie ("at most bch_max_errors bit errors count as corrected").  ValueError (nothing
        changed) unless the code's n is this simulator's k."""
        h = None if code is None else code._h
        if _capi.lib().ldpc_toolbox_sim_set_bch(self._h, h) != 0:
            raise ValueError(_capi.last_error() or "cannot set the BCH code")

    def set_rate_match(self, rm, e: int = 0, rv: int = 0, qm: int = 1):
        """`rm`: an `NrRateMatcher` (no filler bits, the simulator's n) whose transmission (e, rv, qm) the frames go
        through from now on -- n_tx becomes e and the rate k / e -- or None for none.  ValueError (nothing changed) when the
        simulator refuses it."""
        h = None if rm is None else rm._h
        if _capi.lib().ldpc_toolbox_sim_set_rate_match(self._h, h, int(e), int(rv), int(qm)) != 0:
            raise ValueError(_capi.last_error() or "cannot set the rate matcher")
        self.n_tx = self.get("n_tx")
        self.rate = self.k / self.n_tx

    def set_harq(self, rm, transmissions=(), qm: int = 1):
        """`rm`: an `NrRateMatcher` as for `set_rate_match`; `transmissions`: 1 to 8 pairs (e, rv), the HARQ sequence of
        `run_harq` and `generate_harq`.  The simulator is then in the state of set_rate_match(rm, e_0, rv_0, qm): `run`,
        `generate` and `pool_data` are those of that call.  None, like every `set_rate_match` call, clears the sequence.
        ValueError (nothing changed) when the simulator refuses it."""
        seq = [(int(e), int(rv)) for e, rv in transmissions]
        e = np.array([x[0] for x in seq], dtype=np.uint64)
        rv = np.array([x[1] for x in seq], dtype=np.uint32)
        h = None if rm is None else rm._h
        if _capi.lib().ldpc_toolbox_sim_set_harq(self._h, h, e.ctypes.data, rv.ctypes.data, len(seq), int(qm)) != 0:
            raise ValueError(_capi.last_error() or "cannot set the HARQ sequence")
        self.n_tx = self.get("n_tx")
        self.rate = self.k / self.n_tx

    def harq(self):
        """the sequence in force: a list of (e, rv), empty without one"""
        return [(self.get(f"harq_e{t}"), self.get(f"harq_rv{t}")) for t in range(self.get("harq"))]

    def run_harq(self, ebn0_db, seed, first_frame, frames, max_iterations):
        """-> (int64[6], int64[T, 4]): the counters of `run` for every frame's final attempt (iterations summed over its
        attempts), and per transmission: attempts, frames that stopped because the attempt converged, of those with bit
        errors, iterations of these attempts (include/ldpc_toolbox.h, ldpc_toolbox_sim_run_harq)"""
        T = self.get("harq")
        out = np.zeros(6, dtype=np.uint64)
        per_tx = np.zeros((max(T, 1), 4), dtype=np.uint64)
        rc = _capi.lib().ldpc_toolbox_sim_run_harq(self._h, float(ebn0_db), int(seed), int(first_frame), int(frames),
                                                   int(max_iterations), out.ctypes.data, per_tx.ctypes.data)
        if rc == -4:
            raise ValueError(f"sim_run_harq refused ({rc}): {_capi.last_error()}")
        if rc != 0:
            raise RuntimeError(f"sim_run_harq failed ({rc}): {_capi.last_error()}")
        return out.astype(np.int64), per_tx[:T].astype(np.int64)

    def generate_harq(self, ebn0_db, seed, first_frame, frames, t):
        """-> (float32 [frames][E_t], pool index per frame): transmission t of the frames"""
        T = self.get("harq")
        if not 0 <= int(t) < T:
            raise ValueError(f"the HARQ sequence has {T} transmissions: no transmission {t}")
        llrs = np.zeros((frames, self.get(f"harq_e{int(t)}")), dtype=np.float32)
        idx = np.zeros(frames, dtype=np.uint32)
        rc = _capi.lib().ldpc_toolbox_sim_generate_harq(self._h, float(ebn0_db), int(seed), int(first_frame), int(frames), int(t),
                                                        llrs.ctypes.data, idx.ctypes.data)
        if rc == -4:
            raise ValueError(f"sim_generate_harq refused ({rc}): {_capi.last_error()}")
        if rc != 0:
            raise RuntimeError(f"sim_generate_harq failed ({rc}): {_capi.last_error()}")
        return llrs, idx

    def get(self, key):
        v = C.c_int64(0)
        if _capi.lib().ldpc_toolbox_sim_get(self._h, key.encode(), C.byref(v)) != 0:
            raise KeyError(key)
        return int(v.value)

    def set(self, key, value):
        """"soft_bits": 8 keeps `run_harq`'s soft buffers as 8-bit soft bits (an 8-bit implementation only; ValueError and
        nothing changed otherwise), 32 (the default) as floats.  "fading_block": B > 0 puts the Rayleigh block-fading channel
        with perfect CSI, one gain per B symbols, between the NR mapper and demapper of `set_nr_qam` (without one the runs
        are refused); 0 (the default) returns to AWGN."""
        if _capi.lib().ldpc_toolbox_sim_set(self._h, key.encode(), int(value)) != 0:
            if key in ("soft_bits", "fading_block"):
                raise ValueError(_capi.last_error() or f"cannot set {key}")
            raise KeyError(key)

    def run(self, ebn0_db, seed, first_frame, frames, max_iterations, bch_max_errors: int = 0):
        """-> int64[6]: frames, bit errors, frame errors, false decodes, total iterations, iterations of
        the correct frames (sharding.COUNTER_FIELDS); with bch_max_errors > 0 int64[9]: those, then
        the outer-BCH bit errors, frame errors and iterations of the corrected frames
        (sharding.BCH_COUNTER_FIELDS, ber.rs:328-337)"""
        out = np.zeros(9 if bch_max_errors > 0 else 6, dtype=np.uint64)
        if bch_max_errors > 0:
            rc = _capi.lib().ldpc_toolbox_sim_run_bch(self._h, float(ebn0_db), int(seed), int(first_frame), int(frames),
                                                      int(max_iterations), int(bch_max_errors), out.ctypes.data)
        else:
            rc = _capi.lib().ldpc_toolbox_sim_run(self._h, float(ebn0_db), int(seed), int(first_frame), int(frames),
                                                  int(max_iterations), out.ctypes.data)
        if rc == -4:
            raise ValueError(f"sim_run refused ({rc}): {_capi.last_error()}")
        if rc != 0:
            raise RuntimeError(f"sim_run failed ({rc}): {_capi.last_error()}")
        return out.astype(np.int64)

    def generate(self, ebn0_db, seed, first_frame, frames):
        llrs = np.zeros((frames, self.n_tx), dtype=np.float32)
        idx = np.zeros(frames, dtype=np.uint32)
        rc = _capi.lib().ldpc_toolbox_sim_generate(self._h, float(ebn0_db), int(seed), int(first_frame), int(frames),
                                                   llrs.ctypes.data, idx.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"sim_generate failed ({rc}): {_capi.last_error()}")
        return llrs, idx

    def generate_into(self, device_ptr: int, ebn0_db, seed, first_frame, frames):
        """the same frames written straight into a device buffer [frames][n_tx] f32 (e.g. a torch tensor's data_ptr() on
        the simulator's GPU) -> pool index per frame"""
        idx = np.zeros(frames, dtype=np.uint32)
        rc = _capi.lib().ldpc_toolbox_sim_generate(self._h, float(ebn0_db), int(seed), int(first_frame), int(frames),
                                                   C.c_void_p(device_ptr), idx.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"sim_generate failed ({rc}): {_capi.last_error()}")
        return idx

    def pool_data(self):
        msgs = np.zeros((self.pool, self.k), dtype=np.uint8)
        tx = np.zeros((self.pool, self.n_tx), dtype=np.uint8)
        _capi.lib().ldpc_toolbox_sim_pool(self._h, msgs.ctypes.data, tx.ctypes.data)
        return msgs, tx

    def close(self):
        if getattr(self, "_h", None):
            _capi.lib().ldpc_toolbox_sim_dtor(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
