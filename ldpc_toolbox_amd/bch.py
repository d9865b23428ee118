"""Batched BCH outer code on the GPU (include/ldpc_toolbox.h, PART 5): the DVB-S2 outer code and any narrow-sense binary
BCH code over GF(2^4)..GF(2^16) -- a systematic encoder and a bounded-distance decoder.  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _capi
from .decoder import DecoderUnavailable


class BchCode:
    """`BchCode("dvbs2:R1_2")` or `BchCode("bch:M:P:T:N")` (P in hex).  Bytes hold one bit each, the first byte of a row
    the highest power of x.  The handle needs no GPU until the first batched call (device=None: GPU LDPC_TOOLBOX_DEVICE)."""

    def __init__(self, spec: str, device=0):
        L = _capi.lib()
        h = L.ldpc_toolbox_bch_ctor(spec.encode(), -1 if device is None else int(device))
        if not h:
            raise ValueError(_capi.last_error() or "BCH constructor returned NULL")
        self._h = h
        self.spec = spec

    def get(self, key: str) -> int:
        v = C.c_int64(0)
        if _capi.lib().ldpc_toolbox_bch_get(self._h, key.encode(), C.byref(v)) != 0:
            raise KeyError(key)
        return int(v.value)

    n = property(lambda self: self.get("n"))
    k = property(lambda self: self.get("k"))
    t = property(lambda self: self.get("t"))
    m = property(lambda self: self.get("m"))
    parity = property(lambda self: self.get("parity"))

    def generator(self):
        """g_0 .. g_parity as a uint8 array"""
        L = _capi.lib()
        need = L.ldpc_toolbox_bch_generator(self._h, None, 0)
        out = np.zeros(need, dtype=np.uint8)
        L.ldpc_toolbox_bch_generator(self._h, out.ctypes.data, need)
        return out

    @staticmethod
    def _raise(what, rc):
        msg = f"{what} failed ({rc}): {_capi.last_error()}"
        if rc == -4:
            raise ValueError(msg)
        raise (DecoderUnavailable if "no HIP device" in msg else RuntimeError)(msg)

    def encode(self, msgs):
        """msgs [batch][k] uint8 host array (a byte equal to 1 is a one) -> codewords [batch][n]"""
        msgs = np.ascontiguousarray(msgs, dtype=np.uint8)
        if msgs.ndim != 2:
            raise ValueError("msgs must be [batch][k]")
        B, k = msgs.shape
        n = self.n
        out = np.zeros((B, n), dtype=np.uint8)
        rc = _capi.lib().ldpc_toolbox_bch_encode_batch(self._h, out.ctypes.data, n, msgs.ctypes.data, k, B)
        if rc != 0:
            self._raise("encode", rc)
        return out

    def decode(self, bits, whole=False):
        """bits [batch][n] uint8 host array -> (out [batch][k], or [batch][n] with whole=True; errors [batch] int32:
        the number of corrected bits, -1 for a word that no codeword is within t of, which comes back unchanged)"""
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        if bits.ndim != 2:
            raise ValueError("bits must be [batch][n]")
        B, n = bits.shape
        out_len = self.n if whole else self.k
        out = np.zeros((B, out_len), dtype=np.uint8)
        errors = np.zeros(B, dtype=np.int32)
        rc = _capi.lib().ldpc_toolbox_bch_decode_batch(self._h, out.ctypes.data, out_len, bits.ctypes.data, n, B, errors.ctypes.data)
        if rc != 0:
            self._raise("decode", rc)
        return out, errors

    def encode_device(self, in_ptr: int, out_ptr: int, batch: int, stream: int = 0, input_len=None, output_len=None):
        """Raw device pointers (e.g. torch tensors' data_ptr()): messages [batch][k] -> codewords [batch][n]; stream =
        hipStream_t handle (enqueue and return) or 0 (the handle's own stream, synchronous).  input_len / output_len:
        given only to state other lengths than k and n (they are refused)."""
        rc = _capi.lib().ldpc_toolbox_bch_encode_batch_device(self._h, out_ptr, self.n if output_len is None else output_len, in_ptr,
                                                              self.k if input_len is None else input_len, batch, stream or None)
        if rc != 0:
            self._raise("encode_device", rc)

    def decode_device(self, in_ptr: int, out_ptr: int, batch: int, errors_ptr: int = 0, whole=False, stream: int = 0,
                      input_len=None, output_len=None):
        """Raw device pointers: words [batch][n] -> [batch][k] (or [batch][n] with whole=True), errors [batch] int32 or 0."""
        out_len = (self.n if whole else self.k) if output_len is None else output_len
        rc = _capi.lib().ldpc_toolbox_bch_decode_batch_device(self._h, out_ptr, out_len, in_ptr, self.n if input_len is None else input_len,
                                                              batch, errors_ptr or None, stream or None)
        if rc != 0:
            self._raise("decode_device", rc)

    def close(self):
        if getattr(self, "_h", None):
            _capi.lib().ldpc_toolbox_bch_dtor(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
