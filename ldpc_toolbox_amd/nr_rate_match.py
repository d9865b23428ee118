"""Batched 5G NR rate matching and rate recovery on the GPU (include/ldpc_toolbox.h, PART 6; TS 38.212 5.4.2): bit
selection from the circular buffer and the bit interleaver, and on receive the soft combining of repeats and
retransmissions.  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _capi
from .decoder import DecoderUnavailable


class NrRateMatcher:
    """`NrRateMatcher("nr5g:BG:ZC[:F[:NCB]]")`: the code block configuration; the transmission (e, rv, qm) is given per
    call.  Codeword bytes hold one bit each; `rx` and `match`'s output are in transmitted order.  The handle needs no GPU
    until the first batched call (device=None: GPU LDPC_TOOLBOX_DEVICE)."""

    def __init__(self, spec: str, device=0):
        L = _capi.lib()
        h = L.ldpc_toolbox_nr_rm_ctor(spec.encode(), -1 if device is None else int(device))
        if not h:
            raise ValueError(_capi.last_error() or "rate matcher constructor returned NULL")
        self._h = h
        self.spec = spec

    def get(self, key: str) -> int:
        v = C.c_int64(0)
        if _capi.lib().ldpc_toolbox_nr_rm_get(self._h, key.encode(), C.byref(v)) != 0:
            raise KeyError(key)
        return int(v.value)

    n = property(lambda self: self.get("n"))
    k = property(lambda self: self.get("k"))
    zc = property(lambda self: self.get("zc"))
    base_graph = property(lambda self: self.get("base_graph"))
    fillers = property(lambda self: self.get("fillers"))
    n_cb = property(lambda self: self.get("n_cb"))
    buffer_len = property(lambda self: self.get("buffer_len"))

    def k0(self, rv: int) -> int:
        return self.get(f"k0_{int(rv)}")

    @staticmethod
    def _raise(what, rc):
        msg = f"{what} failed ({rc}): {_capi.last_error()}"
        if rc == -4:
            raise ValueError(msg)
        raise (DecoderUnavailable if "no HIP device" in msg else RuntimeError)(msg)

    def match(self, codewords, e: int, rv: int = 0, qm: int = 1):
        """codewords [batch][n] uint8 host array (a byte equal to 1 is a one) -> transmitted bits [batch][e]"""
        codewords = np.ascontiguousarray(codewords, dtype=np.uint8)
        if codewords.ndim != 2:
            raise ValueError("codewords must be [batch][n]")
        B, n = codewords.shape
        out = np.zeros((B, max(int(e), 0)), dtype=np.uint8)
        rc = _capi.lib().ldpc_toolbox_nr_rm_match(self._h, out.ctypes.data, int(e), codewords.ctypes.data, n, B, int(rv), int(qm))
        if rc != 0:
            self._raise("match", rc)
        return out

    def recover(self, rx, rv: int = 0, qm: int = 1, filler_llr: float = float("inf"), into=None):
        """rx [batch][e] float32 or float64 host array -> LLRs [batch][n] of the same type: per column the sum of its
        repeats, +0 for a column that was not sent, filler_llr for a filler column.  into: a C-contiguous [batch][n] array
        of rx's type holding the soft buffer of earlier transmissions; this one is added into it (HARQ combining) and
        the array returned."""
        rx = np.ascontiguousarray(rx)
        if rx.dtype not in (np.float32, np.float64):
            rx = rx.astype(np.float32)
        if rx.ndim != 2:
            raise ValueError("rx must be [batch][e]")
        B, e = rx.shape
        n = self.n
        if into is None:
            out = np.zeros((B, n), dtype=rx.dtype)
        else:
            out = into
            if not (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.flags.writeable and out.dtype == rx.dtype
                    and out.shape == (B, n)):
                raise ValueError("into must be a writable C-contiguous [batch][n] array of rx's type")
        f = getattr(_capi.lib(), "ldpc_toolbox_nr_rm_recover_" + ("f64" if rx.dtype == np.float64 else "f32"))
        rc = f(self._h, out.ctypes.data, n, rx.ctypes.data, e, B, int(rv), int(qm), float(filler_llr), int(into is not None))
        if rc != 0:
            self._raise("recover", rc)
        return out

    def match_device(self, in_ptr: int, out_ptr: int, batch: int, e: int, rv: int = 0, qm: int = 1, stream: int = 0, n=None):
        """Raw device pointers (e.g. torch tensors' data_ptr()): codewords [batch][n] -> [batch][e]; stream = hipStream_t
        handle (enqueue and return) or 0 (the handle's own stream, synchronous).  n: given only to state another length
        than the code's (it is refused)."""
        rc = _capi.lib().ldpc_toolbox_nr_rm_match_device(self._h, out_ptr, int(e), in_ptr, self.n if n is None else n, batch,
                                                         int(rv), int(qm), stream or None)
        if rc != 0:
            self._raise("match_device", rc)

    def recover_device(self, rx_ptr: int, llrs_ptr: int, f64: bool, batch: int, e: int, rv: int = 0, qm: int = 1,
                       filler_llr: float = float("inf"), combine: bool = False, stream: int = 0, n=None):
        """Raw device pointers: rx [batch][e] -> llrs [batch][n], floats or (f64) doubles; combine: add into llrs."""
        f = getattr(_capi.lib(), "ldpc_toolbox_nr_rm_recover_" + ("f64" if f64 else "f32") + "_device")
        rc = f(self._h, llrs_ptr, self.n if n is None else n, rx_ptr, int(e), batch, int(rv), int(qm), float(filler_llr),
               int(bool(combine)), stream or None)
        if rc != 0:
            self._raise("recover_device", rc)

    def recover_i8(self, rx, rv: int = 0, qm: int = 1, filler: int = 127, into=None):
        """rx [batch][e] int8 host array of 8-bit soft bits (-128 read as -127) -> soft bits [batch][n] int8: per column the
        saturating sum (to +-127) of its repeats in transmitted order, 0 for a column that was not sent, `filler` (1 .. 127)
        for a filler column.  into: a C-contiguous int8 [batch][n] array holding the soft buffer of earlier transmissions;
        this one is combined into it with saturation and the array returned."""
        rx = np.ascontiguousarray(rx)
        if rx.dtype != np.int8 or rx.ndim != 2:
            raise ValueError("rx must be an int8 array [batch][e]")
        B, e = rx.shape
        n = self.n
        if into is None:
            out = np.zeros((B, n), dtype=np.int8)
        else:
            out = into
            if not (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.flags.writeable and out.dtype == np.int8
                    and out.shape == (B, n)):
                raise ValueError("into must be a writable C-contiguous int8 [batch][n] array")
        rc = _capi.lib().ldpc_toolbox_nr_rm_recover_i8(self._h, out.ctypes.data, n, rx.ctypes.data, e, B, int(rv), int(qm), int(filler),
                                                       int(into is not None))
        if rc != 0:
            self._raise("recover_i8", rc)
        return out

    def recover_i8_device(self, rx_ptr: int, llrs_ptr: int, batch: int, e: int, rv: int = 0, qm: int = 1, filler: int = 127,
                          combine: bool = False, stream: int = 0, n=None):
        """Raw device pointers, any byte addresses: rx [batch][e] -> llrs [batch][n], int8; combine: combine into llrs."""
        rc = _capi.lib().ldpc_toolbox_nr_rm_recover_i8_device(self._h, llrs_ptr, self.n if n is None else n, rx_ptr, int(e), batch, int(rv),
                                                              int(qm), int(filler), int(bool(combine)), stream or None)
        if rc != 0:
            self._raise("recover_i8_device", rc)

    def close(self):
        if getattr(self, "_h", None):
            _capi.lib().ldpc_toolbox_nr_rm_dtor(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
