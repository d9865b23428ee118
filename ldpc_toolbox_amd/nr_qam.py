"""Batched 5G NR modulation mapper, soft demapper and scrambling on the GPU (include/ldpc_toolbox.h, PART 8): QPSK, 16QAM,
64QAM and 256QAM of TS 38.211 5.1.3-5.1.6 with the Gold sequence of 5.2.1.  Bits and LLRs are in transmitted order -- what
`NrRateMatcher.match` / `NrTransportBlock.concatenate` give and `recover` / `split` take.  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _capi
from .decoder import DecoderUnavailable


class NrQam:
    """`NrQam(6)` or `NrQam("nr5g-qam:6")`: QM = 2, 4, 6 or 8 bits per symbol.  A positive LLR means bit 0.  `c_init`: the
    scrambling seed 0 .. 2^31 - 1, or -1 (default) for no scrambling.  The handle needs no GPU until the first run
    (device=None: GPU LDPC_TOOLBOX_DEVICE, default 0)."""

    def __init__(self, qm, device=None):
        spec = qm if isinstance(qm, str) else f"nr5g-qam:{int(qm)}"
        h = _capi.lib().ldpc_toolbox_nr_qam_ctor(spec.encode(), -1 if device is None else int(device))
        if not h:
            raise ValueError(_capi.last_error() or "NR modulation constructor returned NULL")
        self._h = h

    def get(self, key: str) -> int:
        v = C.c_int64(0)
        if _capi.lib().ldpc_toolbox_nr_qam_get(self._h, key.encode(), C.byref(v)) != 0:
            raise KeyError(key)
        return int(v.value)

    bits_per_symbol = property(lambda self: self.get("bits_per_symbol"))
    device = property(lambda self: self.get("device"))

    @property
    def points(self):
        """the 2^QM points, complex128, point V = sum_j b_j << (QM-1-j) at index V"""
        n = self.get("points")
        out = np.zeros(n, dtype=np.complex128)
        if _capi.lib().ldpc_toolbox_nr_qam_points(self._h, out.ctypes.data, 2 * n) != n:
            raise RuntimeError("ldpc_toolbox_nr_qam_points failed")
        return out

    @staticmethod
    def _raise(what, rc):
        msg = f"{what} failed ({rc}): {_capi.last_error()}"
        if rc == -4:
            raise ValueError(msg)
        raise (DecoderUnavailable if "no HIP device" in msg else RuntimeError)(msg)

    def sequence(self, length: int, c_init: int):
        """c(0 .. length-1) of TS 38.211 5.2.1, uint8, as the GPU generates it"""
        out = np.zeros(int(length), dtype=np.uint8)
        rc = _capi.lib().ldpc_toolbox_nr_qam_sequence(self._h, out.ctypes.data, int(length), int(c_init))
        if rc != 0:
            self._raise("sequence", rc)
        return out

    def modulate(self, bits, c_init: int = -1, f64: bool = True):
        """bits [batch][bits_len] uint8 host array (a byte equal to 1 is a one) -> symbols [batch][bits_len / QM]
        complex128 / complex64; bit i of a row is XORed with c(i) first when c_init >= 0."""
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        if bits.ndim != 2:
            raise ValueError("bits must be [batch][bits_len]")
        B, n = bits.shape
        S = n // self.bits_per_symbol
        out = np.zeros((B, S), dtype=np.complex128 if f64 else np.complex64)
        L = _capi.lib()
        fn = L.ldpc_toolbox_nr_qam_mod_f64 if f64 else L.ldpc_toolbox_nr_qam_mod_f32
        rc = fn(self._h, out.ctypes.data, S, bits.ctypes.data, n, B, int(c_init))
        if rc != 0:
            self._raise("modulate", rc)
        return out

    def modulate_device(self, bits_ptr: int, sym_ptr: int, f64: bool, batch: int, bits_len: int, c_init: int = -1,
                        stream: int = 0, symbols_len=None):
        """Raw device pointers (e.g. torch tensors' data_ptr()): bits [batch][bits_len] uint8 -> symbols
        [batch][bits_len / QM]; stream = hipStream_t handle (enqueue and return) or 0 (the handle's own stream,
        synchronous).  symbols_len: given only to state a length other than bits_len / QM (it is refused)."""
        L = _capi.lib()
        fn = L.ldpc_toolbox_nr_qam_mod_f64_device if f64 else L.ldpc_toolbox_nr_qam_mod_f32_device
        S = bits_len // self.bits_per_symbol if symbols_len is None else symbols_len
        rc = fn(self._h, sym_ptr, S, bits_ptr, bits_len, batch, int(c_init), stream or None)
        if rc != 0:
            self._raise("modulate_device", rc)

    def demodulate(self, symbols, sigma, max_log: bool = False, c_init: int = -1):
        """symbols [batch][symbols_len] complex64 / complex128 host array -> LLRs [batch][QM * symbols_len] float32 /
        float64 in transmitted order, descrambled (the LLR of row position i negated where c(i) = 1) when c_init >= 0."""
        symbols = np.asarray(symbols)
        if symbols.ndim != 2:
            raise ValueError("symbols must be [batch][symbols_len]")
        real = np.float32 if symbols.dtype in (np.complex64, np.float32) else np.float64
        symbols = np.ascontiguousarray(symbols, dtype=np.complex64 if real == np.float32 else np.complex128)
        B, S = symbols.shape
        n = S * self.bits_per_symbol
        out = np.zeros((B, n), dtype=real)
        L = _capi.lib()
        fn = L.ldpc_toolbox_nr_qam_demod_f32 if real == np.float32 else L.ldpc_toolbox_nr_qam_demod_f64
        rc = fn(self._h, out.ctypes.data, n, symbols.ctypes.data, S, B, float(sigma), int(bool(max_log)), int(c_init))
        if rc != 0:
            self._raise("demodulate", rc)
        return out

    def demodulate_device(self, sym_ptr: int, out_ptr: int, f64: bool, batch: int, symbols_len: int, sigma, max_log: bool = False,
                          c_init: int = -1, stream: int = 0):
        """Raw device pointers: symbols [batch][symbols_len] -> LLRs [batch][QM * symbols_len]; stream as in
        `modulate_device`.  The symbol buffer must be aligned to one (re, im) pair, the LLR buffer to 16 bytes."""
        L = _capi.lib()
        fn = L.ldpc_toolbox_nr_qam_demod_f64_device if f64 else L.ldpc_toolbox_nr_qam_demod_f32_device
        rc = fn(self._h, out_ptr, symbols_len * self.bits_per_symbol, sym_ptr, symbols_len, batch, float(sigma), int(bool(max_log)),
                int(c_init), stream or None)
        if rc != 0:
            self._raise("demodulate_device", rc)

    def demap_i8(self, symbols, sigma, max_log: bool = False, c_init: int = -1):
        """symbols [batch][symbols_len] complex64 host array -> 8-bit soft bits [batch][QM * symbols_len] int8: each the
        float32 LLR of `demodulate` quantised (round-half-away(8 x) clamped to +-127), in one kernel."""
        symbols = np.asarray(symbols)
        if symbols.ndim != 2:
            raise ValueError("symbols must be [batch][symbols_len]")
        symbols = np.ascontiguousarray(symbols, dtype=np.complex64)
        B, S = symbols.shape
        n = S * self.bits_per_symbol
        out = np.zeros((B, n), dtype=np.int8)
        rc = _capi.lib().ldpc_toolbox_nr_demap_i8(self._h, out.ctypes.data, n, symbols.ctypes.data, S, B, float(sigma), int(bool(max_log)),
                                                  int(c_init))
        if rc != 0:
            self._raise("demap_i8", rc)
        return out

    def demap_i8_device(self, sym_ptr: int, out_ptr: int, batch: int, symbols_len: int, sigma, max_log: bool = False, c_init: int = -1,
                        stream: int = 0):
        """Raw device pointers: float symbols [batch][symbols_len] -> int8 soft bits [batch][QM * symbols_len]; stream as in
        `modulate_device`.  The symbol buffer must be aligned to one (re, im) pair; the output may be any byte address."""
        rc = _capi.lib().ldpc_toolbox_nr_demap_i8_device(self._h, out_ptr, symbols_len * self.bits_per_symbol, sym_ptr, symbols_len, batch,
                                                         float(sigma), int(bool(max_log)), int(c_init), stream or None)
        if rc != 0:
            self._raise("demap_i8_device", rc)

    def _csi_host(self, what, fn, symbols, scale, sym_t, out_t, max_log, c_init):
        symbols = np.asarray(symbols)
        if symbols.ndim != 2:
            raise ValueError("symbols must be [batch][symbols_len]")
        symbols = np.ascontiguousarray(symbols, dtype=sym_t)
        scale = np.ascontiguousarray(scale, dtype=np.float32 if sym_t == np.complex64 else np.float64)
        if scale.shape != symbols.shape:
            raise ValueError("scale must be [batch][symbols_len], one value per symbol")
        B, S = symbols.shape
        n = S * self.bits_per_symbol
        out = np.zeros((B, n), dtype=out_t)
        rc = fn(self._h, out.ctypes.data, n, symbols.ctypes.data, scale.ctypes.data, S, B, int(bool(max_log)), int(c_init))
        if rc != 0:
            self._raise(what, rc)
        return out

    def demodulate_csi(self, symbols, scale, max_log: bool = False, c_init: int = -1):
        """`demodulate` with a scale per symbol in place of sigma (include/ldpc_toolbox.h, PART 10): symbols
        [batch][symbols_len] complex64 / complex128 equalised symbols, scale [batch][symbols_len] = 1 / sigma_s^2, the
        reciprocal of each symbol's noise variance per real coordinate after equalisation -> LLRs [batch][QM * symbols_len]
        float32 / float64.  The scales are used as given: 0 erases a symbol."""
        symbols = np.asarray(symbols)
        f32 = symbols.dtype in (np.complex64, np.float32)
        L = _capi.lib()
        return self._csi_host("demodulate_csi", L.ldpc_toolbox_nr_demap_csi_f32 if f32 else L.ldpc_toolbox_nr_demap_csi_f64, symbols, scale,
                              np.complex64 if f32 else np.complex128, np.float32 if f32 else np.float64, max_log, c_init)

    def demodulate_csi_device(self, sym_ptr: int, scale_ptr: int, out_ptr: int, f64: bool, batch: int, symbols_len: int,
                              max_log: bool = False, c_init: int = -1, stream: int = 0):
        """Raw device pointers: symbols and scale [batch][symbols_len] -> LLRs [batch][QM * symbols_len]; stream as in
        `modulate_device`.  Alignment as in `demodulate_device`; the scale buffer needs only its element's."""
        L = _capi.lib()
        fn = L.ldpc_toolbox_nr_demap_csi_f64_device if f64 else L.ldpc_toolbox_nr_demap_csi_f32_device
        rc = fn(self._h, out_ptr, symbols_len * self.bits_per_symbol, sym_ptr, scale_ptr, symbols_len, batch, int(bool(max_log)), int(c_init),
                stream or None)
        if rc != 0:
            self._raise("demodulate_csi_device", rc)

    def demap_csi_i8(self, symbols, scale, max_log: bool = False, c_init: int = -1):
        """complex64 symbols and float32 scales [batch][symbols_len] -> 8-bit soft bits [batch][QM * symbols_len] int8: each
        the float32 LLR of `demodulate_csi` quantised as in `demap_i8`, in one kernel."""
        return self._csi_host("demap_csi_i8", _capi.lib().ldpc_toolbox_nr_demap_csi_i8, symbols, scale, np.complex64, np.int8, max_log, c_init)

    def demap_csi_i8_device(self, sym_ptr: int, scale_ptr: int, out_ptr: int, batch: int, symbols_len: int, max_log: bool = False,
                            c_init: int = -1, stream: int = 0):
        """Raw device pointers: float symbols and scales [batch][symbols_len] -> int8 soft bits [batch][QM * symbols_len];
        stream as in `modulate_device`.  The output may be any byte address."""
        rc = _capi.lib().ldpc_toolbox_nr_demap_csi_i8_device(self._h, out_ptr, symbols_len * self.bits_per_symbol, sym_ptr, scale_ptr,
                                                             symbols_len, batch, int(bool(max_log)), int(c_init), stream or None)
        if rc != 0:
            self._raise("demap_csi_i8_device", rc)

    def close(self):
        if getattr(self, "_h", None):
            _capi.lib().ldpc_toolbox_nr_qam_dtor(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
