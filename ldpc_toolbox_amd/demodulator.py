"""Batched soft demapper on the GPU (include/ldpc_toolbox.h, PART 4): received symbols -> channel LLRs in codeword
order, the layout `LdpcDecoder.decode_batch_device` takes.  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _capi
from .decoder import DecoderUnavailable


class Demodulator:
    """`Demodulator("8PSK")` ("BPSK", "QPSK", "8PSK": the DVB-S2 mappings), or `Demodulator(points, energy_term)` with
    2^m complex points (m = 1..5), point V carrying the bits of V with the symbol's first bit most significant.
    A positive LLR means bit 0.  The handle needs no GPU until the first run (device=None: GPU LDPC_TOOLBOX_DEVICE, default 0)."""

    def __init__(self, modulation_or_points, energy_term=False, device=None):
        L = _capi.lib()
        dev = -1 if device is None else int(device)
        if isinstance(modulation_or_points, str):
            h = L.ldpc_toolbox_demod_ctor(modulation_or_points.encode(), dev)
        else:
            pts = np.asarray(modulation_or_points)
            if pts.ndim == 2 and pts.shape[1] == 2 and not np.iscomplexobj(pts):
                pts = pts[:, 0] + 1j * pts[:, 1]
            pts = np.ascontiguousarray(pts.reshape(-1), dtype=np.complex128)
            bits = max(int(pts.size).bit_length() - 1, 0)
            if pts.size != 1 << bits:
                raise ValueError("the number of constellation points must be a power of two")
            h = L.ldpc_toolbox_demod_ctor_table(pts.view(np.float64).ctypes.data, bits, int(bool(energy_term)), dev)
        if not h:
            raise ValueError(_capi.last_error() or "demodulator constructor returned NULL")
        self._h = h
        self.real_symbols = modulation_or_points == "BPSK" if isinstance(modulation_or_points, str) else False

    def get(self, key: str) -> int:
        v = C.c_int64(0)
        if _capi.lib().ldpc_toolbox_demod_get(self._h, key.encode(), C.byref(v)) != 0:
            raise KeyError(key)
        return int(v.value)

    bits_per_symbol = property(lambda self: self.get("bits_per_symbol"))
    points = property(lambda self: self.get("points"))
    energy_term = property(lambda self: bool(self.get("energy_term")))
    device = property(lambda self: self.get("device"))

    @staticmethod
    def _raise(what, rc):
        msg = f"{what} failed ({rc}): {_capi.last_error()}"
        if rc == -4:
            raise ValueError(msg)
        raise (DecoderUnavailable if "no HIP device" in msg else RuntimeError)(msg)

    def demodulate(self, symbols, sigma, interleaving=0, max_log=False):
        """symbols [batch][symbols_len]: complex64 / complex128 (float32 / float64 reals for BPSK) host array ->
        LLRs [batch][bits_per_symbol * symbols_len] float32 / float64, deinterleaved (`interleaving`: signed columns)."""
        symbols = np.asarray(symbols)
        if symbols.ndim != 2:
            raise ValueError("symbols must be [batch][symbols_len]")
        if self.real_symbols:
            if np.iscomplexobj(symbols):
                raise ValueError("BPSK symbols are real")
            real = np.float32 if symbols.dtype == np.float32 else np.float64
            symbols = np.ascontiguousarray(symbols, dtype=real)
        else:
            real = np.float32 if symbols.dtype in (np.complex64, np.float32) else np.float64
            symbols = np.ascontiguousarray(symbols, dtype=np.complex64 if real == np.float32 else np.complex128)
        B, S = symbols.shape
        n = S * self.bits_per_symbol
        out = np.zeros((B, n), dtype=real)
        L = _capi.lib()
        fn = L.ldpc_toolbox_demod_run_f32 if real == np.float32 else L.ldpc_toolbox_demod_run_f64
        rc = fn(self._h, out.ctypes.data, n, symbols.ctypes.data, S, B, float(sigma), int(interleaving), int(bool(max_log)))
        if rc != 0:
            self._raise("demodulate", rc)
        return out

    def demodulate_device(self, sym_ptr: int, out_ptr: int, f64: bool, batch: int, symbols_len: int, sigma,
                          interleaving=0, max_log=False, stream: int = 0):
        """Raw device pointers (e.g. torch tensors' data_ptr()): symbols [batch][symbols_len] -> LLRs
        [batch][bits_per_symbol * symbols_len]; stream = hipStream_t handle (enqueue and return) or 0 (the handle's
        own stream, synchronous)."""
        L = _capi.lib()
        fn = L.ldpc_toolbox_demod_run_f64_device if f64 else L.ldpc_toolbox_demod_run_f32_device
        rc = fn(self._h, out_ptr, symbols_len * self.bits_per_symbol, sym_ptr, symbols_len, batch, float(sigma),
                int(interleaving), int(bool(max_log)), stream or None)
        if rc != 0:
            self._raise("demodulate_device", rc)

    def close(self):
        if getattr(self, "_h", None):
            _capi.lib().ldpc_toolbox_demod_dtor(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
