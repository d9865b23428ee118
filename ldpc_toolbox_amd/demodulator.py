"""Batched soft demapper on the GPU (include/ldpc_toolbox.h, PART 4): received symbols -> channel LLRs in codeword
order, the layout `LdpcDecoder.decode_batch_device` takes -- and, on the same constellation handle, the transmit side:
the modulator (bits -> symbols) and the AWGN channel.  There is no CPU fallback."""
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

    def modulate(self, bits, interleaving=0, f64=True):
        """bits [batch][bits_len] uint8 host array (a byte equal to 1 is a one) -> symbols [batch][bits_len / m]
        complex128 / complex64 (float64 / float32 reals for BPSK), the bits interleaved first (`interleaving`: signed
        columns, the interleaver `demodulate` undoes)."""
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        if bits.ndim != 2:
            raise ValueError("bits must be [batch][bits_len]")
        B, n = bits.shape
        m = self.bits_per_symbol
        S = n // m
        if self.real_symbols:
            out = np.zeros((B, S), dtype=np.float64 if f64 else np.float32)
        else:
            out = np.zeros((B, S), dtype=np.complex128 if f64 else np.complex64)
        L = _capi.lib()
        fn = L.ldpc_toolbox_mod_run_f64 if f64 else L.ldpc_toolbox_mod_run_f32
        rc = fn(self._h, out.ctypes.data, S, bits.ctypes.data, n, B, int(interleaving))
        if rc != 0:
            self._raise("modulate", rc)
        return out

    def modulate_device(self, bits_ptr: int, sym_ptr: int, f64: bool, batch: int, bits_len: int, interleaving=0,
                        stream: int = 0, symbols_len=None):
        """Raw device pointers: bits [batch][bits_len] uint8 -> symbols [batch][bits_len / m]; stream as in
        `demodulate_device`.  symbols_len: given only to state a length other than bits_len / m (it is refused)."""
        L = _capi.lib()
        fn = L.ldpc_toolbox_mod_run_f64_device if f64 else L.ldpc_toolbox_mod_run_f32_device
        S = bits_len // self.bits_per_symbol if symbols_len is None else symbols_len
        rc = fn(self._h, sym_ptr, S, bits_ptr, bits_len, batch, int(interleaving), stream or None)
        if rc != 0:
            self._raise("modulate_device", rc)

    def add_noise(self, symbols, sigma, seed, first_frame=0):
        """symbols [batch][symbols_len] (dtype rules of `demodulate`) -> a new array: row r with the noise of frame
        first_frame + r (the simulator's Philox4x32-10 + polar method, keyed by seed, frame and symbol)."""
        symbols = np.asarray(symbols)
        if symbols.ndim != 2:
            raise ValueError("symbols must be [batch][symbols_len]")
        if self.real_symbols:
            if np.iscomplexobj(symbols):
                raise ValueError("BPSK symbols are real")
            real = np.float32 if symbols.dtype == np.float32 else np.float64
            out = np.array(symbols, dtype=real, order="C")
        else:
            real = np.float32 if symbols.dtype in (np.complex64, np.float32) else np.float64
            out = np.array(symbols, dtype=np.complex64 if real == np.float32 else np.complex128, order="C")
        B, S = out.shape
        L = _capi.lib()
        fn = L.ldpc_toolbox_awgn_run_f32 if real == np.float32 else L.ldpc_toolbox_awgn_run_f64
        rc = fn(self._h, out.ctypes.data, S, B, float(sigma), int(seed), int(first_frame))
        if rc != 0:
            self._raise("add_noise", rc)
        return out

    def add_noise_device(self, sym_ptr: int, f64: bool, batch: int, symbols_len: int, sigma, seed, first_frame=0,
                         stream: int = 0):
        """Raw device pointer: symbols [batch][symbols_len], noise added in place; stream as in `demodulate_device`."""
        L = _capi.lib()
        fn = L.ldpc_toolbox_awgn_run_f64_device if f64 else L.ldpc_toolbox_awgn_run_f32_device
        rc = fn(self._h, sym_ptr, symbols_len, batch, float(sigma), int(seed), int(first_frame), stream or None)
        if rc != 0:
            self._raise("add_noise_device", rc)

    def add_fading(self, symbols, sigma, block, seed, first_frame=0):
        """symbols [batch][symbols_len] complex64 / complex128 -> (equalised symbols, scale): Rayleigh block fading with
        perfect CSI behind a one-tap equaliser, one gain per `block` consecutive symbols of a frame (block >= symbols_len:
        quasi-static); row r is frame first_frame + r, its noise that of `add_noise`.  scale [batch][symbols_len] float32 /
        float64 is each symbol's 1 / sigma_e^2 -- what `NrQam.demodulate_csi` takes.  Complex handles only."""
        symbols = np.asarray(symbols)
        if symbols.ndim != 2:
            raise ValueError("symbols must be [batch][symbols_len]")
        real = np.float32 if symbols.dtype in (np.complex64, np.float32) else np.float64
        out = np.array(symbols, dtype=np.complex64 if real == np.float32 else np.complex128, order="C")
        scale = np.zeros(out.shape, dtype=real)
        B, S = out.shape
        L = _capi.lib()
        fn = L.ldpc_toolbox_fading_run_f32 if real == np.float32 else L.ldpc_toolbox_fading_run_f64
        rc = fn(self._h, out.ctypes.data, scale.ctypes.data, S, B, float(sigma), int(block), int(seed), int(first_frame))
        if rc != 0:
            self._raise("add_fading", rc)
        return out, scale

    def add_fading_device(self, sym_ptr: int, scale_ptr: int, f64: bool, batch: int, symbols_len: int, sigma, block, seed,
                          first_frame=0, stream: int = 0):
        """Raw device pointers: symbols [batch][symbols_len] equalised in place, scale [batch][symbols_len] written; stream
        as in `demodulate_device`.  The symbol buffer must be aligned to one (re, im) pair."""
        L = _capi.lib()
        fn = L.ldpc_toolbox_fading_run_f64_device if f64 else L.ldpc_toolbox_fading_run_f32_device
        rc = fn(self._h, sym_ptr, scale_ptr, symbols_len, batch, float(sigma), int(block), int(seed), int(first_frame), stream or None)
        if rc != 0:
            self._raise("add_fading_device", rc)

    def close(self):
        if getattr(self, "_h", None):
            _capi.lib().ldpc_toolbox_demod_dtor(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
