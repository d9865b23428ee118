"""The 5G NR link handle on the GPU (include/ldpc_toolbox.h, PART 11): one shared-channel configuration, payload to symbols
and symbols to payload in one call each, with HARQ soft buffers that stay on the device and a decoder that runs only on the
code blocks that have not passed their CRC.  It is defined by the composition of `NrTransportBlock`, `Encoder`,
`NrRateMatcher`, `NrQam` and `LdpcDecoder`.  With soft_bits=8 (PART 12) the soft bits are one byte each from the demapper
through the slots to the decoder input, by the composition of the stages' 8-bit entries.  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _capi
from .decoder import DecoderUnavailable


class NrLink:
    """`NrLink("nr5g-link:BG:A:G:QM[:NL]", "Minsumf32", slots)`: base graph, payload bits, coded bits per transmission, bits
    per symbol and layers; the decoder implementation; the number of HARQ slots.  Transport block b of a receive call lives
    in slot first_slot + b.  Bytes hold one bit each.  The handle needs no GPU until the first batched call (device=None: GPU
    LDPC_TOOLBOX_DEVICE).  soft_bits=8: the HARQ slots hold 8-bit soft bits (an 8-bit implementation only; ValueError
    otherwise); 32, the default: floats."""

    def __init__(self, spec: str, implementation: str, slots: int, device=0, soft_bits: int = 32):
        if not 0 <= int(slots) < 2 ** 32:
            raise ValueError("slots must be 1 .. 2^32 - 1")
        h = _capi.lib().ldpc_toolbox_nr_link_ctor(spec.encode(), str(implementation).encode(), int(slots), -1 if device is None else int(device))
        if not h:
            raise ValueError(_capi.last_error() or "link constructor returned NULL")
        self._h = h
        self.spec = spec
        try:
            self.set("soft_bits", soft_bits)
        except Exception:
            self.close()
            raise

    def get(self, key: str) -> int:
        v = C.c_int64(0)
        if _capi.lib().ldpc_toolbox_nr_link_get(self._h, key.encode(), C.byref(v)) != 0:
            raise KeyError(key)
        return int(v.value)

    def set(self, key: str, value: int):
        """"max_log" (0 / 1), "pass_elements" (elements per launch of the fused recover kernel) or "soft_bits" (8 / 32, before
        the first batched call)"""
        rc = _capi.lib().ldpc_toolbox_nr_link_set(self._h, key.encode(), int(value))
        if rc != 0:
            self._raise("set", rc)

    def set_filler_llr(self, value: float):
        """the LLR of the filler columns in the soft rows: positive, +inf (the default) allowed; an 8-bit handle writes its
        quantised value, which must not be 0"""
        rc = _capi.lib().ldpc_toolbox_nr_link_set_filler_llr(self._h, float(value))
        if rc != 0:
            self._raise("set_filler_llr", rc)

    a = property(lambda self: self.get("a"))
    base_graph = property(lambda self: self.get("base_graph"))
    c = property(lambda self: self.get("c"))
    k_prime = property(lambda self: self.get("k_prime"))
    zc = property(lambda self: self.get("zc"))
    k = property(lambda self: self.get("k"))
    fillers = property(lambda self: self.get("fillers"))
    n = property(lambda self: self.get("n"))
    g = property(lambda self: self.get("g"))
    qm = property(lambda self: self.get("qm"))
    layers = property(lambda self: self.get("layers"))
    q = property(lambda self: self.get("q"))
    symbols = property(lambda self: self.get("symbols"), doc="complex symbols per transmission, G / QM")
    slots = property(lambda self: self.get("slots"))
    soft_bits = property(lambda self: self.get("soft_bits"), doc="8: the slots hold 8-bit soft bits; 32: floats")
    soft_bytes = property(lambda self: self.get("soft_bytes"), doc="bytes of the slots' soft rows, C * slots * n * (soft_bits / 8)")
    block_lengths = property(lambda self: (self.get("e_lo"), self.get("e_hi"), self.get("c_lo")),
                             doc="(e_lo, e_hi, c_lo): the first c_lo blocks are rate-matched to e_lo bits, the others to e_hi")
    decoded_rows = property(lambda self: self.get("decoded_rows"), doc="code blocks the last receive call gave to the decoder")
    skipped_rows = property(lambda self: self.get("skipped_rows"), doc="code blocks it left alone: they were done")
    device = property(lambda self: self.get("device"))

    @staticmethod
    def _raise(what, rc):
        msg = f"{what} failed ({rc}): {_capi.last_error()}"
        if rc == -4:
            raise ValueError(msg)
        raise (DecoderUnavailable if "no HIP device" in msg else RuntimeError)(msg)

    def transmit(self, payload, rv: int = 0, c_init: int = -1):
        """payload [batch][A] uint8 host array -> symbols [batch][G / QM] complex64: segmentation, encoding, rate matching
        with `rv`, concatenation, scrambling with `c_init` (-1: none) and mapping"""
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        if payload.ndim != 2:
            raise ValueError("payload must be [batch][A]")
        B, a = payload.shape
        S = self.symbols
        out = np.zeros((B, S), dtype=np.complex64)
        rc = _capi.lib().ldpc_toolbox_nr_link_transmit_f32(self._h, out.ctypes.data, S, payload.ctypes.data, a, B, int(rv), int(c_init))
        if rc != 0:
            self._raise("transmit", rc)
        return out

    def receive(self, symbols, sigma=None, scale=None, rv: int = 0, c_init: int = -1, first_slot: int = 0, combine: bool = False,
                max_iterations: int = 30):
        """symbols [batch][G / QM] complex64 host array -> (payload [batch][A], tb_ok [batch], cb_ok [batch][C], uint8;
        iterations [batch][C] int32, -1 = not decoded), through the slots first_slot .. first_slot + batch - 1.  `sigma`: the
        noise per real coordinate, or `scale` [batch][G / QM] float32: 1 / sigma_s^2 per symbol (`NrQam.demodulate_csi`).
        combine=False is a first transmission: it resets the slots.  combine=True adds this transmission to the soft rows of
        the code blocks that have not passed their CRC and decodes those alone."""
        symbols = np.asarray(symbols)
        if symbols.ndim != 2:
            raise ValueError("symbols must be [batch][G / QM]")
        symbols = np.ascontiguousarray(symbols, dtype=np.complex64)
        B, S = symbols.shape
        if scale is not None:
            scale = np.ascontiguousarray(scale, dtype=np.float32)
            if scale.shape != symbols.shape:
                raise ValueError("scale must be [batch][G / QM], one value per symbol")
        elif sigma is None:
            raise ValueError("give sigma or scale")
        a, c = self.a, self.c
        payload = np.zeros((B, a), dtype=np.uint8)
        tb_ok = np.zeros(B, dtype=np.uint8)
        cb_ok = np.zeros((B, c), dtype=np.uint8)
        its = np.zeros((B, c), dtype=np.int32)
        rc = _capi.lib().ldpc_toolbox_nr_link_receive_f32(
            self._h, payload.ctypes.data, a, tb_ok.ctypes.data, cb_ok.ctypes.data, its.ctypes.data, symbols.ctypes.data,
            None if scale is None else scale.ctypes.data, S, B, 0.0 if sigma is None else float(sigma), int(rv), int(c_init), int(first_slot),
            int(bool(combine)), int(max_iterations))
        if rc != 0:
            self._raise("receive", rc)
        return payload, tb_ok, cb_ok, its

    def slot_state(self, first_slot: int = 0, batch=None):
        """host copies of the slots first_slot .. first_slot + batch - 1 (default: all behind first_slot): (soft rows
        [C * batch][n] float32, or int8 on an 8-bit handle, done flags [batch][C], kept hard decisions [C * batch][K]); the
        rows are block-major, row r * batch + b is block r of slot first_slot + b"""
        B = self.slots - int(first_slot) if batch is None else int(batch)
        if B < 0:
            raise ValueError("first_slot is above the handle's slots")
        c = self.c
        i8 = self.soft_bits == 8
        soft = np.zeros((c * B, self.n), dtype=np.int8 if i8 else np.float32)
        done = np.zeros((B, c), dtype=np.uint8)
        rows = np.zeros((c * B, self.k), dtype=np.uint8)
        L = _capi.lib()
        entry = L.ldpc_toolbox_nr_harq_slots_state_i8 if i8 else L.ldpc_toolbox_nr_link_slot_state
        rc = entry(self._h, soft.ctypes.data, done.ctypes.data, rows.ctypes.data, int(first_slot), B)
        if rc != 0:
            self._raise("slot_state", rc)
        return soft, done, rows

    def transmit_device(self, payload_ptr: int, sym_ptr: int, batch: int, rv: int = 0, c_init: int = -1, stream: int = 0):
        """Raw device pointers (e.g. torch tensors' data_ptr()): payload [batch][A] uint8 -> symbols [batch][G / QM] (re, im)
        floats; stream = hipStream_t handle (enqueue and return) or 0 (the handle's own stream, synchronous)."""
        rc = _capi.lib().ldpc_toolbox_nr_link_transmit_f32_device(self._h, sym_ptr, self.symbols, payload_ptr, self.a, batch, int(rv), int(c_init),
                                                                  stream or None)
        if rc != 0:
            self._raise("transmit_device", rc)

    def receive_device(self, sym_ptr: int, payload_ptr: int, tb_ok_ptr: int, cb_ok_ptr: int, its_ptr: int, batch: int, sigma=None,
                       scale_ptr: int = 0, rv: int = 0, c_init: int = -1, first_slot: int = 0, combine: bool = False, max_iterations: int = 30,
                       stream: int = 0):
        """Raw device pointers: symbols [batch][G / QM] -> payload [batch][A], tb_ok [batch], cb_ok and iterations
        [batch][C] (0: not wanted); scale_ptr: float32 [batch][G / QM] in place of sigma.  stream as in `transmit_device`;
        with combine=True the call waits once for the stream, to learn how many code blocks it has to decode."""
        rc = _capi.lib().ldpc_toolbox_nr_link_receive_f32_device(
            self._h, payload_ptr, self.a, tb_ok_ptr, cb_ok_ptr or None, its_ptr or None, sym_ptr, scale_ptr or None, self.symbols, batch,
            0.0 if sigma is None else float(sigma), int(rv), int(c_init), int(first_slot), int(bool(combine)), int(max_iterations), stream or None)
        if rc != 0:
            self._raise("receive_device", rc)

    def recover_device(self, rx_ptr: int, batch: int, rv: int = 0, first_slot: int = 0, combine: bool = False, stream: int = 0):
        """Raw device pointer: LLRs [batch][G] float32 in transmitted order (a demapper's output) -> the slots' soft rows, by
        the fused de-concatenation and rate recovery kernel; nothing is decoded"""
        rc = _capi.lib().ldpc_toolbox_nr_link_recover_f32_device(self._h, rx_ptr, self.g, batch, int(rv), int(first_slot), int(bool(combine)),
                                                                 stream or None)
        if rc != 0:
            self._raise("recover_device", rc)

    def recover_i8_device(self, rx_ptr: int, batch: int, rv: int = 0, first_slot: int = 0, combine: bool = False, stream: int = 0):
        """`recover_device` of an 8-bit handle: soft bits [batch][G] int8 in transmitted order, at any byte address (-128 reads
        as -127) -> the slots' int8 soft rows; RuntimeError on a float handle, as `recover_device` on an 8-bit one"""
        rc = _capi.lib().ldpc_toolbox_nr_harq_slots_recover_i8_device(self._h, rx_ptr, self.g, batch, int(rv), int(first_slot),
                                                                      int(bool(combine)), stream or None)
        if rc != 0:
            self._raise("recover_i8_device", rc)

    def close(self):
        if getattr(self, "_h", None):
            _capi.lib().ldpc_toolbox_nr_link_dtor(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
