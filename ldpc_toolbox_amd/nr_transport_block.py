"""Batched 5G NR transport block processing on the GPU (include/ldpc_toolbox.h, PART 7; TS 38.212 5.1, 5.2.2, 5.5):
transport block CRC, segmentation into code blocks with CRC24B and filler bits, the CRC verdicts on receive, and code
block concatenation.  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _capi
from .decoder import DecoderUnavailable


def nr_base_graph(a: int, rate: float) -> int:
    """TS 38.212 7.2.2: the LDPC base graph (1 or 2) for payload size `a` at target code rate `rate`"""
    return int(_capi.lib().ldpc_toolbox_nr_base_graph(int(a), float(rate)))


class NrTransportBlock:
    """`NrTransportBlock("nr5g-tb:BG:A")`: base graph and payload bits.  Code block rows are block-major: row
    r * batch + b is block r of transport block b.  Bytes hold one bit each.  The handle needs no GPU until the first
    batched call (device=None: GPU LDPC_TOOLBOX_DEVICE)."""

    def __init__(self, spec: str, device=0):
        L = _capi.lib()
        h = L.ldpc_toolbox_nr_tb_ctor(spec.encode(), -1 if device is None else int(device))
        if not h:
            raise ValueError(_capi.last_error() or "transport block constructor returned NULL")
        self._h = h
        self.spec = spec

    def get(self, key: str) -> int:
        v = C.c_int64(0)
        if _capi.lib().ldpc_toolbox_nr_tb_get(self._h, key.encode(), C.byref(v)) != 0:
            raise KeyError(key)
        return int(v.value)

    a = property(lambda self: self.get("a"))
    base_graph = property(lambda self: self.get("base_graph"))
    tb_crc = property(lambda self: self.get("tb_crc"))
    b = property(lambda self: self.get("b"))
    c = property(lambda self: self.get("c"))
    cb_crc = property(lambda self: self.get("cb_crc"))
    k_prime = property(lambda self: self.get("k_prime"))
    k_b = property(lambda self: self.get("k_b"))
    zc = property(lambda self: self.get("zc"))
    k = property(lambda self: self.get("k"))
    fillers = property(lambda self: self.get("fillers"))
    n = property(lambda self: self.get("n"))
    code_spec = property(lambda self: f"nr5g:{self.base_graph}:{self.zc}", doc="the LDPC code of the blocks")
    rate_match_spec = property(lambda self: f"nr5g:{self.base_graph}:{self.zc}:{self.fillers}", doc="their rate matcher")

    @staticmethod
    def _raise(what, rc):
        msg = f"{what} failed ({rc}): {_capi.last_error()}"
        if rc == -4:
            raise ValueError(msg)
        raise (DecoderUnavailable if "no HIP device" in msg else RuntimeError)(msg)

    def block_lengths(self, g: int, q: int):
        """(e_lo, e_hi, c_lo) of TS 38.212 5.4.2.1: the first c_lo blocks are rate-matched to e_lo bits, the others to e_hi"""
        v = [C.c_uint64(0) for _ in range(3)]
        if min(int(g), int(q)) < 0:
            raise ValueError("g and q must be positive")
        rc = _capi.lib().ldpc_toolbox_nr_tb_block_lengths(self._h, int(g), int(q), *[C.byref(x) for x in v])
        if rc != 0:
            self._raise("block_lengths", rc)
        return tuple(int(x.value) for x in v)

    def segment(self, payload):
        """payload [batch][A] uint8 host array (a byte equal to 1 is a one) -> code blocks [C * batch][K], the encoder's input"""
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        if payload.ndim != 2:
            raise ValueError("payload must be [batch][A]")
        B, a = payload.shape
        k = self.k
        rows = np.zeros((self.c * B, k), dtype=np.uint8)
        rc = _capi.lib().ldpc_toolbox_nr_tb_segment(self._h, rows.ctypes.data, k, payload.ctypes.data, a, B)
        if rc != 0:
            self._raise("segment", rc)
        return rows

    def desegment(self, rows):
        """hard decisions [C * batch][K] -> (payload [batch][A], tb_ok [batch], cb_ok [batch][C]), uint8"""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        c = self.c
        if rows.ndim != 2 or rows.shape[0] % c != 0:
            raise ValueError("rows must be [C * batch][K]")
        B, a = rows.shape[0] // c, self.a
        payload = np.zeros((B, a), dtype=np.uint8)
        tb_ok = np.zeros(B, dtype=np.uint8)
        cb_ok = np.zeros((B, c), dtype=np.uint8)
        rc = _capi.lib().ldpc_toolbox_nr_tb_desegment(self._h, payload.ctypes.data, a, tb_ok.ctypes.data, cb_ok.ctypes.data,
                                                      rows.ctypes.data, rows.shape[1], B)
        if rc != 0:
            self._raise("desegment", rc)
        return payload, tb_ok, cb_ok

    def concatenate(self, packed, g: int, q: int):
        """packed: flat uint8 host array of batch * g bytes -- c_lo * batch rows of e_lo, then (C - c_lo) * batch rows of
        e_hi, block-major -> [batch][g]"""
        packed = np.ascontiguousarray(packed, dtype=np.uint8).reshape(-1)
        g = int(g)
        if g < 1 or packed.size % g != 0:
            raise ValueError("packed must hold batch * g bytes")
        B = packed.size // g
        out = np.zeros((B, g), dtype=np.uint8)
        rc = _capi.lib().ldpc_toolbox_nr_tb_concatenate(self._h, out.ctypes.data, g, packed.ctypes.data, max(int(q), 0), B)
        if rc != 0:
            self._raise("concatenate", rc)
        return out

    def split(self, rx, q: int):
        """rx [batch][g] float32 or float64 host array -> flat packed array of the same type, in concatenate's layout"""
        rx = np.ascontiguousarray(rx)
        if rx.dtype not in (np.float32, np.float64):
            rx = rx.astype(np.float32)
        if rx.ndim != 2:
            raise ValueError("rx must be [batch][g]")
        B, g = rx.shape
        out = np.zeros(B * g, dtype=rx.dtype)
        f = getattr(_capi.lib(), "ldpc_toolbox_nr_tb_split_" + ("f64" if rx.dtype == np.float64 else "f32"))
        rc = f(self._h, out.ctypes.data, rx.ctypes.data, g, max(int(q), 0), B)
        if rc != 0:
            self._raise("split", rc)
        return out

    def segment_device(self, payload_ptr: int, rows_ptr: int, batch: int, stream: int = 0):
        """Raw device pointers (e.g. torch tensors' data_ptr()): payload [batch][A] -> rows [C * batch][K]; stream =
        hipStream_t handle (enqueue and return) or 0 (the handle's own stream, synchronous)."""
        rc = _capi.lib().ldpc_toolbox_nr_tb_segment_device(self._h, rows_ptr, self.k, payload_ptr, self.a, batch, stream or None)
        if rc != 0:
            self._raise("segment_device", rc)

    def desegment_device(self, rows_ptr: int, payload_ptr: int, tb_ok_ptr: int, cb_ok_ptr: int, batch: int, stream: int = 0):
        """Raw device pointers: rows [C * batch][K] -> payload [batch][A], tb_ok [batch], cb_ok [batch][C] (0: not wanted)"""
        rc = _capi.lib().ldpc_toolbox_nr_tb_desegment_device(self._h, payload_ptr, self.a, tb_ok_ptr, cb_ok_ptr or None, rows_ptr, self.k,
                                                             batch, stream or None)
        if rc != 0:
            self._raise("desegment_device", rc)

    def concatenate_device(self, packed_ptr: int, out_ptr: int, batch: int, g: int, q: int, stream: int = 0):
        """Raw device pointers: packed block-major rows -> [batch][g]"""
        rc = _capi.lib().ldpc_toolbox_nr_tb_concatenate_device(self._h, out_ptr, int(g), packed_ptr, int(q), batch, stream or None)
        if rc != 0:
            self._raise("concatenate_device", rc)

    def split_device(self, rx_ptr: int, packed_ptr: int, f64: bool, batch: int, g: int, q: int, stream: int = 0):
        """Raw device pointers: rx [batch][g], floats or (f64) doubles -> packed block-major rows"""
        f = getattr(_capi.lib(), "ldpc_toolbox_nr_tb_split_" + ("f64" if f64 else "f32") + "_device")
        rc = f(self._h, packed_ptr, rx_ptr, int(g), int(q), batch, stream or None)
        if rc != 0:
            self._raise("split_device", rc)

    def close(self):
        if getattr(self, "_h", None):
            _capi.lib().ldpc_toolbox_nr_tb_dtor(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
