"""Numpy restatement of the 8-bit min-sum family, the reference of tests/test_minsum_i8*.py.

Names: [HL]Minsumi8[Norm|Offset][Jones][PartialHardLimit][Deg1Clip][:value].  The arithmetic is
independent_restatement.I8Arithmetic -- the quantiser clamp(round_half_away(8 llr), +-127), i16 variable sums, clip to +-127,
Jones / PartialHardLimit / Deg1Clip, the hard decision llr <= 0, the layered update Q += new - old on inputs clip(Q - R) --
with ONE line changed: the fold step  max(min(x, y) - lookup(|x - y|), 0)  becomes  min(x, y).  So edge i of a check row
gets the magnitude m_i = min over the other edges of |x_j| and the sign parity of x_j < 0 over the other edges, and then,
in integers,

    Norm:   c = (a * m + 8) >> 4,  a = 16 * value in 1..16 (default value 0.75, a = 12)
    Offset: c = max(m - b, 0),     b =  8 * value in 0..127 (default value 0.5, b = 4)
    plain:  c = m

the message is -c for odd parity, else c (zero stays zero), and PartialHardLimit applies to that signed value.

  * MinsumI8      the definition, literally: the O(d^2) fold per excluded edge (I8Arithmetic._minstar_all without the lookup
                  term), then the correction, the sign, the hard limit;
  * MinsumI8Fast  the closed form (min1, min2, first argmin) for the larger cases; test_minsum_i8.py shows the two equal.

Both are driven by independent_restatement._flooding / _layered.  The quantiser maps NaN to 0 (Rust's `as` cast), which
I8Arithmetic leaves to numpy's undefined float -> int conversion: stated here.
"""
import re

import numpy as np

import independent_restatement as ir

_NAME = re.compile(r"(HL)?Minsumi8(Norm|Offset)?(Jones)?(PartialHardLimit)?(Deg1Clip)?(?::([0-9]+(?:\.[0-9]+)?))?")
DEFAULTS = {"Norm": 0.75, "Offset": 0.5}
SCALE = {"Norm": 16, "Offset": 8}
RANGE = {"Norm": (1, 16), "Offset": (0, 127)}


def parse(name):
    """-> (layered, kind or None, integer a / b (0 for plain), jones, hardlimit, deg1clip); ValueError for anything that is
    not a valid 8-bit min-sum name"""
    m = _NAME.fullmatch(name)
    if not m:
        raise ValueError("invalid decoder implementation")
    layered, kind, jones, hard, deg1, value = m.groups()
    if layered and (jones or deg1):
        raise ValueError("invalid decoder implementation")       # as the reference's layered i8 names
    if kind is None:
        if value is not None:
            raise ValueError("invalid decoder implementation")
        return bool(layered), None, 0, bool(jones), bool(hard), bool(deg1)
    scaled = (float(value) if value is not None else DEFAULTS[kind]) * SCALE[kind]
    lo, hi = RANGE[kind]
    if scaled != np.floor(scaled) or not lo <= scaled <= hi:
        raise ValueError("invalid decoder implementation")
    return bool(layered), kind, int(scaled), bool(jones), bool(hard), bool(deg1)


class MinsumI8(ir.I8Arithmetic):
    def __init__(self, kind, value_int, jones, hardlimit, deg1clip):
        super().__init__(False, jones, hardlimit, deg1clip)
        self.kind, self.value_int = kind, value_int

    def input_llr_quantize(self, llr):
        llr = np.asarray(llr, dtype=np.float64)
        return super().input_llr_quantize(np.where(np.isnan(llr), 0.0, llr))

    def correct(self, m):
        if self.kind == "Norm":
            return (self.value_int * m + 8) >> 4
        if self.kind == "Offset":
            return np.maximum(m - self.value_int, 0)
        return m

    def _minstar_all(self, x):                       # I8Arithmetic._minstar_all with the lookup term removed
        B, d = x.shape
        if d < 2:
            raise ValueError("only one variable message connected to check node")
        out = np.empty_like(x)
        for i in range(d):
            sign = np.zeros(B, dtype=bool)
            acc = None
            for j in range(d):
                if j == i:
                    continue
                v = x[:, j]
                sign ^= v < 0
                v = np.abs(v)
                acc = v if acc is None else np.minimum(v, acc)
            c = self.correct(acc)
            out[:, i] = self._hl(np.where(sign, -c, c))
        return out


class MinsumI8Fast(MinsumI8):
    """min1 / min2 / FIRST argmin: edge i gets min2 when it is the argmin and min1 otherwise"""
    def _minstar_all(self, x):
        B, d = x.shape
        if d < 2:
            raise ValueError("only one variable message connected to check node")
        a = np.abs(x)
        arg = a.argmin(axis=1)                       # the first of equal minima
        rows = np.arange(B)
        min1 = a[rows, arg]
        rest = a.copy()
        rest[rows, arg] = 1 << 20
        min2 = rest.min(axis=1)
        c1, c2 = self.correct(min1), self.correct(min2)
        neg = x < 0
        total = np.logical_xor.reduce(neg, axis=1)
        mag = np.where(np.arange(d)[None, :] == arg[:, None], c2[:, None], c1[:, None])
        return self._hl(np.where(total[:, None] ^ neg, -mag, mag)).astype(x.dtype)


def build(name, fast=True):
    layered, kind, value_int, jones, hard, deg1 = parse(name)
    return (MinsumI8Fast if fast else MinsumI8)(kind, value_int, jones, hard, deg1), layered


def decode(alist, name, llrs, max_iterations, fast=True):
    """llrs [B][n] (depunctured) -> (bits [B][n] u8, iterations [B] i32 with -1 = failed, posterior [B][n] f64 in quantiser
    units: the clipped i8 value, as the existing i8 names return it)"""
    A, layered = build(name, fast)
    return decode_with(A, layered, alist, llrs, max_iterations)


def decode_with(A, layered, alist, llrs, max_iterations):
    """independent_restatement.decode for an arithmetic object; a frame that passes the pre-check on the raw input (0
    iterations) has no decoder state: its posterior is stated as the quantised input, which is what the library returns"""
    rows, cols = ir.from_alist(alist)
    llrs = np.ascontiguousarray(llrs, dtype=np.float64)
    raw_hard = llrs <= 0.0
    done = ir.check_llrs(rows, raw_hard)
    iters = np.where(done, 0, -1).astype(np.int32)
    bits = raw_hard.astype(np.uint8)
    with np.errstate(all="ignore"):
        inp = A.input_llr_quantize(llrs)
        final, it_done, bits_run = (ir._layered if layered else ir._flooding)(A, rows, cols, inp, max_iterations, ~done)
    run = ~done
    iters[run] = it_done[run]
    bits[run] = bits_run[run]
    out_llr = np.asarray(final, dtype=np.float64)
    out_llr[done] = inp[done]
    return bits, iters, out_llr
