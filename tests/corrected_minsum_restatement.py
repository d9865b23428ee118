"""Numpy restatement of normalized and offset min-sum, the reference of tests/test_corrected_minsum*.py.

The rule (include/ldpc_toolbox.h): with m_i the magnitude plain Minsum sends on edge i -- the fold from
+inf with the NaN-ignoring minimum over the OTHER edges' |x_j| -- and s_i the parity of x_j < 0 over the other edges,

    normalized:  c_i = alpha * m_i                 offset:  c_i = max(m_i - beta, 0)

in the decoder's type, each result rounded once, and the message is c_i with the sign bit set iff s_i.  Everything else is
the Minsum decoder of independent_restatement.py, whose _flooding / _layered drive the classes below.

  * CorrectedMinsum      the definition, literally: the O(d^2) fold per excluded edge, then one of the two formulas
                         (or, with combined=True, the single form max(alpha * m - beta, 0) the kernels evaluate);
  * CorrectedMinsumFast  the closed form (min1, min2, first argmin) for the larger cases; test_corrected_minsum.py shows it
                         equal to the literal one bit for bit, signs of zero included.
"""
import re

import numpy as np

import independent_restatement as ir

_NAME = re.compile(r"(HL)?(Norm|Offset)Minsumf(32|64)(?::([0-9]+(?:\.[0-9]+)?))?")
DEFAULTS = {"Norm": 0.75, "Offset": 0.5}


def parse(name):
    """-> (layered, kind, dtype, value); ValueError for anything that is not a valid normalized / offset min-sum name"""
    m = _NAME.fullmatch(name)
    if not m:
        raise ValueError("invalid decoder implementation")
    kind = m.group(2)
    value = float(m.group(4)) if m.group(4) is not None else DEFAULTS[kind]
    if not np.isfinite(value) or (kind == "Norm" and not 0.0 < value <= 1.0):
        raise ValueError("invalid decoder implementation")
    return m.group(1) is not None, kind, (np.float64 if m.group(3) == "64" else np.float32), value


class CorrectedMinsum(ir.Minsum):
    def __init__(self, f, kind, value, combined=False):
        super().__init__(f, start="inf")
        self.kind, self.combined = kind, combined
        self.value = f(value)                        # decimal -> double -> the decoder's type, once

    def correct(self, m):
        f = self.f
        if self.combined:
            alpha = self.value if self.kind == "Norm" else f(1.0)
            beta = self.value if self.kind == "Offset" else f(0.0)
            return np.maximum((alpha * m).astype(f) - beta, f(0.0)).astype(f)
        if self.kind == "Norm":
            return (self.value * m).astype(f)
        return np.maximum((m - self.value).astype(f), f(0.0)).astype(f)

    def _all(self, x):
        B, d = x.shape
        if d < 2:
            raise ValueError("only one variable message connected to check node")
        out = np.empty_like(x)
        for i in range(d):
            sign = np.zeros(B, dtype=bool)
            acc = np.full(B, np.inf, dtype=self.f)
            for j in range(d):
                if j == i:
                    continue
                v = x[:, j]
                sign ^= v < 0
                acc = np.fmin(np.abs(v), acc)
            c = self.correct(acc)
            out[:, i] = np.where(sign, -c, c)
        return out


class CorrectedMinsumFast(CorrectedMinsum):
    """min1 / min2 / FIRST argmin: edge i gets min2 when it is the argmin and min1 otherwise -- the minimum over the other
    edges either way; a NaN magnitude never is a minimum (fmin), so it counts as +inf here."""
    def _all(self, x):
        B, d = x.shape
        if d < 2:
            raise ValueError("only one variable message connected to check node")
        a = np.abs(x)
        a = np.where(np.isnan(a), np.inf, a).astype(self.f)
        arg = a.argmin(axis=1)
        rows = np.arange(B)
        min1 = a[rows, arg]
        rest = a.copy()
        rest[rows, arg] = np.inf
        min2 = rest.min(axis=1)
        c1, c2 = self.correct(min1), self.correct(min2)
        neg = x < 0
        total = np.logical_xor.reduce(neg, axis=1)
        mag = np.where(np.arange(d)[None, :] == arg[:, None], c2[:, None], c1[:, None])
        return np.where(total[:, None] ^ neg, -mag, mag).astype(self.f)


def decode(alist, name, llrs, max_iterations, fast=True, combined=False):
    """independent_restatement.decode for a normalized / offset min-sum name: llrs [B][n] (depunctured) ->
    (bits [B][n] u8, iterations [B] i32 with -1 = failed, final LLRs [B][n] f64)"""
    layered, kind, f, value = parse(name)
    A = (CorrectedMinsumFast if fast else CorrectedMinsum)(f, kind, value, combined)
    return decode_with(A, layered, alist, llrs, max_iterations)


def decode_with(A, layered, alist, llrs, max_iterations):
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
    out_llr[done] = llrs[done]
    return bits, iters, out_llr


def same(a, b):
    """bit equality of two float arrays: values (NaN == NaN) and the sign of every zero"""
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))
