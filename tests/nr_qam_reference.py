"""Numpy restatement of the 5G NR modulation mapper, soft demapper and scrambling -- TEST INFRASTRUCTURE ONLY.

Written from the definition in include/ldpc_toolbox.h (PART 8) and from 3GPP TS 38.211 5.1.3-5.1.6 (the mappings) and 5.2.1
(the sequence).  It shares nothing with ldpc_toolbox_amd/csrc: the Gold sequence is the literal serial LFSR, 1600 + len
steps; the levels are built by the nested form as written; arrays are vectorised over symbols here, one thread per symbol
there.

exp / ln_1p are the platform libm's (independent_restatement.m_exp / m_ln_1p, as in demod_restatement.py); numpy's
elementwise *, +, - round once each: no fused multiply-add.  The noise is channel_restatement's.
"""
import numpy as np

import channel_restatement as cr
from independent_restatement import m_exp, m_ln_1p

NORM = {2: 2.0, 4: 10.0, 6: 42.0, 8: 170.0}


def levels(h):
    """L_u, u < 2^h: (1 - 2 a_0) [2^(h-1) - (1 - 2 a_1) [2^(h-2) - ... (1 - 2 a_(h-1)) [1]]], a_0 the top bit of u"""
    out = []
    for u in range(1 << h):
        a = [(u >> (h - 1 - t)) & 1 for t in range(h)]
        inner = 1
        for t in range(h - 1, -1, -1):
            inner = (1 - 2 * a[t]) * (inner if t == h - 1 else (1 << (h - 1 - t)) - inner)
        out.append(inner)
    return out


def amplitudes(qm):
    """A_u = L_u * a, a = sqrt(1.0 / norm), each rounded once (float64)"""
    a = np.sqrt(np.float64(1.0) / np.float64(NORM[qm]))
    return np.array(levels(qm // 2), dtype=np.float64) * a


def axis_indices(v, qm):
    """(uI, uQ) of the point index V = sum_j b_j << (QM-1-j): I takes b_0, b_2, ..., Q takes b_1, b_3, ..."""
    h = qm // 2
    b = [(v >> (qm - 1 - j)) & 1 for j in range(qm)]
    return (sum(b[2 * t] << (h - 1 - t) for t in range(h)), sum(b[2 * t + 1] << (h - 1 - t) for t in range(h)))


def points(qm):
    """the 2^QM points, complex128, indexed by V"""
    A = amplitudes(qm)
    return np.array([complex(A[ui], A[uq]) for ui, uq in (axis_indices(v, qm) for v in range(1 << qm))], dtype=np.complex128)


def gold(c_init, length):
    """c(0 .. length-1) of 38.211 5.2.1, uint8: the two registers stepped serially, 1600 + length times"""
    assert 0 <= c_init < (1 << 31)
    total = 1600 + length
    x1 = bytearray(total + 31)
    x2 = bytearray(total + 31)
    x1[0] = 1
    for i in range(31):
        x2[i] = (c_init >> i) & 1
    for n in range(total):
        x1[n + 31] = x1[n + 3] ^ x1[n]
        x2[n + 31] = x2[n + 3] ^ x2[n + 2] ^ x2[n + 1] ^ x2[n]
    a = np.frombuffer(bytes(x1), dtype=np.uint8)[1600:1600 + length]
    b = np.frombuffer(bytes(x2), dtype=np.uint8)[1600:1600 + length]
    return a ^ b


def modulate(bits, qm, c_init=-1, real=np.float64):
    """bits [..., n] uint8 (a byte equal to 1 is a one) -> symbols [..., n / QM]; bit i XOR c(i) first when c_init >= 0;
    real = np.float32: each coordinate rounded once"""
    ones = (np.asarray(bits) == 1).astype(np.int64)
    n, h = ones.shape[-1], qm // 2
    assert n % qm == 0
    if c_init >= 0:
        ones = ones ^ gold(c_init, n).astype(np.int64)
    g = ones.reshape(ones.shape[:-1] + (n // qm, qm))
    ui = sum(g[..., 2 * t] << (h - 1 - t) for t in range(h))
    uq = sum(g[..., 2 * t + 1] << (h - 1 - t) for t in range(h))
    A = amplitudes(qm)
    out = np.empty(ui.shape, dtype=np.complex128)
    out.real, out.imag = A[ui], A[uq]
    return out if real == np.float64 else out.astype(np.complex64)


def maxstar(a, b):
    """max(a, b) + log1p(exp(-|a - b|)), the maximum ignoring a NaN operand"""
    return np.fmax(a, b) + m_ln_1p(m_exp(-np.abs(a - b)))


def maxnum(a, b):
    """the max-log step: a NaN operand is ignored, and -0 < +0"""
    r = np.fmax(a, b)
    zeros = (a == 0) & (b == 0)
    return np.where(zeros, np.where(np.signbit(a) & np.signbit(b), r.dtype.type(-0.0), r.dtype.type(0.0)), r)


def axis_llrs(x, scale, qm, t, step):
    """the h LLRs of one axis: x [...] coordinates in the arithmetic type t -> list of h arrays"""
    h, A = qm // 2, amplitudes(qm)
    half = 0.5 * scale
    sx = x * t(scale)
    d = [sx * t(A[u]) - t(half * (A[u] * A[u])) for u in range(1 << h)]
    out = []
    for j in range(h):
        acc = [None, None]
        for u in range(1 << h):                      # ascending u, each fold starting from its first element
            b = (u >> (h - 1 - j)) & 1
            acc[b] = d[u] if acc[b] is None else step(acc[b], d[u])
        out.append(acc[0] - acc[1])
    return out


def demodulate(symbols, sigma, qm, max_log=False, c_init=-1):
    """symbols [..., S] complex64 / complex128 -> LLRs [..., QM * S] float32 / float64 in transmitted order, the LLR at row
    position i negated where c(i) = 1.  complex128: f64 arithmetic.  complex64: exact = widened, f64 arithmetic, rounded
    once; max_log = f32 throughout"""
    symbols = np.asarray(symbols)
    h = qm // 2
    out_t = np.float32 if symbols.dtype == np.complex64 else np.float64
    t = np.float32 if (out_t == np.float32 and max_log) else np.float64
    scale = 1.0 / (float(sigma) * float(sigma))
    step = maxnum if max_log else maxstar
    with np.errstate(all="ignore"):
        li = axis_llrs(symbols.real.astype(t), scale, qm, t, step)
        lq = axis_llrs(symbols.imag.astype(t), scale, qm, t, step)
        cols = []
        for j in range(h):
            cols += [li[j].astype(out_t), lq[j].astype(out_t)]
    out = np.stack(cols, axis=-1).reshape(symbols.shape[:-1] + (qm * symbols.shape[-1],))
    if c_init >= 0:
        out = np.where(gold(c_init, out.shape[-1]) == 1, -out, out)
    return out


def simulator_llrs(tx_rows, qm, sigma, seed, first_frame, max_log=False):
    """the simulator's DEFINED RESULT: tx_rows [frames][n_tx] (the pooled transmitted row of each frame) -> float32 LLRs:
    the f64 mapper without scrambling, the AWGN channel of (seed, first_frame + row, sigma), the f64 demapper"""
    sym = cr.awgn(modulate(tx_rows, qm), sigma, seed, first_frame)
    return demodulate(sym, sigma, qm, max_log=max_log).astype(np.float32)
