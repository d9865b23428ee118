"""Numpy restatement of the batched soft demapper -- TEST INFRASTRUCTURE ONLY.

Written from the definition in include/ldpc_toolbox.h (PART 4) and from the reference's src/simulation/modulation.rs
(BpskDemodulator :123-141, Psk8Demodulator :222-264, maxstar :286-288) and src/simulation/interleaving.rs:65-86.  It
shares nothing with ldpc_toolbox_amd/csrc: arrays vectorised over symbols here, one thread per symbol there.

exp / ln_1p are the platform libm's, called through tests/libm_map.c (numpy's own are SIMD re-implementations that
differ in the last ulp).  numpy's elementwise *, +, - round once each: no fused multiply-add.
"""
import numpy as np

from independent_restatement import m_exp, m_ln_1p

A = 0.70710678118654757     # (0.5f64).sqrt()

QPSK = np.array([complex((1 - 2 * b0) * A, (1 - 2 * b1) * A) for b0 in (0, 1) for b1 in (0, 1)])
# modulation.rs:168-179, at index V = b0 b1 b2
PSK8 = np.array([complex(A, A), complex(1.0, 0.0), complex(-1.0, 0.0), complex(-A, -A),
                 complex(0.0, 1.0), complex(A, -A), complex(-A, A), complex(0.0, -1.0)])
NAMED = {"QPSK": QPSK, "8PSK": PSK8}

# one row of special symbols: 0, -0.0, the smallest subnormal, 1e300, inf, -inf and NaN in either coordinate, and in both
_SPECIAL_VALUES = [0.0, -0.0, 5e-324, 1e300, np.inf, -np.inf, np.nan]
SPECIALS = np.array([complex(v, w) for v in _SPECIAL_VALUES for w in (0.3, -0.0)]
                    + [complex(w, v) for v in _SPECIAL_VALUES for w in (0.3, -0.0)]
                    + [complex(v, v) for v in _SPECIAL_VALUES])


def same_bits(got, want):
    """the tests' equality: NaN exactly where the reference value is NaN, otherwise identical bit patterns"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(u)[~nan], want.view(u)[~nan]))


def maxstar(a, b):
    """modulation.rs:286-288: a.max(b) + (-((a - b).abs())).exp().ln_1p()   (f64::max ignores a NaN operand)"""
    return np.fmax(a, b) + m_ln_1p(m_exp(-np.abs(a - b)))


def maxnum(a, b):
    """the max-log step: IEEE 754-2019 maximumNumber -- a NaN operand is ignored, and -0 < +0 (754-2008 maxNum, and
    with it np.fmax, leaves the sign of max(+0, -0) open; the demodulator is defined to give +0)"""
    r = np.fmax(a, b)
    zeros = (a == 0) & (b == 0)
    return np.where(zeros, np.where(np.signbit(a) & np.signbit(b), r.dtype.type(-0.0), r.dtype.type(0.0)), r)


def deinterleave(x, interleaving):
    """interleaving.rs:65-86 along the last axis; interleaving = signed columns (0: none, negative: rows read backwards)"""
    if interleaving == 0:
        return x
    columns, n = abs(interleaving), x.shape[-1]
    assert n % columns == 0
    t = np.swapaxes(x.reshape(x.shape[:-1] + (n // columns, columns)), -1, -2)   # a2.t()
    if interleaving < 0:
        t = t[..., ::-1, :]                                                        # invert_axis(Axis(0))
    return np.ascontiguousarray(t).reshape(x.shape)


def bpsk(symbols, sigma, interleaving=0):
    """symbols [..., n] float32 / float64 -> LLRs of the same type: scale * x, scale = -2 / sigma^2 computed in double"""
    scale = -2.0 / (float(sigma) * float(sigma))
    symbols = np.asarray(symbols)
    with np.errstate(all="ignore"):
        return deinterleave(symbols.dtype.type(scale) * symbols, interleaving)


def demodulate(symbols, sigma, points, energy_term=False, max_log=False, interleaving=0):
    """symbols [..., S] complex64 / complex128, points: 2^m complex128 -> LLRs [..., m * S] float32 / float64.
    complex128: f64 arithmetic.  complex64: exact = widened, f64 arithmetic, rounded once; max_log = f32 throughout."""
    symbols = np.asarray(symbols)
    points = np.asarray(points, dtype=np.complex128)
    m = int(len(points)).bit_length() - 1
    assert len(points) == 1 << m and 1 <= m <= 5
    out_t = np.float32 if symbols.dtype == np.complex64 else np.float64
    t = np.float32 if (out_t == np.float32 and max_log) else np.float64
    scale = 1.0 / (float(sigma) * float(sigma))
    half = 0.5 * scale
    step = maxnum if max_log else maxstar
    with np.errstate(all="ignore"):
        sr = symbols.real.astype(t) * t(scale)
        si = symbols.imag.astype(t) * t(scale)
        d = []
        for p in points:
            dv = sr * t(p.real) + si * t(p.imag)
            if energy_term:
                dv = dv - t(half * (p.real * p.real + p.imag * p.imag))
            d.append(dv)
        llrs = []
        for j in range(m):
            acc = [None, None]
            for v in range(1 << m):                   # ascending V, each fold starting from its first element
                b = (v >> (m - 1 - j)) & 1
                acc[b] = d[v] if acc[b] is None else step(acc[b], d[v])
            llrs.append((acc[0] - acc[1]).astype(out_t))
    out = np.stack(llrs, axis=-1).reshape(symbols.shape[:-1] + (m * symbols.shape[-1],))
    return deinterleave(out, interleaving)
