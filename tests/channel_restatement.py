"""Numpy restatement of the batched modulator and the AWGN channel -- TEST INFRASTRUCTURE ONLY.

Written from the definitions in include/ldpc_toolbox.h (PART 4: ldpc_toolbox_mod_run_*, ldpc_toolbox_awgn_run_*) and from
the reference's src/simulation/modulation.rs (trait Modulator :40-62, BpskModulator :87-95), src/simulation/interleaving.rs
:40-58 and src/simulation/channel.rs:60-81.  Philox4x32-10 is written from Salmon et al., "Parallel random numbers: as easy
as 1, 2, 3" (SC'11).  It shares nothing with ldpc_toolbox_amd/csrc: arrays vectorised over all symbols of all frames here,
one thread per symbol there.

logf is the platform libm's (independent_restatement.m_ln on float32); numpy's float32 *, +, / and sqrt round once each.
"""
import numpy as np

from independent_restatement import m_ln

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (values below 2^32, any integer type) -> [..., 4] uint32; uint64 arithmetic"""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _M32, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _M32]
        k = [(k[0] + w0) & _M32, (k[1] + w1) & _M32]
    return np.stack(c, axis=-1).astype(np.uint32)


def unit(w):
    """the upper 24 bits of a word as a float32 in [-1, 1): (w >> 8) * 2^-23 - 1, exact"""
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)


def normal_pairs(seed, frames, pairs):
    """two float32 standard normals for every (frame, pair): frames and pairs are integer arrays of one shape.  Polar
    method: block `attempt` = Philox(counter (attempt, pair, frame low, frame high), key (seed low, seed high)) offers the
    candidates (w0, w1) and (w2, w3); the first with 0 < s = v1^2 + v2^2 < 1 gives f = sqrt(-2 ln(s) / s), (v1 f, v2 f)"""
    frames = np.asarray(frames, dtype=np.uint64)
    pairs = np.asarray(pairs, dtype=np.uint64)
    shape = frames.shape
    frames, pairs = frames.reshape(-1), pairs.reshape(-1)
    z0 = np.zeros(frames.size, dtype=np.float32)
    z1 = np.zeros(frames.size, dtype=np.float32)
    key = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    todo = np.arange(frames.size)
    attempt = 0
    while todo.size:
        ctr = np.stack([np.full(todo.size, attempt, dtype=np.uint64), pairs[todo], frames[todo] & _M32, frames[todo] >> _S32],
                       axis=-1)
        w = philox4x32_10(ctr, key)
        open_ = np.ones(todo.size, dtype=bool)
        for h in (0, 1):
            v1, v2 = unit(w[:, 2 * h]), unit(w[:, 2 * h + 1])
            s = v1 * v1 + v2 * v2
            take = open_ & (s > np.float32(0.0)) & (s < np.float32(1.0))
            if take.any():
                st = s[take]
                f = np.sqrt(np.float32(-2.0) * m_ln(st) / st)
                z0[todo[take]] = v1[take] * f
                z1[todo[take]] = v2[take] * f
            open_ &= ~take
        todo = todo[open_]
        attempt += 1
    return z0.reshape(shape), z1.reshape(shape)


def interleave(bits, interleaving):
    """interleaving.rs:40-58 along the last axis: the codeword written row-wise into [columns][rows], read column-wise
    (the rows backwards for a negative value); 0 = none"""
    if interleaving == 0:
        return bits
    columns, n = abs(interleaving), bits.shape[-1]
    assert n % columns == 0
    a = bits.reshape(bits.shape[:-1] + (columns, n // columns))
    if interleaving < 0:
        a = a[..., ::-1, :]
    return np.ascontiguousarray(np.swapaxes(a, -1, -2)).reshape(bits.shape)


def modulate(bits, points, interleaving=0, real=np.float64):
    """bits [..., n] uint8 (a byte equal to 1 is a one) -> symbols [..., n / m].  points: 2^m complex128, or None for BPSK
    (reals: +1 for a one, -1 for a zero).  real = np.float32: each coordinate rounded once"""
    ones = interleave((np.asarray(bits) == 1).astype(np.int64), interleaving)
    if points is None:
        return np.where(ones == 1, real(1.0), real(-1.0)).astype(real)
    points = np.asarray(points, dtype=np.complex128)
    m = int(len(points)).bit_length() - 1
    assert len(points) == 1 << m and ones.shape[-1] % m == 0
    groups = ones.reshape(ones.shape[:-1] + (ones.shape[-1] // m, m))
    v = (groups << (m - 1 - np.arange(m))).sum(axis=-1)
    out = points[v]
    return out if real == np.float64 else out.astype(np.complex64)


def awgn(symbols, sigma, seed, first_frame=0):
    """symbols [B][S] -> a new array of the same type; row r is frame first_frame + r.  Complex: symbol s uses pair s.
    Real (BPSK): position j uses pair j / 2, its first normal for even j and its second for odd j.
    float64: x + sigma * float64(z).  float32: x + float32(sigma) * z"""
    symbols = np.asarray(symbols)
    B, S = symbols.shape
    frames = (int(first_frame) + np.arange(B, dtype=object)) % (1 << 64)
    frames = np.array([int(f) for f in frames], dtype=np.uint64)
    is_complex = np.iscomplexobj(symbols)
    real = symbols.real.dtype.type
    P = S if is_complex else (S + 1) // 2
    z0, z1 = normal_pairs(seed, np.repeat(frames[:, None], P, axis=1), np.repeat(np.arange(P)[None, :], B, axis=0))
    sg = real(sigma)
    if is_complex:
        re = symbols.real + sg * z0.astype(real)
        im = symbols.imag + sg * z1.astype(real)
        out = np.empty_like(symbols)
        out.real, out.imag = re, im
        return out
    z = np.stack([z0, z1], axis=-1).reshape(B, 2 * P)[:, :S]
    return symbols + sg * z.astype(real)
