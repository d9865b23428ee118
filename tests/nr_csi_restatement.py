"""Numpy restatement of the per-symbol-CSI NR demapper and the Rayleigh block-fading channel -- TEST INFRASTRUCTURE ONLY.

Written from the definitions in include/ldpc_toolbox.h (PART 10; the fading channel beside the AWGN channel of PART 4).  It
builds on nr_qam_reference (amplitudes, fold steps, the Gold sequence) and channel_restatement (the normal pairs) and
shares nothing with ldpc_toolbox_amd/csrc: arrays vectorised over all symbols of all frames here, one thread per symbol
there.  numpy's elementwise *, -, / and float32 sqrt round once each: no fused multiply-add.
"""
import numpy as np

import channel_restatement as cr
import nr_qam_reference as nq

GAIN_KEY = 0x9E3779B97F4A7C15      # the gains' Philox key is seed ^ GAIN_KEY: another stream than the noise's


def axis_llrs_csi(x, s, qm, t, step):
    """the h LLRs of one axis: coordinates x and per-symbol scales s, both arrays of the arithmetic type t.
    sx = x * s, K_u = (0.5 * s) * Q_u with Q_u = t(A_u * A_u), d_u = sx * A_u - K_u, then the folds of the scalar demapper"""
    h, A = qm // 2, nq.amplitudes(qm)
    sx = x * s
    half = t(0.5) * s                                  # exact
    d = [sx * t(A[u]) - half * t(A[u] * A[u]) for u in range(1 << h)]
    out = []
    for j in range(h):
        acc = [None, None]
        for u in range(1 << h):                        # ascending u, each fold starting from its first element
            b = (u >> (h - 1 - j)) & 1
            acc[b] = d[u] if acc[b] is None else step(acc[b], d[u])
        out.append(acc[0] - acc[1])
    return out


def demodulate_csi(symbols, scale, qm, max_log=False, c_init=-1):
    """symbols [..., S] complex64 / complex128 and scale [..., S] (1 / sigma_s^2 per symbol) -> LLRs [..., QM * S] float32 /
    float64 in transmitted order, the LLR at row position i negated where c(i) = 1.  complex128: f64 arithmetic.  complex64:
    exact = symbol and scale widened, f64 arithmetic, each LLR rounded once; max_log = f32 throughout"""
    symbols = np.asarray(symbols)
    h = qm // 2
    out_t = np.float32 if symbols.dtype == np.complex64 else np.float64
    t = np.float32 if (out_t == np.float32 and max_log) else np.float64
    s = np.asarray(scale, dtype=out_t).astype(t)
    assert s.shape == symbols.shape
    step = nq.maxnum if max_log else nq.maxstar
    with np.errstate(all="ignore"):
        li = axis_llrs_csi(symbols.real.astype(t), s, qm, t, step)
        lq = axis_llrs_csi(symbols.imag.astype(t), s, qm, t, step)
        cols = []
        for j in range(h):
            cols += [li[j].astype(out_t), lq[j].astype(out_t)]
    out = np.stack(cols, axis=-1).reshape(symbols.shape[:-1] + (qm * symbols.shape[-1],))
    if c_init >= 0:
        out = np.where(nq.gold(c_init, out.shape[-1]) == 1, -out, out)
    return out


def _frames(first_frame, rows):
    return np.array([(int(first_frame) + r) % (1 << 64) for r in range(rows)], dtype=np.uint64)


def gains(seed, frames, blocks):
    """af for every (frame, block index): float32 sqrt(0.5 * (w0^2 + w1^2)) of the normal pair keyed seed ^ GAIN_KEY"""
    w0, w1 = cr.normal_pairs(int(seed) ^ GAIN_KEY, frames, blocks)
    gf = np.float32(0.5) * (w0 * w0 + w1 * w1)
    return np.sqrt(gf)


def fading(symbols, sigma, block, seed, first_frame=0):
    """symbols [B][S] complex64 / complex128 -> (equalised symbols, scale [B][S] float32 / float64); row r is frame
    first_frame + r.  Symbol s: gain af of block s // block, sigma_e = sigma / float64(af), scale_s = 1 / sigma_e^2 (both
    float64), noise pair s of the AWGN channel.  float64: x + sigma_e * float64(z).  float32: x + float32(sigma_e) * z and
    float32(scale_s)"""
    symbols = np.asarray(symbols)
    B, S = symbols.shape
    assert int(block) >= 1
    real = symbols.real.dtype.type
    fr = np.repeat(_frames(first_frame, B)[:, None], S, axis=1)
    sym = np.repeat(np.arange(S, dtype=np.uint64)[None, :], B, axis=0)
    af = gains(seed, fr, sym // np.uint64(block))
    sigma_e = np.float64(sigma) / af.astype(np.float64)
    scale = np.float64(1.0) / (sigma_e * sigma_e)
    z0, z1 = cr.normal_pairs(seed, fr, sym)
    se = sigma_e.astype(real)
    out = np.empty_like(symbols)
    out.real = symbols.real + se * z0.astype(real)
    out.imag = symbols.imag + se * z1.astype(real)
    return out, scale.astype(real)


def simulator_llrs(tx_rows, qm, sigma, seed, first_frame, block, max_log=False):
    """the simulator's DEFINED RESULT with "fading_block" = block: tx_rows [frames][n_tx] (the pooled transmitted row of
    each frame, or a HARQ process's concatenated row) -> float32 LLRs: the f64 mapper without scrambling, the f64 fading
    channel of (seed, first_frame + row, sigma, block), the f64 CSI demapper"""
    sym, scale = fading(nq.modulate(tx_rows, qm), sigma, block, seed, first_frame)
    return demodulate_csi(sym, scale, qm, max_log=max_log).astype(np.float32)
