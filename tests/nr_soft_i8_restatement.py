"""A numpy restatement of the 8-bit soft-bit receive path (include/ldpc_toolbox.h, PART 9) that shares nothing with the
library: the quantiser Q, the symmetric clip, and rate recovery / HARQ combining on int8 soft bits written on top of
`nr_rate_match_reference.Config` -- its `selection` and the literal interleaver loop -- left to right with a clip after
every sum.  All arithmetic is in int64: nothing wraps, and the clip is the only place a value is cut."""
import numpy as np

SOFT_MAX = 127


def clip(v):
    """min(max(v, -127), 127) on integers: an int8 of -128 reads as -127"""
    return np.clip(np.asarray(v).astype(np.int64), -SOFT_MAX, SOFT_MAX)


def quantise(x):
    """Q(x): round-half-away(8 x) clamped to +-127, NaN -> 0, as int8.  8 x is exact in float64 for float32 and float64 x."""
    y = 8.0 * np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        r = np.sign(y) * np.floor(np.abs(y) + 0.5)          # half away from zero (np.round would go to even)
        r = np.where(np.isnan(y), 0.0, np.clip(r, -SOFT_MAX, SOFT_MAX))
    return r.astype(np.int8)


def dequantise(v):
    """the float32 row the 8-bit decode entry is defined on: clip(v) / 8"""
    return (clip(v).astype(np.float32) / np.float32(8.0)).astype(np.float32)


def recover_i8(cfg, rx, rv: int, qm: int, filler: int = SOFT_MAX, old=None, saturated=None):
    """rx [B][E] int8 -> [B][n] int8; old: the int8 soft buffer to combine into (a new array is returned).
    saturated: an optional bool [B][n] array, set where some partial sum of the column (the combining included) left +-127."""
    rx = np.asarray(rx)
    assert rx.dtype == np.int8 and 1 <= filler <= SOFT_MAX
    B, e = rx.shape
    sel = cfg.selection(e, rv)
    pos = np.zeros(e, dtype=np.int64)                     # where selection index k lies after the interleaver
    for i in range(qm):
        for q in range(e // qm):
            pos[i * (e // qm) + q] = i + q * qm
    t = clip(rx)
    kept = np.zeros((B, cfg.n), dtype=np.int64) if old is None else clip(old)
    out = kept.copy()
    carried_by = [[] for _ in range(cfg.n)]               # per column, ascending selection index
    for k in range(e):
        carried_by[sel[k]].append(k)
    for c in range(cfg.n):
        if cfg.k - cfg.fillers <= c < cfg.k:
            out[:, c] = filler
            continue
        carriers = carried_by[c]
        if not carriers:
            continue                                      # R = 0: 0, or clip(old)
        s = t[:, pos[carriers[0]]].copy()
        for k in carriers[1:]:
            raw = s + t[:, pos[k]]
            s = clip(raw)
            if saturated is not None:
                saturated[:, c] |= raw != s
        if old is not None:
            raw = kept[:, c] + s
            s = clip(raw)
            if saturated is not None:
                saturated[:, c] |= raw != s
        out[:, c] = s
    return out.astype(np.int8)
