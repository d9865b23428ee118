"""Codes and frames of test_vn_records_gpu.py: synthetic staircase codes [H0 | bidiagonal] of about a hundred columns whose
information columns have prescribed weights -- one of 13, one of 9 (both force a second round of the record kernel's
in-flight loop, at four and at eight records in flight), fifteen of 8 and the rest of 3 -- and whose rows have prescribed
lengths: 4 to 7 edges, and in every cycle of eight rows two of exactly `wmax` edges (12: the longest row the 16-bit flags
take; 13: the first they do not).  Frames are the all-zero codeword plus seeded AWGN.  Everything is computed once and
handed out read-only."""
import functools

import numpy as np

from encoder_reference import alist_from_rows

M = 48
FRAMES = 300
SIGMA, SEED = 0.7, 20264
ROW_CYCLE = (0, 7, 5, 6, 7, 4, 0, 5)      # row lengths, staircase entries included; 0 stands for wmax


@functools.lru_cache(maxsize=None)
def staircase_code(wmax):
    """(K, rows, alist).  Every row is filled exactly: the column weights add up to the rows' information slots, and a
    column's entries go to the rows with the most slots left (ties broken by a seeded shuffle), heaviest column first."""
    lengths = [ROW_CYCLE[r % len(ROW_CYCLE)] or wmax for r in range(M)]
    slots = [w - (2 if r else 1) for r, w in enumerate(lengths)]
    rest = sum(slots) - 13 - 9
    eights = next(a for a in range(15, 40) if (rest - 8 * a) % 3 == 0)
    weights = [13, 9] + [8] * eights + [3] * ((rest - 8 * eights) // 3)
    # interleave the weights so that a wave's consecutive variables differ: 13, 9, then 8 and 3 alternating
    tail = weights[2:]
    mixed = [w for pair in zip(tail[:eights], tail[eights:2 * eights]) for w in pair] + tail[2 * eights:]
    weights = weights[:2] + mixed
    K = len(weights)
    rng = np.random.default_rng(wmax)
    h0 = [[] for _ in range(M)]
    left = list(slots)
    for c in sorted(range(K), key=lambda c: -weights[c]):
        order = rng.permutation(M).tolist()
        order.sort(key=lambda r: -left[r])
        take = order[:weights[c]]
        assert all(left[r] > 0 for r in take), "the rows cannot take this column"
        for r in take:
            h0[r].append(c)
            left[r] -= 1
    assert not any(left)
    rows = [sorted(h0[r]) + ([K + r - 1] if r else []) + [K + r] for r in range(M)]
    assert [len(r) for r in rows] == lengths and max(lengths) == wmax
    col_w = np.bincount([c for r in rows for c in r], minlength=K + M)
    assert sorted(set(col_w[:K].tolist())) == [3, 8, 9, 13] and set(col_w[K:].tolist()) == {1, 2}
    return K, rows, alist_from_rows(K + M, rows)


@functools.lru_cache(maxsize=None)
def frames(wmax):
    """[FRAMES][n] f32 channel LLRs of the all-zero codeword over BPSK + AWGN: 2 y / sigma^2"""
    K = staircase_code(wmax)[0]
    rng = np.random.default_rng(SEED + wmax)
    y = 1.0 + SIGMA * rng.standard_normal((FRAMES, K + M))
    out = (2.0 * y / SIGMA ** 2).astype(np.float32)
    out.setflags(write=False)
    return out
