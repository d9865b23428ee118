"""Codes and frames of the record-flags tests (test_record_flags_host.py, test_record_flags_gpu.py): two synthetic staircase
codes, about 240 information columns and 120 rows, whose longest rows have exactly 12 and exactly 13 edges -- the two sides
of the boundary between the 16-bit flags array and the record's own third word.  Frames are the all-zero codeword plus
seeded AWGN.  Everything is computed once and handed out read-only."""
import functools

import numpy as np

from encoder_reference import alist_from_rows

K, M = 240, 120
FRAMES = 333
SIGMA, SEED = 0.6, 20261
# the compaction batch: CALM_FRAMES frames at CALM_SIGMA, which converge at once, in the leading slots, then the first
# BUSY_FRAMES of frames(), whose convergences are spread over the iterations, in the trailing ones
CALM_FRAMES, BUSY_FRAMES = 448, 192
CALM_SIGMA = 0.3


@functools.lru_cache(maxsize=None)
def staircase_code(wmax):
    """(rows, alist): [H0 | bidiagonal] whose longest rows have exactly `wmax` edges.  The information columns are dealt
    from shuffled passes over all K columns, so every one of them has degree 3 or 4 (the variable-node kernel walks them)
    and the degree-1/2 variables are the staircase's: their peers are the neighbouring rows."""
    rng = np.random.default_rng(wmax)
    info_degrees = [4, 6, 8, wmax - 2, 5, 7, 3, wmax - 2]
    deck = []
    rows = []
    for r in range(M):
        want = info_degrees[r % len(info_degrees)]
        h0 = []
        while len(h0) < want:
            if not deck:
                deck = rng.permutation(K).tolist()
            c = deck.pop()
            if c in h0:
                deck.insert(0, c)
                continue
            h0.append(c)
        rows.append(sorted(h0) + ([K + r - 1] if r else []) + [K + r])
    assert max(map(len, rows)) == wmax and sum(len(r) == wmax for r in rows) >= 10
    return rows, alist_from_rows(K + M, rows)


def _awgn(rng, count, sigma):
    """[count][n] f32 channel LLRs of the all-zero codeword over BPSK + AWGN: 2 y / sigma^2"""
    y = 1.0 + sigma * rng.standard_normal((count, K + M))
    return (2.0 * y / sigma ** 2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def frames():
    out = _awgn(np.random.default_rng(SEED), FRAMES, SIGMA)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def compaction_frames():
    """[CALM_FRAMES + BUSY_FRAMES][n]: see CALM_FRAMES above"""
    out = np.concatenate([_awgn(np.random.default_rng(SEED + 1), CALM_FRAMES, CALM_SIGMA), frames()[:BUSY_FRAMES]])
    out.setflags(write=False)
    return out
