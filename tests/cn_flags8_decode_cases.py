"""Codes and frames of test_cn_flags8_decode_gpu.py: the smallest codes on which the byte form of the flooding min-sum
check-node kernel (rows of at most 7 edges, seven loads in flight, the record's argmins decoded once per load) can go wrong.

  staircase(w), w = 3..7   [H0 | bidiagonal] whose longest rows have exactly w edges.  w = 7 is record_flags8_cases.py's code
                           (rows of 4 to 7 edges: every slot of the seven is filled); below 7, where that module's generator
                           always deals 7-edge rows, 48 rows of 3 to w edges dealt here the same way: information columns of
                           weight 3 or 4, each put on the rows with the most room left.
  hand_built()             40 rows of exactly 7 edges -- five runs of the kernel's 8-row walk, upwards and downwards, with inner
                           rows and boundaries in both directions -- with a degree-1 variable (the last staircase column), two
                           degree-2 variables that join the SAME pair of rows (inside a run: rows 3, 4; across a run
                           boundary: rows 15, 16), and degree-2 variables whose rows are not neighbours (rows 2 and 21: another
                           run; rows 10 and 13: the same run, two rows apart): their peer record is fetched on its own.

Frames, 257 per code: the all-zero codeword plus AWGN at two noise levels, interleaved -- an odd frame converges within a
few iterations, an even one (frame 0 too: a batch of one) mostly never --, and at every third place from 2 on a frame that
exercises the stored format until those run out:
  ties          the code's own noisy frames in multiples of 0.5 with exact +0.0 and -0.0 (min1 == min2, zero magnitudes)
  NaN           one noisy frame with NaN LLRs sprinkled in: compared between the forms only, bit pattern for bit pattern
  w = 7 only    record_flags8_cases.py's quantised frames (ties, zeros, a few +-inf) and infinite frames (min2 or both minima
                +inf; the CPU reference holds for ONE iteration, a second computes inf - inf)
ORACLE_ALWAYS / ORACLE_ONCE / ORACLE_NEVER say per frame when the CPU reference is a reference.  Everything is computed once
and handed out read-only."""
import functools

import numpy as np

import record_flags8_cases as r8
from encoder_reference import alist_from_rows

M = 48
FRAMES = 257
SEED = 81807
SIGMA_CALM, SIGMA_BUSY = 0.5, 1.4
ORACLE_ALWAYS, ORACLE_ONCE, ORACLE_NEVER = 0, 1, 2
CODES = ("staircase3", "staircase4", "staircase5", "staircase6", "staircase7", "hand_built")


def _deal(slots, seed):
    """information columns of weight 3 (a few of 4, so that every slot is taken) over rows with `slots` free places: a
    column's entries go to the rows with the most room left, ties broken by a seeded shuffle -> (K, entries per row)"""
    total = sum(slots)
    K = total // 3
    weights = [3 + (1 if c < total - 3 * K else 0) for c in range(K)]
    rng = np.random.default_rng(seed)
    left, h0 = list(slots), [[] for _ in slots]
    for c in sorted(range(K), key=lambda c: -weights[c]):
        order = rng.permutation(len(slots)).tolist()
        order.sort(key=lambda r: -left[r])
        take = order[:weights[c]]
        assert all(left[r] > 0 for r in take), "the rows cannot take this column"
        for r in take:
            h0[r].append(c)
            left[r] -= 1
    assert not any(left)
    return K, h0


@functools.lru_cache(maxsize=None)
def staircase(w):
    """(n, rows, alist)"""
    assert 3 <= w <= 7
    if w == 7:
        K, rows, a = r8.staircase_code(7)
        return K + r8.M, rows, a
    cycle = (w, max(3, w - 2), w, max(3, w - 1), 3, w)
    lengths = [cycle[r % len(cycle)] for r in range(M)]
    K, h0 = _deal([n - (2 if r else 1) for r, n in enumerate(lengths)], 100 + w)
    rows = [sorted(h0[r]) + ([K + r - 1] if r else []) + [K + r] for r in range(M)]
    assert [len(r) for r in rows] == lengths and max(lengths) == w and min(lengths) == 3
    return K + M, rows, alist_from_rows(K + M, rows)


HAND_ROWS = 40
SAME_PAIRS = ((3, 4), (15, 16))      # a second degree-2 variable beside the staircase's, inside a run and across a boundary
FAR_PAIRS = ((2, 21), (10, 13))      # degree-2 variables whose rows are not neighbours


@functools.lru_cache(maxsize=None)
def hand_built():
    """(n, rows, alist): columns are the information columns, then the 40 staircase columns, then the four extra degree-2
    columns"""
    extra = [[] for _ in range(HAND_ROWS)]
    for j, (a, b) in enumerate(SAME_PAIRS + FAR_PAIRS):
        extra[a].append(j)
        extra[b].append(j)
    slots = [7 - (2 if r else 1) - len(extra[r]) for r in range(HAND_ROWS)]
    K, h0 = _deal(slots, 77)
    first_extra = K + HAND_ROWS
    rows = [sorted(h0[r]) + ([K + r - 1] if r else []) + [K + r] + [first_extra + j for j in extra[r]] for r in range(HAND_ROWS)]
    n = first_extra + len(SAME_PAIRS + FAR_PAIRS)
    assert all(len(r) == 7 and r == sorted(r) for r in rows)
    col_w = np.bincount([c for r in rows for c in r], minlength=n)
    assert col_w[K + HAND_ROWS - 1] == 1 and (col_w[K:K + HAND_ROWS - 1] == 2).all() and (col_w[first_extra:] == 2).all()
    assert (col_w[:K] >= 3).all()
    return n, rows, alist_from_rows(n, rows)


def code(name):
    return hand_built() if name == "hand_built" else staircase(int(name[-1]))


def _awgn(rng, count, n, sigma):
    y = 1.0 + sigma * rng.standard_normal((count, n))
    return (2.0 * y / sigma ** 2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def frames(name):
    """(llrs [FRAMES][n] f32, kind [FRAMES] of ORACLE_*)"""
    n = code(name)[0]
    rng = np.random.default_rng([SEED, CODES.index(name)])
    out = np.where((np.arange(FRAMES) % 2 == 1)[:, None], _awgn(rng, FRAMES, n, SIGMA_CALM), _awgn(rng, FRAMES, n, SIGMA_BUSY))
    kind = np.full(FRAMES, ORACLE_ALWAYS)
    special = []
    for sigma in (SIGMA_CALM, SIGMA_BUSY, SIGMA_BUSY):
        tie = (np.round(_awgn(rng, 1, n, sigma)[0].astype(np.float64) * 2.0) / 2.0).astype(np.float32)
        zero = rng.random(n) < 0.06
        tie[zero] = np.where(rng.random(int(zero.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
        special.append((tie, ORACLE_ALWAYS))
    nan = _awgn(rng, 1, n, SIGMA_BUSY)[0]
    nan[rng.random(n) < 0.03] = np.float32(np.nan)
    assert np.isnan(nan).any()
    special.insert(1, (nan, ORACLE_NEVER))
    if name == "staircase7":
        special += [(f, ORACLE_ALWAYS) for f in r8.quantised_frames()[:6]]
        special += [(f, ORACLE_ONCE) for f in r8.infinite_frames()[:3]]
    for j, (f, k) in enumerate(special):
        out[2 + 3 * j], kind[2 + 3 * j] = f, k
    assert 2 + 3 * len(special) <= 65          # the batch of 65 has them all
    out = out.astype(np.float32)
    out.setflags(write=False)
    kind.setflags(write=False)
    return out, kind
