"""Codes and frames of test_record_flags8_gpu.py and test_record_flags8_host.py: vn_records_cases.py's synthetic staircase
codes with the longest row at 7 edges (48 rows of 4 to 7 edges, kept columns of weight 3, 8, 9 and 13: the byte form's code,
whose argmin 4..6 uses both stolen sign bits) and at 8 edges (the first length the byte form does not take), that module's
AWGN frames, and three frame sets that exercise the stored format:
  quantised_frames   LLRs in multiples of 0.5 (ties min1 == min2 in most rows), exact +0.0 and -0.0 among them (zero
                     magnitudes) and a few +-inf, at most one per row, so that nothing becomes NaN: compared with the oracle
  infinite_frames    +inf everywhere except a few finite LLRs: rows whose min2, or both minima, are +inf.  Compared
                     with the oracle in a ONE-iteration decode (a second iteration computes inf - inf)
  nan_frames         the two above with NaN LLRs sprinkled in: compared between the byte form and the 16-bit form only, bit
                     pattern for bit pattern
Everything is computed once and handed out read-only."""
import functools

import numpy as np

from vn_records_cases import M, frames, staircase_code  # noqa: F401  (re-exported)

WMAX = 7
QUANTISED, INFINITE, NANS = 64, 8, 24
SEED = 70807


def _read_only(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def quantised_frames():
    """[QUANTISED][n] f32"""
    K, rows, _ = staircase_code(WMAX)
    rng = np.random.default_rng(SEED)
    out = (np.round(frames(WMAX)[:QUANTISED].astype(np.float64) * 2.0) / 2.0).astype(np.float32)
    zero = rng.random(out.shape) < 0.04
    out[zero] = np.where(rng.random(int(zero.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    assert np.signbit(out[out == 0]).any() and not np.signbit(out[out == 0]).all()
    rows_of = [[r for r, cs in enumerate(rows) if c in cs] for c in range(K)]
    for f in range(0, QUANTISED, 2):                 # every second frame: three infinite LLRs on information columns of weight 3
        taken, placed = set(), 0
        for c in rng.permutation(K).tolist():
            if len(rows_of[c]) == 3 and not taken & set(rows_of[c]):
                taken |= set(rows_of[c])
                out[f, c] = np.float32(np.inf if placed else -np.inf)     # one wrong, two right (the all-zero codeword)
                placed += 1
                if placed == 3:
                    break
        assert placed == 3
    for cs in rows:
        assert (np.isinf(out[:, cs]).sum(axis=1) <= 1).all()
    return _read_only(out)


@functools.lru_cache(maxsize=None)
def infinite_frames():
    """[INFINITE][n] f32: the infinite LLRs all positive -- a message of infinite magnitude has the sign of the row's other
    inputs, all of them infinite, so no sum sees +inf and -inf -- and a fifth of the finite ones negative, so that no frame is
    a codeword before the first iteration"""
    n = staircase_code(WMAX)[0] + M
    rng = np.random.default_rng(SEED + 1)
    out = np.full((INFINITE, n), np.inf, dtype=np.float32)
    finite = rng.random(out.shape) < 0.25
    value = rng.integers(1, 12, int(finite.sum())) / 2.0
    out[finite] = np.where(rng.random(value.shape) < 0.2, -value, value).astype(np.float32)
    return _read_only(out)


@functools.lru_cache(maxsize=None)
def nan_frames():
    """[NANS][n] f32"""
    rng = np.random.default_rng(SEED + 2)
    out = np.concatenate([quantised_frames()[:NANS - INFINITE], infinite_frames()]).copy()
    nan = rng.random(out.shape) < 0.02
    nan[0] = False                                   # one frame without any
    out[nan] = np.float32(np.nan)
    assert np.isnan(out).any(axis=1).sum() >= NANS - 4
    return _read_only(out)
