"""A numpy statement of systematic LDPC encoding, independent of the library (this file does not import it), and the
synthetic codes the encoder tests run on.  Test helper only.

For a parity check matrix H = [H0 | H1] (k message columns, then m = n - k parity columns) with H1 invertible the
codeword of a message is the only vector that starts with the message and has H c = 0.  Two shapes of H1 make that a few
lines of numpy:
  * staircase (H1 bidiagonal): parity[r] = XOR over rows 0..r of (XOR of the message bits in the H0 columns of the row);
  * unit lower-triangular: forward substitution down the rows.
GF(2) throughout: every comparison made with these functions is exact equality.

A code is a list of rows, each a list of column indices (0-based) whose LAST entry is the row's diagonal k + r.
"""
import functools

import numpy as np

# (k, m) of the synthetic codes the tests use.  Staircase: the forms of the batched staircase encoder change at
# k rounded up to 8 = 40704 | 40712 and 81408 | 81416; (301, 1100) and (1000, 257) have k and m that are no multiple of
# 8 or 256.  Triangular (the dense-generator path): k on both sides of one and two 64-bit words, m on both sides of 64.
STAIRCASE_FORM_CODES = {(40704, 2300): 0, (40701, 2300): 0, (40712, 2300): 1, (81408, 2300): 1, (81409, 2300): 2,
                        (81416, 2300): 2}
STAIRCASE_ODD_CODES = ((301, 1100), (1000, 257))
TRIANGULAR_CODES = ((6, 6), (67, 65), (130, 200), (1000, 70))
LONG_ROW = 2000         # H0 columns of the planted long rows (all k of them in a code with k < 2000)


def alist_from_rows(n, rows):
    """alist text of the matrix with `n` columns and these rows, without padding (a 2000-column row would otherwise pad
    every row line to 2000 tokens)"""
    cols = [[] for _ in range(n)]
    for r, cs in enumerate(rows):
        for c in cs:
            cols[c].append(r)
    out = [f"{n} {len(rows)}", f"{max(map(len, cols))} {max(map(len, rows))}",
           " ".join(str(len(c)) for c in cols), " ".join(str(len(r)) for r in rows)]
    out += [" ".join(str(r + 1) for r in c) for c in cols]
    out += [" ".join(str(c + 1) for c in sorted(r)) for r in rows]
    return "\n".join(out) + "\n"


def _draw(rng, k, degree):
    degree = min(degree, k)
    return sorted(rng.choice(k, size=degree, replace=False).tolist()) if degree else []


def planted_degrees(m):
    """row -> H0 degree of the irregular rows of staircase_rows: none, one and LONG_ROW columns at the start of the
    matrix, at its end, and on each side of row 1024 (where a 1024-row chunk of the scan hands its carry to the next)"""
    at = {0: 0, 1: 1, 2: LONG_ROW, m - 3: LONG_ROW, m - 2: 1, m - 1: 0}
    if m > 1027 + 3:
        at.update({1021: 0, 1022: 1, 1023: LONG_ROW, 1024: LONG_ROW, 1025: 0, 1026: 1})
    return at


def staircase_rows(k, m, seed):
    """[H0 | bidiagonal]: H0 columns uniform over [0, k), row degrees 2..8, the rows of planted_degrees, and columns 0
    and k - 1 both in row 5"""
    assert k >= 8 and m >= 16
    rng = np.random.default_rng(seed)
    planted = planted_degrees(m)
    rows = []
    for r in range(m):
        h0 = _draw(rng, k, planted[r] if r in planted else int(rng.integers(2, 9)))
        if r == 5:
            h0 = sorted(set(h0) | {0, k - 1})
        rows.append(h0 + ([k + r - 1] if r else []) + [k + r])
    return rows


def triangular_rows(k, m, seed):
    """[H0 | L], L unit lower-triangular with up to 3 entries below the diagonal at any distance (so: no staircase);
    H0 rows of 0..6 columns, so some are empty"""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(m):
        h0 = _draw(rng, k, int(rng.integers(0, 7)))
        if r == 1:
            h0 = []
        if r == 2:
            h0 = sorted(set(h0) | {0, k - 1})
        below = sorted(set(rng.integers(0, r, size=min(r, 3)).tolist())) if r else []
        if r == m - 1:
            below = sorted(set(below) | {0})     # (never a bidiagonal, whatever was drawn)
        rows.append(h0 + [k + j for j in below] + [k + r])
    return rows


@functools.lru_cache(maxsize=None)
def synthetic(kind, k, m):
    """(rows, alist) of the synthetic code of this kind ("staircase" or "triangular") and size; the seed is k"""
    rows = (staircase_rows if kind == "staircase" else triangular_rows)(k, m, seed=k)
    return rows, alist_from_rows(k + m, rows)


def _ones(msgs):
    """the C ABI's convention: a byte equal to 1 is a one, anything else a zero"""
    return (np.asarray(msgs) == 1).astype(np.uint8)


def encode_staircase(k, rows, msgs):
    """msgs [B][k] -> codewords [B][k + m] of the staircase code `rows`"""
    for r, cs in enumerate(rows):
        assert [c for c in cs if c >= k] == ([k + r - 1] if r else []) + [k + r], r
    h0 = [[c for c in cs if c < k] for cs in rows]
    deg = np.array([len(cs) for cs in h0])
    idx = np.array([c for cs in h0 for c in cs], dtype=np.int64)
    start = np.cumsum(deg) - deg
    b = _ones(msgs)
    sums = np.zeros((b.shape[0], len(rows)), dtype=np.uint8)
    some = np.nonzero(deg)[0]        # (reduceat gives an empty segment its first element, not zero: those rows stay out)
    if len(some):
        sums[:, some] = np.bitwise_xor.reduceat(b[:, idx], start[some], axis=1)
    return np.concatenate([b, np.bitwise_xor.accumulate(sums, axis=1)], axis=1)


def encode_triangular(k, rows, msgs):
    """msgs [B][k] -> codewords [B][k + m] of a code whose parity part is unit lower-triangular"""
    b = _ones(msgs)
    cw = np.concatenate([b, np.zeros((b.shape[0], len(rows)), dtype=np.uint8)], axis=1)
    for r, cs in enumerate(rows):
        rest = [c for c in cs if c != k + r]
        assert len(rest) == len(cs) - 1 and all(c < k + r for c in rest), r
        if rest:
            cw[:, k + r] = np.bitwise_xor.reduce(cw[:, rest], axis=1)
    return cw


def syndrome(rows, codewords):
    """H c of every frame: [m][ceil(B / 8)] bytes, frame f in bit 7 - f % 8 of byte f // 8; all zero = every frame of
    the batch is a codeword.  The frames are bit-packed along the batch, so a row costs one XOR per 8 frames and edge."""
    cw = np.asarray(codewords)
    assert cw.ndim == 2 and ((cw == 0) | (cw == 1)).all()
    packed = np.packbits(cw.T, axis=1)                       # [n][ceil(B / 8)]
    deg = np.array([len(cs) for cs in rows])
    idx = np.array([c for cs in rows for c in cs], dtype=np.int64)
    start = np.cumsum(deg) - deg
    out = np.zeros((len(rows), packed.shape[1]), dtype=np.uint8)
    some = np.nonzero(deg)[0]
    if len(some):
        out[some] = np.bitwise_xor.reduceat(packed[idx], start[some], axis=0)
    return out


def puncture(codewords, pattern):
    """keeps the blocks of n / len(pattern) columns whose pattern entry is true"""
    cw = np.asarray(codewords)
    batch, n = cw.shape
    assert n % len(pattern) == 0
    keep = [j for j, p in enumerate(pattern) if p]
    return cw.reshape(batch, len(pattern), n // len(pattern))[:, keep, :].reshape(batch, -1)
