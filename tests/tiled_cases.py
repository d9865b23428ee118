"""Large batches for the entries that cut a call into passes or stages, built from a few rows -- TEST INFRASTRUCTURE ONLY.

The restatements are Python loops, so a call of millions of rows cannot be restated row by row.  Rows (or transport
blocks) of these entries are independent, so the restatement is computed once for `patterns` distinct random rows and row b
of the large call is pattern ids[b]:

    ids[b] = b % P                      P = 61, a prime
    ids[b] = P + i                      for the i-th row of `special`: boundary - 1 and boundary of every boundary at which
                                        the entry cuts the call, and the last row -- patterns that occur nowhere else

The expected output row b is the restatement's row ids[b]; for block-major arrays ([C * batch][K], row r * batch + b) the
same holds per block r.  No boundary is a multiple of P: a pass or stage that reads row b0 + f from offset f, or writes it
there, then meets another pattern and cannot match.  Tiling and comparison run on the device in chunks (torch
index_select), floats compared as integers, so nothing of gigabyte size crosses PCIe and numpy never holds it; the host
entries' arrays are a quarter of a gigabyte and use np.take."""
import functools

import numpy as np
import torch

import nr_transport_block_reference as tr

P = 61
BYTES = np.array([0, 1, 1, 2, 255], dtype=np.uint8)     # input bytes: a byte equal to 1 is a one, anything else a zero
CHUNK_ELEMENTS = 1 << 27


class Tiling:
    """the patterns of a call of `batch` rows that an entry cuts at `boundaries` (first rows of its later passes)"""

    def __init__(self, batch, boundaries):
        cuts = sorted({int(x) for x in boundaries})
        assert cuts, "a tiled case is about a call that is cut"
        for x in cuts:
            assert 0 < x < batch, f"the call of {batch} rows is not cut at {x}"
            assert x % P != 0, f"the boundary {x} is a multiple of {P}: a pass reading from offset 0 would match"
        self.batch = int(batch)
        self.boundaries = cuts
        self.special = sorted({x - 1 for x in cuts} | set(cuts) | {self.batch - 1})
        self.patterns = P + len(self.special)

    def pattern_of(self, b):
        """the pattern of row b (a special row's own)"""
        assert 0 <= b < self.batch
        return P + self.special.index(b) if b in self.special else b % P

    def ids(self):
        """numpy int64 [batch]"""
        ids = np.arange(self.batch, dtype=np.int64) % P
        ids[self.special] = P + np.arange(len(self.special))
        return ids

    def device_ids(self, device):
        """torch int64 [batch] on the device"""
        ids = torch.arange(self.batch, dtype=torch.int64, device=device) % P
        ids[torch.tensor(self.special, dtype=torch.int64, device=device)] = P + torch.arange(len(self.special), dtype=torch.int64,
                                                                                             device=device)
        return ids


def as_ints(x):
    """a torch tensor's bit patterns: floats as integers of their width (-0.0 and +0.0 differ, as do two NaNs)"""
    if x.dtype == torch.float32:
        return x.view(torch.int32)
    if x.dtype == torch.float64:
        return x.view(torch.int64)
    return x


def _chunks(batch, row):
    rows = max(CHUNK_ELEMENTS // max(int(row), 1), 1)
    return [(at, min(at + rows, batch)) for at in range(0, batch, rows)]


def tile_into(out, patterns, ids):
    """out [batch][row] (a view into a larger buffer is fine) = patterns[ids], on the device, chunk by chunk"""
    assert out.shape[0] == ids.numel() and out.shape[1:] == patterns.shape[1:] and out.dtype == patterns.dtype
    for lo, hi in _chunks(out.shape[0], patterns[0].numel()):
        out[lo:hi] = patterns.index_select(0, ids[lo:hi])
    return out


def tile(patterns, ids):
    """a new device tensor [batch][row] = patterns[ids]"""
    return tile_into(torch.empty((ids.numel(),) + tuple(patterns.shape[1:]), dtype=patterns.dtype, device=patterns.device), patterns, ids)


def first_mismatch(got, patterns, ids):
    """None when got [batch][row] equals patterns[ids] bit for bit, else (row b, its pattern, the first differing column)"""
    assert got.shape[0] == ids.numel() and got.shape[1:] == patterns.shape[1:] and got.dtype == patterns.dtype
    g, p = as_ints(got), as_ints(patterns)
    for lo, hi in _chunks(got.shape[0], patterns[0].numel()):
        want = p.index_select(0, ids[lo:hi])
        if torch.equal(g[lo:hi], want):
            continue
        bad = (g[lo:hi] != want).reshape(hi - lo, -1)
        b = int(bad.any(dim=1).nonzero()[0])
        return lo + b, int(ids[lo + b]), int(bad[b].nonzero()[0])
    return None


def assert_tiled(got, patterns, ids, what=""):
    bad = first_mismatch(got, patterns, ids)
    assert bad is None, f"{what}: row {bad[0]} (pattern {bad[1]}) differs from the restatement at column {bad[2]}"


def to_device(a, device):
    """a numpy array as a device tensor of the same type and shape"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(device)     # (torch takes no read-only array)


@functools.lru_cache(maxsize=None)
def two_block_patterns(patterns):
    """(2, 3826): C = 2, K = 2080, the smallest two-block configuration.  Returns (config, raw payload bytes
    [patterns][A], their restated rows [2 * patterns][K], block-major), computed once for the pass and the stage tests; the
    arrays are read-only."""
    ref = tr.Config(2, 3826)
    assert (ref.c, ref.k) == (2, 2080)
    raw = np.random.default_rng(3826).choice(BYTES, (patterns, ref.a))
    rows = ref.segment(raw)
    raw.setflags(write=False)
    rows.setflags(write=False)
    return ref, raw, rows


def flip(rows, row, pos):
    """the bit of byte (row, pos) inverted: a one becomes 0, anything else 1"""
    rows[row, pos] = 0 if rows[row, pos] == 1 else 1


def packed_views(flat, lengths, batch):
    """the blocks of a packed block-major array (numpy or torch, flat): block r is [batch][lengths[r]], block 0 first"""
    out, at = [], 0
    for e in lengths:
        out.append(flat[at:at + batch * e].reshape(batch, e))
        at += batch * e
    assert at == flat.shape[0]
    return out
