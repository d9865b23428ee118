"""Codes, frames and the host's own count for the row-shape tests ("cn_row_shape": test_cn_row_shape_host.py,
test_cn_row_shape_gpu.py).

The codes are cn_flags8_decode_cases.py's -- staircase codes whose longest rows have 3 to 7 edges, none of which has a run of
fitting rows, and its hand-built code of 7-edge rows, in which some runs of the check-node walk conform and others hold a
second degree-2 variable, a far peer, a degree-1 variable or the graph's first rows -- and one more:

  hand_built_np   the hand-built code with its staircase columns numbered backwards.  A row then lists the variable it shares
                  with the NEXT row before the one it shares with the previous row, as the built-in DVB-S2 tables do: the
                  kernel's other kind of straight-line step ("NP"; an alist's rows come out sorted by column, so only the
                  numbering can make one).  Frames: the hand-built code's, their columns moved the same way.
"""
import functools

import numpy as np

import cn_flags8_decode_cases as c8
from encoder_reference import alist_from_rows

CODES = c8.CODES + ("hand_built_np",)
ORACLE_ALWAYS, ORACLE_ONCE = c8.ORACLE_ALWAYS, c8.ORACLE_ONCE


@functools.lru_cache(maxsize=None)
def _np_columns():
    """new column of every column of hand_built()"""
    n, rows, _ = c8.hand_built()
    K = rows[0][6]  # (row 0: six information columns, then the first staircase column)
    perm = np.arange(n)
    perm[K:K + c8.HAND_ROWS] = K + c8.HAND_ROWS - 1 - np.arange(c8.HAND_ROWS)
    return perm


@functools.lru_cache(maxsize=None)
def code(name):
    """(n, rows as the decoder's tables list them, alist)"""
    if name != "hand_built_np":
        n, rows, a = c8.code(name)
        return n, [sorted(r) for r in rows], a
    n, rows, _ = c8.hand_built()
    perm = _np_columns()
    moved = [sorted(int(perm[c]) for c in r) for r in rows]
    return n, moved, alist_from_rows(n, moved)


@functools.lru_cache(maxsize=None)
def frames(name):
    """(llrs [257][n] f32, kind [257] of ORACLE_*), read-only"""
    if name != "hand_built_np":
        return c8.frames(name)
    llrs, kind = c8.frames("hand_built")
    out = np.empty_like(llrs)
    out[:, _np_columns()] = llrs
    out.setflags(write=False)
    return out, kind


def fitting_rows(n, rows):
    """-> (kind, fits per row).  A row fits kind "PN" when it has 7 edges: five variables of degree 3 or more, then a degree-2
    variable whose other edge is slot 6 of the row before, then one whose other edge is slot 5 of the row after; kind "NP": the
    same two the other way round, slot for slot.  (The rows are sorted and so are a column's rows: a variable's first edge is
    the one in its lower row.)  The kind is the one more rows fit, "none" where no row fits either."""
    deg = np.bincount([c for r in rows for c in r], minlength=n)
    at = {}
    for r, row in enumerate(rows):
        for slot, c in enumerate(row):
            at.setdefault(c, []).append((r, slot))
    fits = {"PN": [], "NP": []}
    for kind, (p_slot, n_slot) in (("PN", (5, 6)), ("NP", (6, 5))):
        for r, row in enumerate(rows):
            ok = len(row) == 7 and all(deg[c] >= 3 for c in row[:5]) and deg[row[5]] == 2 and deg[row[6]] == 2
            if ok:
                before = [x for x in at[row[p_slot]] if x[0] != r][0]
                after = [x for x in at[row[n_slot]] if x[0] != r][0]
                ok = before == (r - 1, n_slot) and after == (r + 1, p_slot)
            fits[kind].append(ok)
    if not any(fits["PN"]) and not any(fits["NP"]):
        return "none", fits["PN"]
    kind = "PN" if sum(fits["PN"]) >= sum(fits["NP"]) else "NP"
    return kind, fits[kind]


def conforming_runs(fits, run):
    """the runs of `run` rows (the last one shorter) whose rows all fit"""
    m = len(fits)
    return [r for r in range((m + run - 1) // run) if min(r * run + run, m) - r * run <= 0xFFFF and all(fits[r * run:r * run + run])]
