"""Codes and frames of the row-weight tests (test_row_weight_host.py, test_row_weight_gpu.py): synthetic codes whose longest
check rows have EXACTLY `w` edges, for every w at which the decoder changes its check-node kernel, its record form, a mask
width or a workgroup size ("row-weight selectors").  Two families, so that a full row is met with and without
degree-1/2 variables beside it:

  staircase_code(w)  [H0 | bidiagonal], record_flags_cases.staircase_code for any w in 8..65: information columns of degree
                     3 or more, the staircase's degree-1/2 variables (row records, L-free tables), short rows of 5-8 edges
                     between the full ones, one row per layered level;
  regular_code(w)    every column of degree 3 or 4 -- no L-free variable, so no row records and the plain check-node /
                     variable-node pair -- in four layers of variable-disjoint rows: the layered schedule gets four levels,
                     the first of them twelve full rows;
  regular_6_32()     every row 32 edges, every column 6: 512 x 96, six levels of sixteen rows.

Frames are the all-zero codeword plus seeded AWGN as f32 LLRs, one sigma per (family, w); frame 0 is noise-free (the
pre-check takes it: 0 iterations), frame 1 is noise alone (it never converges).  Everything is computed once and handed out
read-only."""
import functools

import numpy as np

from encoder_reference import alist_from_rows

WEIGHTS = (8, 9, 10, 11, 12, 13, 20, 21, 24, 25, 26, 27, 32, 33, 58, 59, 64, 65)
FAMILIES = ("staircase", "regular")
M = 120                  # rows of a staircase code
FRAMES = 130             # two full 64-frame waves and a partial one
SEED = 20262
# noise levels, chosen on the CPU by a scan over sigma: at these every implementation that decodes the code
# (DECODES below) shows, in its reference, what premises() states -- test_row_weight_gpu.py asserts it from the references'
# output.  The higher a code's rate, the less noise its min-sum decoders take.  Whoever changes a seed or a code
# re-establishes them.
SIGMA = {
    "staircase": {8: 0.68, 9: 0.66, 10: 0.62, 11: 0.66, 12: 0.66, 13: 0.64, 20: 0.62, 21: 0.64, 24: 0.62, 25: 0.64, 26: 0.60,
                  27: 0.62, 32: 0.58, 33: 0.60, 58: 0.48, 59: 0.50, 64: 0.48, 65: 0.46},
    "regular": {8: 0.76, 9: 0.80, 10: 0.74, 11: 0.72, 12: 0.68, 13: 0.66, 20: 0.58, 21: 0.56, 24: 0.56, 25: 0.52, 26: 0.52,
                27: 0.52, 32: 0.50, 33: 0.48, 58: 0.44, 59: 0.42, 64: 0.42, 65: 0.42},
    "regular_6_32": 0.50,
}
# regular_6_32's compaction batch (as record_flags_cases.compaction_frames): calm frames, which converge at once, in the
# leading slots, busy ones behind them
CALM_FRAMES, BUSY_FRAMES = 448, 192
CALM_SIGMA = 0.25


def staircase_columns(w):
    """information columns of staircase_code(w): 240 as in record_flags_cases from 10 edges on, fewer below (the deal must
    reach every column three times), 8 per edge of the longest row beyond 30 edges (the column degrees stay at 4-5)"""
    info_edges = (M // 8) * sum(_info_degrees(w))
    return min(240, info_edges // 3 // 8 * 8) if w < 12 else max(240, 8 * w)


def _info_degrees(w):
    return [4, min(6, w - 2), min(8, w - 2), w - 2, 5, min(7, w - 2), 3, w - 2]


@functools.lru_cache(maxsize=None)
def staircase_code(w):
    """(rows, alist): [H0 | bidiagonal] whose longest rows have exactly `w` edges (30 of the 120 rows, at least; the others
    5 to 10).  record_flags_cases.staircase_code with the short rows capped at w and the column count following w: with w = 12
    and 13 it deals the same codes, edge for edge (test_row_weight_host.py)."""
    assert 8 <= w <= 65
    K = staircase_columns(w)
    rng = np.random.default_rng(w)
    info_degrees = _info_degrees(w)
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
    assert max(map(len, rows)) == w and sum(len(r) == w for r in rows) >= 10
    return rows, alist_from_rows(K + M, rows)


def _partition(columns, sizes):
    """rows over `columns` in order, their lengths cycling through `sizes`; a last row of one edge takes an edge of the row
    before it (a degree-1 check is undefined for most rules)"""
    rows, at, i = [], 0, 0
    while at < len(columns):
        take = min(sizes[i % len(sizes)], len(columns) - at)
        rows.append(columns[at:at + take])
        at += take
        i += 1
    if len(rows[-1]) == 1:
        rows[-1].insert(0, rows[-2].pop())
    return [sorted(int(c) for c in r) for r in rows]


@functools.lru_cache(maxsize=None)
def regular_code(w):
    """(rows, alist): n = 12 w columns, every one of degree 3 or 4, in four layers of rows that share no column -- so the
    layered schedule has four levels.  Layer 1: twelve rows of exactly w edges; layers 2 and 3: each column once more, in
    rows of w - 1 edges down to 4; layer 4: a third of the columns a fourth time, in rows of at most w - 2 edges."""
    assert 8 <= w <= 65
    n = 12 * w
    rng = np.random.default_rng(1000 + w)
    rows = _partition(rng.permutation(n).tolist(), [w])
    rows += _partition(rng.permutation(n).tolist(), [w - 1, (w + 1) // 2, 5, w - 1, 4])
    rows += _partition(rng.permutation(n).tolist(), [w - 2, 6, w - 1, (w + 3) // 2])
    rows += _partition(rng.permutation(n)[:n // 3].tolist(), [w - 2, min(7, w - 2), w // 2])
    assert max(map(len, rows)) == w and sum(len(r) == w for r in rows) == 12 and min(map(len, rows)) >= 2
    return rows, alist_from_rows(n, rows)


@functools.lru_cache(maxsize=None)
def regular_6_32():
    """(rows, alist): the shape of the 10GBASE-T code -- every row 32 edges, every column 6 -- at n = 512, m = 96: six
    layers, each a random partition of the columns into sixteen rows"""
    n = 512
    rng = np.random.default_rng(632)
    rows = []
    for _ in range(6):
        rows += _partition(rng.permutation(n).tolist(), [32])
    return rows, alist_from_rows(n, rows)


def code(family, w=None):
    if family == "regular_6_32":
        return regular_6_32()
    return staircase_code(w) if family == "staircase" else regular_code(w)


def columns(family, w=None):
    return int(code(family, w)[1].split(None, 1)[0])


def _awgn(rng, count, n, sigma):
    """[count][n] f32 channel LLRs of the all-zero codeword over BPSK + AWGN: 2 y / sigma^2"""
    y = 1.0 + sigma * rng.standard_normal((count, n))
    return (2.0 * y / sigma ** 2).astype(np.float32)


def _frames(family, w, count):
    n = columns(family, w)
    sigma = SIGMA[family] if w is None else SIGMA[family][w]
    rng = np.random.default_rng([SEED, FAMILIES.index(family) if w is not None else 2, w or 0])
    out = _awgn(rng, count, n, sigma)
    out[0] = np.float32(2.0 / sigma ** 2)                                # noise-free
    out[1] = (2.0 * sigma * rng.standard_normal(n) / sigma ** 2).astype(np.float32)    # noise alone: no codeword under it
    return out


@functools.lru_cache(maxsize=None)
def frames(family, w=None):
    """[FRAMES][n] f32 (200 frames for regular_6_32)"""
    out = _frames(family, w, FRAMES if w is not None else 200)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def compaction_frames():
    """[CALM_FRAMES + BUSY_FRAMES][512] for regular_6_32: see CALM_FRAMES above"""
    calm = _awgn(np.random.default_rng(SEED + 1), CALM_FRAMES, 512, CALM_SIGMA)
    out = np.concatenate([calm, frames("regular_6_32")[:BUSY_FRAMES]])
    out.setflags(write=False)
    return out


def last_slot_argmins(family, w):
    """(frame, full row) pairs whose smallest channel magnitude sits in the row's LAST slot (its largest column): in the first
    iteration a row's inputs are the channel LLRs themselves, so there the min-sum kernels see argmin = w - 1"""
    rows, _ = code(family, w)
    llrs = frames(family, w)
    width = max(map(len, rows))
    return sum(int((np.abs(llrs[:, cs]).argmin(axis=1) == width - 1).sum()) for cs in rows if len(cs) == width)


def last_slot_negatives(family, w):
    """(frame, full row) pairs with a negative channel LLR in the row's last slot: the top bit of the sign mask"""
    rows, _ = code(family, w)
    llrs = frames(family, w)
    width = max(map(len, rows))
    return sum(int((llrs[:, cs[-1]] < 0).sum()) for cs in rows if len(cs) == width)


def premises(its):
    """what every reference decode of frames() must show, from its iteration counts alone: frame 0 passes the pre-check,
    converged frames at three or more distinct positive iteration counts, a failure"""
    converged = sorted(set(its[its > 0].tolist()))
    return its[0] == 0 and len(converged) >= 3 and bool((its < 0).any())


ITERATIONS = 12


def is_f64(impl):
    return impl.split(":")[0].endswith("f64")


def cpu_decode(oracle, family, w, impl, llrs, iterations=ITERATIONS):
    """(bits, iterations, posterior in the type the GPU returns): oracle_binding (`oracle`) for every rule the reference has;
    the numpy restatements of the corrected and the 8-bit min-sum tests for the Norm / Offset / Minsumi8 names"""
    a = code(family, w)[1]
    if "Minsumi8" in impl:
        import minsum_i8_restatement as mi
        bits, its, post = mi.decode(a, impl, llrs, iterations)
    elif "NormMinsum" in impl or "OffsetMinsum" in impl:
        import corrected_minsum_restatement as cm
        bits, its, post = cm.decode(a, impl, llrs, iterations)
    else:
        bits, its, post = oracle.decode_batch(oracle.Graph(a), impl, llrs, iterations, threads=8)
    return bits, its, (post if is_f64(impl) else post.astype(np.float32))


# ---- which implementation decodes which weight ---------------------------------------------------------------------------
# Every weight of WEIGHTS is one side of a pair at which a selector of the decoder changes with the longest row (in the
# layered schedule: the longest row of a level); an implementation decodes the weights at which ITS selector changes.
# (csrc = ldpc_toolbox_amd/csrc; the line is that of the selector)
#
#   8 | 9     Launch::rec_long of the flooding record kernels              run_group.hip.h:30          Minsum / NormMinsum f32, Minsum / OffsetMinsum f64
#             layered min-sum register bucket 8 -> 12                      launch.hip.h:238            HLMinsum / HLOffsetMinsum f32, HLMinsumf64
#   10 | 11   cn_reg_kernel bucket 10 -> 12 (flooding Tanh)                run_group.hip.h:122         Tanhf32
#             layered register rows 10 -> 12 of the other float rules      run_group.hip.h:312         HLTanhf32, HLPhif64
#   12 | 13   16-bit record flags -> the decoder's word                    graph_tables.h:84           flooding min-sum, both types
#             cn_reg_kernel 12 -> cn_staged_kernel, kLevelRecShort         run_group.hip.h:122, slice_tasks.h:48   Tanhf32
#             layered min-sum bucket 12 -> 20                              launch.hip.h:238            HLMinsum*
#             layered register rows 12 -> 24, floats and 8-bit             run_group.hip.h:312, run_group_i8.hip:126   HLTanhf32, HLPhif64, HLAminstari8, HLMinsumi8Norm
#   20 | 21   layered min-sum bucket 20 -> 32 (f32), -> none (f64)         launch.hip.h:238-239        HLMinsum*
#   24 | 25   layered register rows 24 -> the two-pass kernel              run_group.hip.h:312, run_group_i8.hip:126   HLTanhf32, HLPhif64, HLAminstari8, HLMinsumi8Norm
#   26 | 27   f32 records: argmin inside the flags word -> a fourth word   graph_tables.h:88,121       Minsum / NormMinsum f32
#             layered row records (three words) -> per-edge messages       run_group.hip.h:248         HLMinsum / HLOffsetMinsum f32
#   32 | 33   32-bit -> 64-bit sign mask of the streaming kernels          run_group.hip.h:123         flooding min-sum f32 and f64 (regular family, "records" 0, "lfree" 0)
#             f32 row records exist -> per-edge messages                   graph_tables.h:89           Minsum / NormMinsum f32
#             layered min-sum bucket 32 -> hl_minsum_kernel                launch.hip.h:238            HLMinsum / HLOffsetMinsum f32
#             staged_block (device_decoder_internal.h:202), 256 -> 128 threads: two f32 columns (Phif32, Minstarapproxi8),
#             one f64 column (Tanhf64); 128 -> 64 threads: two f64 columns (Aminstarf64)
#   58 | 59   f64 records: argmin inside the flags word -> a fourth word   graph_tables.h:88,121       Minsum / OffsetMinsum f64
#             (layered f64 row records would end here, run_group.hip.h:248, had f64 a register bucket beyond 20)   HLMinsumf64
#   64 | 65   f64 row records exist -> per-edge messages                   graph_tables.h:89           Minsum / OffsetMinsum f64
#             streaming -> LDS-staged flooding min-sum                     run_group.hip.h:95          flooding min-sum, both types
#             small-batch tables ready -> not                              graph_tables.h:137,218      Minsumf32, HLMinsumf32, Phif64, Minstarapproxi8
#             staged_block, 256 -> 128 threads: one f32 column (Tanhf32); 128 -> 64 threads: two f32 columns (Phif32,
#             Minstarapproxi8), one f64 column (Tanhf64); two f64 columns (Phif64): 64 threads on both sides, beyond 64 KiB of
#             LDS at 65
_UP_TO_33 = tuple(w for w in WEIGHTS if w <= 33)
_STAGED = (32, 33, 64, 65)
_LAYERED_ROWS = (10, 11, 12, 13, 24, 25)
DECODES = {
    "Minsumf32": _UP_TO_33 + (64, 65), "NormMinsumf32": _UP_TO_33 + (64, 65),
    "Minsumf64": WEIGHTS, "OffsetMinsumf64": WEIGHTS,
    "HLMinsumf32": _UP_TO_33 + (64, 65), "HLOffsetMinsumf32": _UP_TO_33,      # (HLMinsumf32 at 64, 65: the small-batch test)
    "HLMinsumf64": tuple(w for w in WEIGHTS if w <= 27) + (58, 59),
    "Tanhf32": (10, 11, 12, 13, 64, 65), "Phif32": _STAGED, "Aminstarf64": (32, 33), "Tanhf64": _STAGED,
    "Phif64": (64, 65),                                                        # (the small-batch test)
    "HLTanhf32": _LAYERED_ROWS, "HLPhif64": _LAYERED_ROWS, "HLAminstari8": _LAYERED_ROWS, "HLMinsumi8Norm": _LAYERED_ROWS,
    "Minstarapproxi8": _STAGED,
}
REGULAR_6_32 = ("Minsumf32", "Minsumf64", "HLMinsumf32", "HLMinsumf64", "Tanhf32", "HLTanhf32", "Minstarapproxi8", "HLMinsumi8")


def implementations(w):
    return tuple(impl for impl, ws in DECODES.items() if w in ws)
