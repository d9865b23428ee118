"""The record kernel's carried channel row (csrc/kernels_flooding.hip.h, cn_minsum_rec_kernel: carry_chan / carry_var) against
the CPU references: bits, iteration counts and posterior LLRs with np.array_equal -- no tolerance.

A row of the walk hands the channel row of a degree-2 variable it shares with the NEXT row of the walk to that row, which
then issues no load for it.  What can go wrong is which variable takes the carried pack (two variables between the same pair
of rows, a variable whose peer is two rows away, a degree-1 variable beside a shared one, a shared variable beyond slot 8 of a
long row) and where a carry begins and ends (run boundaries, both walk directions, a short last run).  The codes below are the
smallest that have each of these: 26-37 rows.  Every code is [H0 | staircase] plus the planted variables of its case;
"shuffled" codes number their columns at random, so the shared variables sit at every slot of their rows.

References: the oracle for plain min-sum, the numpy restatement of the corrected rules for the normalized and offset ones,
once per (code, rule) on the CPU."""
import functools
import itertools

import numpy as np
import pytest

import corrected_minsum_restatement as cm
import ldpc_toolbox_amd as lt
from encoder_reference import alist_from_rows
from frames import alist, awgn_frames

pytestmark = pytest.mark.gpu

ITERATIONS = 10
FRAMES = 300
BATCHES = (1, 255, 256, 257, 300)   # tile and slice edges; frozen lanes inside a pack come with the convergences
SIGMA, SEED = 0.72, 4711
RULES = ("Minsumf32", "Minsumf64", "NormMinsumf32", "NormMinsumf64", "OffsetMinsumf32", "OffsetMinsumf64")

# name -> (rows, H0 degrees (cycled), pairs (c, c+1) with a second shared variable, pairs (c, c+2) with a far variable,
#          rows with an extra degree-1 variable, shuffled column numbers)
# 29 rows: 4 runs of 8 (the last one short and walked downwards), 10 runs of 3; 37 rows: 5 runs of 8 (the last one short and
# walked upwards), 13 runs of 3.  Rows 7 | 8 and 15 | 16 are run boundaries of the default run (8), 8 | 9 one of run 3.
CODES = {
    "plain29": (29, (2, 1, 3, 5, 4), (), (), (), False),
    "plain37": (37, (3, 1, 2, 5, 4, 2), (), (), (), False),
    "parallel": (30, (2, 1, 3, 4), (3, 7, 8, 12, 15, 22, 28), (), (), True),
    "far": (30, (2, 1, 3, 4), (), (2, 6, 7, 13, 14, 22, 27), (), True),
    "single": (29, (2, 1, 3, 4), (), (), (0, 5, 8, 15, 28), True),
    "mixed": (37, (2, 1, 3, 4, 2), (4, 7, 20, 31), (5, 7, 16, 30), (3, 8, 24, 36), True),
    "long12": (26, (2, 8, 9, 3, 9, 8, 1, 8, 9), (2, 9, 10), (4, 12), (5, 13), True),         # rows of up to 12 edges
    "long14": (26, (2, 9, 11, 3, 10, 9, 1, 11, 10), (2, 9, 10), (4, 12), (5, 13), True),     # beyond 12: the wide flags
}


@functools.lru_cache(maxsize=None)
def code(name):
    """(rows, alist text, n)"""
    m, degrees, parallel, far, single, shuffled = CODES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    want = [degrees[r % len(degrees)] for r in range(m)]
    k = max(3, sum(want) // 4)          # every information column gets degree 3 or more: the variable-node kernel's
    deck, rows = [], []
    for r in range(m):
        h0 = []
        while len(h0) < want[r]:
            if not deck:
                deck = rng.permutation(k).tolist()
            c = deck.pop()
            if c in h0:
                deck.insert(0, c)
                continue
            h0.append(c)
        rows.append(h0 + ([k + r - 1] if r else []) + [k + r])      # p_{r-1}, p_r: p_{m-1} has degree 1
    n = k + m
    for c in parallel:
        rows[c].append(n)
        rows[c + 1].append(n)
        n += 1
    for c in far:
        rows[c].append(n)
        rows[c + 2].append(n)
        n += 1
    for c in single:
        rows[c].append(n)
        n += 1
    if shuffled:
        perm = rng.permutation(n)
        rows = [[int(perm[c]) for c in row] for row in rows]
    rows = [sorted(row) for row in rows]
    deg = np.bincount(np.concatenate(rows), minlength=n)
    assert deg.min() >= 1 and (deg >= 3).sum() == k and (deg <= 2).sum() == n - k
    return rows, alist_from_rows(n, rows), n


def shared_slots(rows):
    """[(slot in row c, slot in row c + 1)] of every variable that joins two consecutive rows"""
    out = []
    for c in range(len(rows) - 1):
        for v in set(rows[c]) & set(rows[c + 1]):
            out.append((rows[c].index(v), rows[c + 1].index(v)))
    return out


@functools.lru_cache(maxsize=None)
def frames(name):
    """[FRAMES][n] f32 channel LLRs of the all-zero codeword over BPSK + AWGN"""
    n = code(name)[2]
    y = 1.0 + SIGMA * np.random.default_rng(SEED).standard_normal((FRAMES, n))
    out = (2.0 * y / SIGMA ** 2).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(oracle, name, rule):
    """(bits, iterations, posterior) of all FRAMES frames, with the premise every case relies on: some frames converge in
    the first iterations, some later, some never -- so lanes freeze inside packs, the L-free posteriors are written from
    the first convergence on, and both kinds of frame return a posterior"""
    a = code(name)[1]
    if rule.startswith(("Norm", "Offset")):
        bits, its, post = cm.decode(a, rule, frames(name), ITERATIONS)
    else:
        bits, its, post = oracle.decode_batch(oracle.Graph(a), rule, frames(name), ITERATIONS, threads=8)
    post = post if rule.endswith("f64") else post.astype(np.float32)
    ok = its[its > 0]
    print(f"{name} {rule}: converged at {np.bincount(ok, minlength=ITERATIONS + 1)[1:].tolist()}, {int((its == 0).sum())} clean, "
          f"{int((its < 0).sum())} failures")
    assert (ok <= 2).sum() >= 5 and (ok >= 4).sum() >= 5 and (its < 0).sum() >= 5
    return bits, its, post


def decoder(name, rule):
    dec = lt.LdpcDecoder(code(name)[1], rule)
    dec.set("latency", 0)       # the batched kernels at every batch size
    dec.set("records", 2)       # row records wherever they are possible
    assert dec.get("row_records") == 3
    longest = max(map(len, code(name)[0]))
    assert dec.get("record_flag_bits") == (16 if longest <= 12 else (64 if rule.endswith("f64") else 32))
    return dec


def gpu_input(rule, llrs):
    return llrs.astype(np.float64) if rule.endswith("f64") else llrs


def assert_same(got, want, count, what):
    assert np.array_equal(got[1], want[1][:count]), ("iterations", what)
    assert np.array_equal(got[0], want[0][:count]), ("bits", what)
    assert got[2].dtype == want[2].dtype
    assert np.array_equal(got[2], want[2][:count]), ("posterior", what)


def test_the_codes_have_what_their_cases_need():
    """host-side premises: run counts, planted variables, and the shared variable on either side of slot 8"""
    assert all(len(code(n)[0]) % 8 and len(code(n)[0]) % 3 for n in ("plain29", "plain37"))     # a short last run
    assert -(-29 // 8) % 2 == 0 and -(-37 // 8) % 2 == 1 and -(-37 // 3) % 2 == 1              # last run down / up / up
    for name in ("plain29", "plain37"):
        assert all(3 <= len(r) <= 7 for r in code(name)[0][1:])
    for name in ("long12", "long14"):
        rows = code(name)[0]
        assert max(map(len, rows)) == (12 if name == "long12" else 14), sorted(map(len, rows))
        s = shared_slots(rows)
        assert any(a >= 8 > b for a, b in s) and any(b >= 8 > a for a, b in s) and any(a >= 8 and b >= 8 for a, b in s)
    for name in ("parallel", "mixed", "long12"):
        rows = code(name)[0]
        assert sum(len(set(rows[c]) & set(rows[c + 1])) == 2 for c in range(len(rows) - 1)) >= 3
    # shuffled columns: in some row the far variable, or the second shared one, has the slot that the carried variable
    # had in the row before
    rows = code("far")[0]
    deg = np.bincount(np.concatenate(rows))
    hits = 0
    for c in range(len(rows) - 2):
        for v in set(rows[c]) & set(rows[c + 2]):
            if deg[v] == 2:
                hits += 1
    assert hits == 7


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", sorted(CODES))
def test_every_walk_carries_the_right_row(oracle, name, rule):
    """pack widths 4 / 2 / 1, run lengths 1 (no carry ever), 3, 8 and 64 (one run, upwards), with one run per wavefront (the
    default at this size) and with as few wavefronts as the tiling allows ("waves" = 1: a wavefront walks several runs, up
    and down, one after the other: a carry must not survive a run), and the long-row variant of the kernel forced on.
    A stale carry can only match where a wavefront walks ADJACENT runs of one row each: "rec_run" 1 with one wavefront per
    slice, which the tiling gives for "waves" 1 at "vec" 1 in f32 (four 64-codeword slices per 256-codeword tile fill a
    workgroup).  A build that keeps the carried variable across runs fails exactly there, (vec, run, waves, long) =
    (1, 1, 1, 0), in the f32 rules (profiles/chan_carry.txt, section 6)."""
    want = reference(oracle, name, rule)
    dec = decoder(name, rule)
    dec.set("group_size", FRAMES)
    llrs = gpu_input(rule, frames(name))
    for vec, run, waves, long_rows in itertools.product((4, 2, 1), (1, 3, 8, 64), (0, 1), (0, 1)):
        for k, v in (("vec", vec), ("rec_run", run), ("waves", waves), ("rec_long", long_rows)):
            dec.set(k, v)
        got = dec.decode_batch(llrs, ITERATIONS, want_posterior=True)
        assert_same(got, want, FRAMES, (vec, run, waves, long_rows))


@pytest.mark.parametrize("rule", ["Minsumf32", "NormMinsumf64", "OffsetMinsumf32"])
@pytest.mark.parametrize("name", ["plain29", "mixed", "long12", "long14"])
def test_partial_tiles_and_the_posterior_stores(oracle, name, rule):
    """batches at the tile and slice edges, batch compaction on and off, the L-free posteriors stored every iteration or
    from a slice's first convergence on, rebuilt inside the variable-node launch or by a launch of their own"""
    want = reference(oracle, name, rule)
    dec = decoder(name, rule)
    llrs = gpu_input(rule, frames(name))
    for batch in BATCHES:
        dec.set("group_size", batch)
        for vec, run, compact, quiet, vn_event in itertools.product((4, 1), (3, 8), (0, 1), (0, 1), (0, 1)):
            for k, v in (("vec", vec), ("rec_run", run), ("compact", compact), ("rec_quiet", quiet), ("vn_event", vn_event)):
                dec.set(k, v)
            got = dec.decode_batch(llrs[:batch], ITERATIONS, want_posterior=True)
            assert_same(got, want, batch, (batch, vec, run, compact, quiet, vn_event))


def test_dvbs2_short_frame(oracle):
    """one real code: DVB-S2 short frame, nominal rate 1/2 -- 9000 rows of 4 to 7 edges, 1125 runs of 8"""
    spec = "dvbs2:R1_2short"
    _, llrs, _ = awgn_frames(spec, 64, 3.1, 99)       # 8 iterations: convergences at 6, 7 and 8, 14 failures
    want = oracle.decode_batch(oracle.Graph(alist(spec)), "Minsumf32", llrs, 8, threads=8)
    its = want[1]
    print(f"{spec}: converged at {np.bincount(its[its >= 0], minlength=9).tolist()}, {int((its < 0).sum())} failures")
    assert (its >= 0).sum() >= 5 and (its < 0).sum() >= 5
    want = (want[0], want[1], want[2].astype(np.float32))
    dec = lt.LdpcDecoder(alist(spec), "Minsumf32")
    dec.set("latency", 0)
    dec.set("group_size", 64)
    assert dec.get("row_records") == 3 and dec.get("record_flag_bits") == 16
    for opts in ({}, {"rec_run": 3, "vec": 1}, {"rec_run": 64, "vec": 2, "rec_quiet": 0}):
        for k, v in opts.items():
            dec.set(k, v)
        assert_same(dec.decode_batch(llrs, 8, want_posterior=True), want, 64, opts)
