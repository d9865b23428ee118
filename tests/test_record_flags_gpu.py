"""Flooding min-sum row records with 16-bit flags (rows of at most 12 edges: csrc/graph_tables.h, record_flag_bits) against
the oracle and the per-edge message kernels: bits, iteration counts and posterior LLRs with np.array_equal -- no tolerance.

The codes and frames are record_flags_cases.py's: staircase codes whose longest rows have exactly 12 and exactly 13 edges.
The references are computed once per (code, rule) on the CPU and shared; every GPU decode of the parametrised tests is a
sub-millisecond job on a 360-column code."""
import functools
import itertools

import numpy as np
import pytest

import corrected_minsum_restatement as cm
import ldpc_toolbox_amd as lt
from frames import alist, awgn_frames
from record_flags_cases import BUSY_FRAMES, CALM_FRAMES, FRAMES, compaction_frames, frames, staircase_code

pytestmark = pytest.mark.gpu

ITERATIONS = 30
BATCHES = (1, 3, 65, 333)           # partial tiles and partial packs (none of them can free half a group: the 2-byte
                                    # compaction mover is test_flags_travel_with_a_compaction's)
RULES = ("Minsumf32", "Minsumf64", "NormMinsumf32")


def cpu_decode(oracle, wmax, rule, llrs):
    """(bits, iterations, posterior): the oracle for plain min-sum; the numpy restatement the corrected min-sum tests use
    for the normalized rule, which the oracle does not have"""
    a = staircase_code(wmax)[1]
    if rule.startswith("Norm"):
        bits, its, post = cm.decode(a, rule, llrs, ITERATIONS)
    else:
        bits, its, post = oracle.decode_batch(oracle.Graph(a), rule, llrs, ITERATIONS, threads=8)
    post = post if rule.endswith("f64") else post.astype(np.float32)
    return bits, its, post


@functools.lru_cache(maxsize=None)
def reference(oracle, wmax, rule):
    """of all FRAMES frames"""
    return cpu_decode(oracle, wmax, rule, frames())


@functools.lru_cache(maxsize=None)
def compaction_reference(oracle, wmax, rule):
    return cpu_decode(oracle, wmax, rule, compaction_frames())


def gpu_input(rule, llrs):
    return llrs.astype(np.float64) if rule.endswith("f64") else llrs


def assert_same(got, want, count, what):
    assert np.array_equal(got[1], want[1][:count]), ("iterations", what)
    assert np.array_equal(got[0], want[0][:count]), ("bits", what)
    assert got[2].dtype == want[2].dtype
    assert np.array_equal(got[2], want[2][:count]), ("posterior", what)


@pytest.mark.parametrize("wmax", [12, 13])
@pytest.mark.parametrize("rule", RULES)
def test_narrow_flags_are_invisible(oracle, wmax, rule):
    """every record path -- pack widths 4 / 2 / 1, run lengths of the row walk 1 / 3 / 8 / 64, the first convergences'
    L-free posteriors rebuilt inside the variable-node launch or by a launch of their own, deferred L-free stores on and off,
    batch compaction on and off -- returns what the reference and the per-edge kernels return, at batches that leave tiles
    and packs partly empty.  "record_flag_bits": 16 with 12-edge rows; with 13 the decoder's own word, 32 bits in f32 and
    64 in f64; "row_records" stays 3, the family."""
    flag_bits = 16 if wmax == 12 else (64 if rule.endswith("f64") else 32)
    want = reference(oracle, wmax, rule)
    dec = lt.LdpcDecoder(staircase_code(wmax)[1], rule)
    dec.set("latency", 0)              # the batched kernels at every batch size
    assert dec.get("row_records") == 3 and dec.get("record_flag_bits") == flag_bits
    llrs = gpu_input(rule, frames())
    dec.set("group_size", FRAMES)
    dec.set("records", 0)
    assert dec.get("row_records") == 0 and dec.get("record_flag_bits") == 0
    edge = dec.decode_batch(llrs, ITERATIONS, want_posterior=True)
    spread = edge[1][edge[1] >= 0]
    print(f"{rule} weight {wmax}: per-edge path converges at iterations {sorted(set(spread.tolist()))}, "
          f"{int((edge[1] < 0).sum())} failures")
    assert len(spread) and spread.max() - spread.min() >= 5        # convergences spread over the iterations
    assert_same(edge, want, FRAMES, "per-edge")
    dec.set("records", 1)
    for batch in BATCHES:
        dec.set("group_size", batch)
        for vec, run, vn_event, quiet, compact in itertools.product((4, 2, 1), (1, 3, 8, 64), (0, 1), (0, 1), (0, 1)):
            for k, v in (("vec", vec), ("rec_run", run), ("vn_event", vn_event), ("rec_quiet", quiet), ("compact", compact)):
                dec.set(k, v)
            got = dec.decode_batch(llrs[:batch], ITERATIONS, want_posterior=True)
            assert_same(got, want, batch, (batch, vec, run, vn_event, quiet, compact))
    assert dec.get("row_records") == 3 and dec.get("record_flag_bits") == flag_bits


@pytest.mark.parametrize("wmax", [12, 13])
@pytest.mark.parametrize("rule", RULES)
def test_flags_travel_with_a_compaction(oracle, wmax, rule):
    """A batch whose compaction plan fires, so that compact_move_kernel<uint16_t> carries the live codewords' flags to their
    new slots beside the magnitudes: 640 frames in one group, the 448 calm ones in the leading slots, the 192 busy ones
    behind them.  compact_plan_kernel packs when the live codewords, rounded up to 256 slots, free at least half of the
    group's slots, and the saving (freed slots x min(remaining, 8) iterations) exceeds 9/4 codeword-iterations per live
    codeword.  At the first checkpoint (iteration 6) the calm frames are done and at most 192 frames live: 256 of 640 slots
    (768 if the group is rounded up to the next tile) stay, at least 384 are freed, and every live codeword sits beyond
    slot 256 and moves.  The reference alone shows those premises; the frames that converge after the move, and the ones
    that never do, then come out bit for bit as without compaction and as on the CPU."""
    want = compaction_reference(oracle, wmax, rule)
    its = want[1]
    calm, busy = its[:CALM_FRAMES], its[CALM_FRAMES:]
    late = int(((busy < 0) | (busy >= 9)).sum())
    print(f"{rule} weight {wmax}: calm frames converge at {sorted(set(calm.tolist()))}, busy at {sorted(set(busy.tolist()))}, "
          f"{late} busy frames live beyond iteration 8, {int((busy >= 9).sum())} of them converge")
    # (these premises hold for record_flags_cases.py's seeds and noise levels: whoever changes those re-establishes them)
    assert calm.min() >= 0 and calm.max() <= 3          # done well before the first checkpoint
    assert late >= 8 and (busy >= 9).sum() >= 3         # moved codewords: some converge later, from the moved records
    total = CALM_FRAMES + BUSY_FRAMES
    llrs = gpu_input(rule, compaction_frames())
    dec = lt.LdpcDecoder(staircase_code(wmax)[1], rule)
    dec.set("latency", 0)
    dec.set("group_size", total)
    assert dec.get("record_flag_bits") == (16 if wmax == 12 else (64 if rule.endswith("f64") else 32))
    for vec, run, vn_event, quiet, compact in itertools.product((4, 2, 1), (1, 8), (0, 1), (0, 1), (1, 0)):
        for k, v in (("vec", vec), ("rec_run", run), ("vn_event", vn_event), ("rec_quiet", quiet), ("compact", compact)):
            dec.set(k, v)
        got = dec.decode_batch(llrs, ITERATIONS, want_posterior=True)
        assert_same(got, want, total, (vec, run, vn_event, quiet, compact))


@pytest.mark.parametrize("rule", ["Minsumf32", "Minsumf64"])
def test_far_peers_with_narrow_flags(oracle, rule):
    """AR4JA's degree-2 variables join distant rows: with "records" = 2 the check-node kernel fetches the peer's record --
    magnitudes and 16-bit flags -- instead of finding it in the neighbouring row of its walk"""
    spec, punct = "ar4ja:1/2:1024", "1,1,1,1,0"
    _, llrs, full = awgn_frames(spec, 256, 2.2, 4242, punct)
    gpu_in = llrs.astype(np.float64) if rule.endswith("f64") else llrs
    dec = lt.LdpcDecoder(alist(spec), rule, punct)
    dec.set("group_size", 256)
    dec.set("records", 0)
    ref = dec.decode_batch(gpu_in, 30, want_posterior=True)
    spread = ref[1][ref[1] >= 0]
    assert len(spread) and spread.max() - spread.min() >= 5
    dec.set("records", 2)
    for opts in ({}, {"rec_run": 1, "vec": 2}, {"rec_run": 64, "vec": 1, "compact": 0}):
        for k, v in opts.items():
            dec.set(k, v)
        got = dec.decode_batch(gpu_in, 30, want_posterior=True)
        assert dec.get("row_records") == 3 and dec.get("record_flag_bits") == 16
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), (opts,)
    sub = slice(0, 256, 4)
    ob_, oi_, op_ = oracle.decode_batch(oracle.Graph(alist(spec)), rule, full[sub], 30, threads=8)
    assert np.array_equal(ref[1][sub], oi_) and np.array_equal(ref[0][sub], ob_)
    assert np.array_equal(ref[2][sub].astype(np.float64), op_)
