"""Decode parity on codes whose longest check rows fill a register bucket, a sign mask or a packed record EXACTLY, and on the
weight one beyond: every row-weight selector of the decoder ("row-weight selectors"; the table beside
row_weight_cases.DECODES names each selector's source line and the implementations that decode its two weights) against the
CPU oracle -- or, for the Norm / Offset / Minsumi8 names, the numpy restatements -- with np.array_equal on iteration counts,
bits and posterior LLRs.  There is no tolerance anywhere.

The codes and frames are row_weight_cases.py's: a staircase family (degree-1/2 variables: row records, L-free tables, one
row per layered level) and a regular family (no L-free variable: the plain check-node / variable-node pair, four layered
levels of several rows), a few hundred columns each; a GPU decode is a sub-millisecond job, a reference at most half a
second, computed once per (family, w, implementation)."""
import functools

import numpy as np
import pytest

import ldpc_toolbox_amd as lt
import row_weight_cases as rc
from row_weight_cases import ITERATIONS, is_f64

pytestmark = pytest.mark.gpu

BATCHES = (5, 130)                  # a partial wave; two waves and a partial one (no tile, no pack of 2 or 4 is full)
SMALL = (1, 8, 19)                  # the single-launch paths' sizes: one codeword, one per XCD, bundles


def is_layered(impl):
    return impl.startswith("HL")


def is_float_minsum(impl):
    return "Minsumf" in impl


def oracle_i8(impl):
    """the reference's own 8-bit rules: a frame that passes the pre-check has no decoder state there, so its posterior is
    compared for the frames that ran (the `its != 0` rule of test_gpu_parity.py / test_gpu_stress.py)"""
    return "i8" in impl and "Minsumi8" not in impl


@functools.lru_cache(maxsize=None)
def reference(oracle, family, w, impl):
    """of all frames of (family, w), read-only"""
    want = rc.cpu_decode(oracle, family, w, impl, rc.frames(family, w))
    for a in want:
        a.setflags(write=False)
    return want


def assert_same(got, want, frames, impl, what):
    """frames: how many leading frames of `want` were decoded, or their slice"""
    sl = frames if isinstance(frames, slice) else slice(0, frames)
    assert np.array_equal(got[1], want[1][sl]), ("iterations", impl, what)
    assert np.array_equal(got[0], want[0][sl]), ("bits", impl, what)
    assert got[2].dtype == want[2].dtype, (impl, what)
    if oracle_i8(impl):
        run = got[1] != 0
        assert np.array_equal(got[2][run], want[2][sl][run]), ("posterior", impl, what)
    else:
        assert np.array_equal(got[2], want[2][sl]), ("posterior", impl, what)


def gpu_input(impl, llrs):
    return llrs.astype(np.float64) if is_f64(impl) else llrs            # the f64 rules through the f64 entry


def expected_records(family, w, f64):
    """("row_records", "record_flag_bits") of a flooding min-sum decoder.  Records need L-free variables
    (csrc/graph_tables.h:89, `!lf.ready`): none in the regular family.  In a staircase code: rows of at most 32 (f32) / 64
    (f64) edges (graph_tables.h:89); three words while the argmin fits the flags word beside the flip bits, 26 / 58 edges,
    four beyond (graph_tables.h:121); the flags as 16-bit words up to 12 edges, else the decoder's own word (graph_tables.h:84)."""
    word = 64 if f64 else 32
    if family != "staircase" or w > word:
        return 0, 0
    return (3 if w <= (58 if f64 else 26) else 4), (16 if w <= 12 else word)


# The execution choices that swap a bucketed kernel for the general one, by rule: each entry is applied over the defaults.
FLOODING_MINSUM = ({"records": 1, "lfree": 1, "staged_minsum": 0, "rec_long": 0, "vec": 4},
                   ({"records": 0}, {"records": 0, "vec": 2}, {"records": 0, "lfree": 0}, {"records": 0, "lfree": 0, "vec": 2},
                    {"records": 0, "lfree": 0, "vec": 1}, {"lfree": 0, "vec": 1}, {"records": 2}, {"records": 2, "rec_long": 1},
                    {"records": 2, "vec": 2}, {"records": 2, "vec": 1, "rec_long": 1}, {"staged_minsum": 1}))
LAYERED_MINSUM = ({"hl_reg": 1, "hl_records": 1, "staged_minsum": 0, "vec": 4, "serial_levels": 512},
                  ({"hl_records": 0}, {"hl_reg": 0}, {"hl_records": 0, "vec": 2}, {"hl_records": 0, "vec": 1}, {"vec": 2}, {"vec": 1},
                   {"staged_minsum": 1}, {"staged_minsum": 1, "hl_reg": 0},
                   {"serial_levels": 1}, {"serial_levels": 1, "hl_records": 0}, {"serial_levels": 1, "hl_reg": 0}))   # row-serial mode
FLOODING_TANH = ({"cn_reg": 1}, ({"cn_reg": 0},))
LAYERED_OTHER = ({"hl_reg": 1, "serial_levels": 512}, ({"hl_reg": 0}, {"serial_levels": 1}, {"serial_levels": 1, "hl_reg": 0}))
NONE = ({}, ())                     # flooding Phi / A-Min* / 8-bit: one kernel, its workgroup size from the longest row


def choices(impl):
    if is_float_minsum(impl):
        return LAYERED_MINSUM if is_layered(impl) else FLOODING_MINSUM
    if is_layered(impl):
        return LAYERED_OTHER
    return FLOODING_TANH if impl.startswith("Tanh") else NONE


def batched_decoder(family, w, impl, group):
    dec = lt.LdpcDecoder(rc.code(family, w)[1], impl)
    dec.set("group_size", group)     # before the first decode: a workspace of one small group
    dec.set("latency", 0)            # the batched kernels at every batch size
    dec.set("latency_edge", 0)
    return dec


def check_premises(family, w, impl, its):
    print(f"{family} weight {w} {impl}: converged at {sorted(set(its[its >= 0].tolist()))}, {int((its < 0).sum())} failures")
    # (these hold for row_weight_cases.py's seeds and noise levels: whoever changes those re-establishes them)
    assert its[0] == 0                                             # frame 0: the pre-check
    assert len(set(its[its > 0].tolist())) >= 3                    # convergences spread over the iterations
    assert its[1] < 0 and (its < 0).any()                          # the noise-only frame fails


@pytest.mark.parametrize("w", rc.WEIGHTS)
@pytest.mark.parametrize("family", rc.FAMILIES)
def test_full_rows(oracle, family, w):
    """every implementation whose selector changes at w (row_weight_cases.DECODES): batches of 5 and 130 through the batched
    kernels, by default and under every execution choice that swaps the bucketed kernel for the general one -- one result,
    the reference's.  The frames put a smallest magnitude and a negative input into the LAST slot of a full row (argmin =
    w - 1, the top bit of the mask); the references show a pre-check hit, convergences at three or more iteration counts
    and failures."""
    assert rc.last_slot_argmins(family, w) >= 1 and rc.last_slot_negatives(family, w) >= 1
    llrs = rc.frames(family, w)
    for impl in rc.implementations(w):
        want = reference(oracle, family, w, impl)
        check_premises(family, w, impl, want[1])
        dec = batched_decoder(family, w, impl, rc.FRAMES)
        x = gpu_input(impl, llrs)
        flooding_minsum = is_float_minsum(impl) and not is_layered(impl)
        if flooding_minsum:
            assert (dec.get("row_records"), dec.get("record_flag_bits")) == expected_records(family, w, is_f64(impl)), impl
        defaults, sets = choices(impl)
        for opts in ({},) + sets:
            for k, v in {**defaults, **opts}.items():
                dec.set(k, v)
            for batch in BATCHES:
                got = dec.decode_batch(x[:batch], ITERATIONS, want_posterior=True)
                assert_same(got, want, batch, impl, (batch, opts))
            if flooding_minsum and opts.get("records") == 0:
                assert dec.get("row_records") == 0 and dec.get("record_flag_bits") == 0
        dec.close()


@pytest.mark.parametrize("w", [64, 65])
@pytest.mark.parametrize("family", rc.FAMILIES)
def test_small_batches_at_the_table_limit(oracle, family, w):
    """The sliced tables of the single-launch path (csrc/graph_tables.h:137) and the lane-per-edge tables (graph_tables.h:218:
    a row is one wavefront's lanes) are ready up to 64 edges.  With the default "latency" / "latency_edge", batches of 1, 8
    and 19 return the reference's result: at 64 from the single launch -- "last_group" is then the batch itself
    (latency_paths.hip:44) -- for Minsumf32 (decode_latency, whose tables device_decoder.hip:111-117 builds) and for
    HLMinsumf32, Phif64 and Minstarapproxi8 (decode_latency_edge, device_decoder.hip:143-151: the staircase code's 120 levels
    are within the 512 the layered form takes; up to 64 codewords, edge_latency_limit); at 65 neither path exists and the
    batched kernels take the call, in a group of at least 64."""
    llrs = rc.frames(family, w)
    for impl in ("Minsumf32", "HLMinsumf32", "Phif64", "Minstarapproxi8"):
        want = reference(oracle, family, w, impl)
        check_premises(family, w, impl, want[1])
        head = want[1][:SMALL[-1]]
        assert want[1][2] != 0 and (head > 0).any() and (head < 0).any()   # the small batches iterate, converge and fail
        dec = lt.LdpcDecoder(rc.code(family, w)[1], impl)
        x = gpu_input(impl, llrs)
        for batch in SMALL:
            sl = slice(2, 3) if batch == 1 else slice(0, batch)      # (the single codeword: one that iterates, not frame 0)
            got = dec.decode_batch(x[sl], ITERATIONS, want_posterior=True)
            assert_same(got, want, sl, impl, ("small batch", batch))
            assert (dec.get("last_group") == batch) == (w == 64), (impl, batch)
        dec.close()


def test_regular_6_32(oracle):
    """every row 32 edges, every column 6 (the shape of the 10GBASE-T code): the 32-bit sign mask with its top bit in every row,
    the 32-edge layered bucket, no L-free variable -- 200 frames, both schedules, floats and 8-bit"""
    family = "regular_6_32"
    llrs = rc.frames(family)
    a = rc.code(family)[1]
    for impl in rc.REGULAR_6_32:
        want = reference(oracle, family, None, impl)
        check_premises(family, 32, impl, want[1])
        dec = batched_decoder(family, None, impl, 256)
        if impl.startswith("Minsumf"):
            assert dec.get("row_records") == 0 and dec.get("record_flag_bits") == 0
        got = dec.decode_batch(gpu_input(impl, llrs), ITERATIONS, want_posterior=True)
        assert_same(got, want, len(llrs), impl, "batch 200")
        dec.close()


def test_regular_6_32_compaction_and_device_entry(oracle):
    """Minsumf32 without L-free variables through a batch compaction -- 640 frames in one group, the 448 calm ones in the leading
    slots: at the first checkpoint (iteration 6) at most 192 frames live, 256 of 640 slots stay and every live codeword
    moves, with its per-edge messages (test_record_flags_gpu.py's test_flags_travel_with_a_compaction states the plan's
    rule) -- and through the device-resident entry."""
    import torch
    family, impl, iterations = "regular_6_32", "Minsumf32", 20
    llrs = rc.compaction_frames()
    total = rc.CALM_FRAMES + rc.BUSY_FRAMES
    want = rc.cpu_decode(oracle, family, None, impl, llrs, iterations)
    calm, busy = want[1][:rc.CALM_FRAMES], want[1][rc.CALM_FRAMES:]
    late = int(((busy < 0) | (busy >= 9)).sum())
    print(f"calm frames converge at {sorted(set(calm.tolist()))}, busy at {sorted(set(busy.tolist()))}, {late} busy frames live "
          f"beyond iteration 8, {int((busy >= 9).sum())} of them converge")
    assert calm.min() >= 0 and calm.max() <= 3          # done well before the first checkpoint
    assert late >= 8 and (busy >= 9).sum() >= 3         # moved codewords: some converge later, from the moved messages
    dec = batched_decoder(family, None, impl, total)
    for compact in (1, 0):
        dec.set("compact", compact)
        got = dec.decode_batch(llrs, iterations, want_posterior=True)
        assert_same(got, want, total, impl, ("compact", compact))
    host = got
    d_llrs = torch.from_numpy(llrs.copy()).cuda()          # (the frames are read-only)
    d_bits = torch.zeros((total, dec.n), dtype=torch.uint8, device="cuda")
    d_its = torch.zeros(total, dtype=torch.int32, device="cuda")
    d_post = torch.zeros((total, dec.n), dtype=torch.float32, device="cuda")
    dec.set("compact", 1)
    dec.decode_batch_device(d_llrs.data_ptr(), False, total, iterations, d_bits.data_ptr(), dec.n, d_its.data_ptr(),
                            d_post.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_same((d_bits.cpu().numpy(), d_its.cpu().numpy(), d_post.cpu().numpy()), host, total, impl, "device entry")
    dec.close()
