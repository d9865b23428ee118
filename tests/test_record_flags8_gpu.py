"""Flooding min-sum row records with BYTE flags ("flags8" = 1 on rows of at most 7 edges: the flip bits and argmin bit 0 in
one byte per row and codeword, argmin bits 1 and 2 in the sign bits of the stored min1 and min2 -- csrc/record_flags8.h)
against the 16-bit form ("flags8" = 0) and the CPU reference, in the message form and the record form of the variable-node
launch ("vn_records" 0 / 1): hard decisions, iteration counts and posterior LLRs with np.array_equal -- no tolerance -- and
"last_record_flag_bytes" says in every call which form ran.

The codes are record_flags8_cases.py's synthetic staircase codes (rows of 4 to 7 edges, kept columns of weight 3, 8, 9 and
13; the 8-edge-row twin, on which the form must not engage) and one DVB-S2 short frame.  The references are computed once
per (code, rule, iteration limit) on the CPU and shared; a GPU decode is a sub-millisecond job."""
import functools
import itertools

import numpy as np
import pytest

import corrected_minsum_restatement as cm
import ldpc_toolbox_amd as lt
from frames import alist, awgn_frames
from record_flags8_cases import WMAX, frames, infinite_frames, nan_frames, quantised_frames, staircase_code

pytestmark = pytest.mark.gpu

RULES = ("Minsumf32", "NormMinsumf32", "OffsetMinsumf32", "Minsumf64")
LIMITS = (20, 8, 1)     # checkpoints move byte flags (12 and more) / none / only the FIRST launches
FORMS = tuple(itertools.product((0, 1), (0, 1)))    # ("flags8", "vn_records")


def is_f64(rule):
    return rule.endswith("f64")


def batches(rule):
    """around the 256-codeword tile of f32 and the 128-codeword tile of f64, partial packs, several slices"""
    return (127, 128, 129) if is_f64(rule) else (1, 3, 255, 256, 257, 300)


def vecs(rule):
    return (1, 2) if is_f64(rule) else (1, 2, 4)


def cpu_decode(oracle, a, rule, llrs, limit):
    """the oracle for plain min-sum, the numpy restatement of the corrected min-sum tests for the normalized and the
    offset rule, which the oracle does not have"""
    if rule.startswith(("Norm", "Offset")):
        bits, its, post = cm.decode(a, rule, llrs, limit)
    else:
        bits, its, post = oracle.decode_batch(oracle.Graph(a), rule, llrs, limit, threads=8)
    return bits, its, post if is_f64(rule) else post.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(oracle, wmax, rule, limit, which="awgn"):
    """(bits, iterations, posterior) of a whole frame set of record_flags8_cases.py"""
    llrs = {"awgn": lambda: frames(wmax), "quantised": quantised_frames, "infinite": infinite_frames}[which]()
    return cpu_decode(oracle, staircase_code(wmax)[2], rule, llrs, limit)


def gpu_input(rule, llrs):
    return np.array(llrs, dtype=np.float64 if is_f64(rule) else np.float32)      # (a writable copy: the frames are read-only)


def decoders(a, rule, forms=FORMS):
    """the same code once per ("flags8", "vn_records")"""
    out = []
    for flags8, vn_records in forms:
        dec = lt.LdpcDecoder(a, rule)
        dec.set("latency", 0)              # the batched kernels at every batch size
        dec.set("flags8", flags8)
        dec.set("vn_records", vn_records)
        assert dec.get("flags8") == flags8
        out.append(dec)
    return out


def decode(dec, llrs, limit, device_entry):
    """host entry, or the device entry on a stream of the caller's"""
    if not device_entry:
        return dec.decode_batch(llrs, limit, want_posterior=True)
    import torch
    batch = llrs.shape[0]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_llrs = torch.from_numpy(llrs).cuda()
        d_bits = torch.zeros((batch, dec.n), dtype=torch.uint8, device="cuda")
        d_its = torch.zeros(batch, dtype=torch.int32, device="cuda")
        d_post = torch.zeros((batch, dec.n), dtype=d_llrs.dtype, device="cuda")
        stream.synchronize()
        dec.decode_batch_device(d_llrs.data_ptr(), llrs.dtype == np.float64, batch, limit, d_bits.data_ptr(), dec.n,
                                d_its.data_ptr(), d_post.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        return d_bits.cpu().numpy(), d_its.cpu().numpy(), d_post.cpu().numpy()


def assert_ran(dec, form, what):
    flags8, vn_records = form
    assert dec.get("last_record_flag_bytes") == (1 if flags8 else 2), what
    assert dec.get("last_vn_records") == vn_records, what


def assert_same(got, want, index, what):
    assert np.array_equal(got[1], want[1][index]), ("iterations", what)
    assert np.array_equal(got[0], want[0][index]), ("bits", what)
    assert got[2].dtype == want[2].dtype
    assert np.array_equal(got[2], want[2][index]), ("posterior", what)


CASES = [(rule, batch) for rule in RULES for batch in batches(rule)]


@pytest.mark.parametrize("rule,batch", CASES)
def test_byte_flags_are_invisible(oracle, rule, batch):
    """every pack width (one b8 / b16 / b32 access of flags per lane), with and without checkpoints, a one-iteration call,
    both entries: the four forms return the reference's bits, iteration counts and posterior, and each says what it ran"""
    quad = decoders(staircase_code(WMAX)[2], rule)
    for dec in quad:
        assert dec.get("row_records") == 3 and dec.get("record_flag_bits") == 16     # the family keeps its name
        dec.set("group_size", batch)
    llrs = gpu_input(rule, frames(WMAX)[:batch])
    index = slice(0, batch)
    for limit in LIMITS:
        want = reference(oracle, WMAX, rule, limit)
        if limit == 20 and batch >= 127:
            spread = want[1][index][want[1][index] >= 0]
            assert spread.max() - spread.min() >= 8     # convergences spread over the iterations: a premise of the frames
        for vec, device_entry in itertools.product(vecs(rule), (False, True)):
            for form, dec in zip(FORMS, quad):
                dec.set("vec", vec)
                got = decode(dec, llrs, limit, device_entry)
                assert_ran(dec, form, (limit, vec, device_entry))
                assert_same(got, want, index, (form, limit, vec, device_entry))


@pytest.mark.parametrize("rule", ["Minsumf32", "Minsumf64"])
def test_eight_edge_rows_keep_half_words(oracle, rule):
    """rows of 8 edges need 8 flip bits and 3 argmin bits: the key changes nothing, the read-back says 2"""
    wmax = 8
    batch = 129
    llrs = gpu_input(rule, frames(wmax)[:batch])
    want = reference(oracle, wmax, rule, 20)
    for form, dec in zip(FORMS, decoders(staircase_code(wmax)[2], rule)):
        assert dec.get("row_records") == 3 and dec.get("record_flag_bits") == 16
        for vec in vecs(rule):
            dec.set("vec", vec)
            got = decode(dec, llrs, 20, False)
            assert_ran(dec, (0, form[1]), (form, vec))
            assert_same(got, want, slice(0, batch), (form, vec))


def test_long_row_variant_keeps_half_words(oracle):
    """"rec_long" takes the record kernel's long-row variant, which has no byte form: every launch of the call stays with
    the 16-bit form"""
    batch = 257
    llrs = frames(WMAX)[:batch]
    want = reference(oracle, WMAX, "Minsumf32", 20)
    for form, dec in zip(FORMS, decoders(staircase_code(WMAX)[2], "Minsumf32")):
        dec.set("rec_long", 1)
        got = decode(dec, llrs, 20, False)
        assert_ran(dec, (0, form[1]), form)
        assert_same(got, want, slice(0, batch), form)
        dec.set("rec_long", 0)
        got = decode(dec, llrs, 20, False)
        assert_ran(dec, form, form)
        assert_same(got, want, slice(0, batch), form)


@pytest.mark.parametrize("rule", RULES)
def test_group_that_converges_inside_one_variable_node_launch(oracle, rule):
    """groups of one, two and three frames that all converge at the same iteration: the launch that latches them also
    rebuilds their L-free posteriors from the records of the latched iteration -- the OTHER record buffer, byte flags
    included -- inside the launch ("vn_event" 1) or in a launch of its own (0), with the L-free stores deferred
    ("rec_quiet" 1) or not"""
    want = reference(oracle, WMAX, rule, 20)
    its = want[1]
    at = max(range(2, 20), key=lambda i: int((its == i).sum()))     # the busiest iteration from 2 on
    same = np.flatnonzero(its == at)
    assert len(same) >= 3
    quad = decoders(staircase_code(WMAX)[2], rule)
    for count in (1, 2, 3):
        index = same[:count]
        llrs = gpu_input(rule, frames(WMAX)[index])
        for vn_event, quiet, device_entry in itertools.product((1, 0), (1, 0), (False, True)):
            for form, dec in zip(FORMS, quad):
                dec.set("vn_event", vn_event)
                dec.set("rec_quiet", quiet)
                got = decode(dec, llrs, 20, device_entry)
                assert_ran(dec, form, (count, vn_event, quiet, device_entry))
                assert_same(got, want, index, (form, count, vn_event, quiet, device_entry))


@pytest.mark.parametrize("rule", RULES)
def test_ties_zeros_and_infinite_llrs(oracle, rule):
    """LLRs in multiples of 0.5 with exact +-0.0 and a few +-inf among them: rows with min1 == min2, with zero magnitudes
    (for the offset rule also after the correction's clamp), variables whose posterior is infinite -- against the CPU"""
    quad = decoders(staircase_code(WMAX)[2], rule)
    llrs = gpu_input(rule, quantised_frames())
    index = slice(0, llrs.shape[0])
    for limit in (20, 1):
        want = reference(oracle, WMAX, rule, limit, "quantised")
        assert not np.isnan(want[2]).any()
        for vec in vecs(rule):
            for form, dec in zip(FORMS, quad):
                dec.set("vec", vec)
                got = decode(dec, llrs, limit, False)
                assert_ran(dec, form, (limit, vec))
                assert_same(got, want, index, (form, limit, vec))


@pytest.mark.parametrize("rule", RULES)
def test_infinite_magnitudes_in_one_iteration(oracle, rule):
    """frames that are +inf but for a few LLRs: rows whose min2, or both minima, are +inf -- stored with a stolen sign bit
    beside an all-ones exponent -- in a one-iteration decode, whose L-free posteriors are read out of those records"""
    quad = decoders(staircase_code(WMAX)[2], rule)
    llrs = gpu_input(rule, infinite_frames())
    want = reference(oracle, WMAX, rule, 1, "infinite")
    assert np.isinf(want[2]).any() and not np.isnan(want[2]).any()
    for vec in vecs(rule):
        for form, dec in zip(FORMS, quad):
            dec.set("vec", vec)
            got = decode(dec, llrs, 1, False)
            assert_ran(dec, form, vec)
            assert_same(got, want, slice(0, llrs.shape[0]), (form, vec))


@pytest.mark.parametrize("rule", RULES)
def test_nan_llrs_decode_as_in_the_half_word_form(rule):
    """NaN LLRs (and the inf - inf of the infinite frames' later iterations): the byte form against the 16-bit form, which
    the rest of the suite pins -- bits, iteration counts and the posterior's bit patterns"""
    llrs = gpu_input(rule, nan_frames())
    word = np.uint64 if is_f64(rule) else np.uint32
    for vn_records in (0, 1):
        half, byte = decoders(staircase_code(WMAX)[2], rule, ((0, vn_records), (1, vn_records)))
        for limit, vec in itertools.product((20, 2), vecs(rule)):
            out = []
            for flags8, dec in ((0, half), (1, byte)):
                dec.set("vec", vec)
                out.append(decode(dec, llrs, limit, False))
                assert_ran(dec, (flags8, vn_records), (limit, vec))
            assert np.isnan(out[0][2]).any()
            assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), (vn_records, limit, vec)
            assert np.array_equal(out[0][2].view(word), out[1][2].view(word)), (vn_records, limit, vec)


@pytest.mark.parametrize("rule", ["Minsumf32", "Minsumf64"])
def test_one_dvbs2_short_frame(oracle, rule):
    """DVB-S2 1/2 short (n = 16200, rows of at most 7 edges, kept variables of weight 3 and 8): one frame"""
    spec = "dvbs2:R1_2short"
    _, llrs, full = awgn_frames(spec, 1, 1.7, 4242)
    obits, oits, opost = oracle.decode_batch(oracle.Graph(alist(spec)), rule, full, 20, threads=1)
    want = (obits, oits, opost if is_f64(rule) else opost.astype(np.float32))
    assert oits[0] > 1
    for form, dec in zip(FORMS, decoders(alist(spec), rule)):
        assert dec.get("record_flag_bits") == 16
        for device_entry in (False, True):
            got = decode(dec, gpu_input(rule, llrs), 20, device_entry)
            assert_ran(dec, form, device_entry)
            assert_same(got, want, slice(0, 1), (form, device_entry))
