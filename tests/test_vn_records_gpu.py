"""Flooding min-sum with the variable nodes summed from the ROW RECORDS ("vn_records" = 1: vn_kernel's record form gathers, per kept
edge, the record of the edge's row, and the check-node launch stores no per-edge messages) against the message form
("vn_records" = 0) and the CPU reference: hard decisions, iteration counts and posterior LLRs with np.array_equal -- no
tolerance -- and "last_vn_records" says which form ran.

The codes are vn_records_cases.py's synthetic staircase codes of about a hundred columns (kept variables of weight 3, 8, 9
and 13; rows of 4 to 7 and of exactly 12 edges; the 13-edge-row twin, on which the form must not engage) and one DVB-S2
short frame.  The references are computed once per (code, rule, iteration limit) on the CPU and shared; a GPU decode is a
sub-millisecond job."""
import functools
import itertools

import numpy as np
import pytest

import corrected_minsum_restatement as cm
import ldpc_toolbox_amd as lt
from frames import alist, awgn_frames
from vn_records_cases import frames, staircase_code

pytestmark = pytest.mark.gpu

RULES = ("Minsumf32", "NormMinsumf32", "OffsetMinsumf32", "Minsumf64")
LIMITS = (20, 8, 1)     # checkpoints and re-packing active (12 and more) / none / only the FIRST launches


def is_f64(rule):
    return rule.endswith("f64")


def batches(rule):
    """around the 256-codeword tile of f32 and the 128-codeword tile of f64, partial packs, several slices"""
    return (127, 128, 129) if is_f64(rule) else (1, 3, 255, 256, 257, 300)


def vecs(rule):
    return (1, 2) if is_f64(rule) else (1, 2, 4)


@functools.lru_cache(maxsize=None)
def reference(oracle, wmax, rule, limit):
    """(bits, iterations, posterior) of all FRAMES frames: the oracle for plain min-sum, the numpy restatement of the
    corrected min-sum tests for the normalized and the offset rule, which the oracle does not have"""
    a = staircase_code(wmax)[2]
    if rule.startswith(("Norm", "Offset")):
        bits, its, post = cm.decode(a, rule, frames(wmax), limit)
    else:
        bits, its, post = oracle.decode_batch(oracle.Graph(a), rule, frames(wmax), limit, threads=8)
    return bits, its, post if is_f64(rule) else post.astype(np.float32)


def gpu_input(rule, llrs):
    return llrs.astype(np.float64) if is_f64(rule) else np.ascontiguousarray(llrs)


def decoder_pair(a, rule):
    """the same code twice: the message form and the record form"""
    pair = []
    for form in (0, 1):
        dec = lt.LdpcDecoder(a, rule)
        dec.set("latency", 0)              # the batched kernels at every batch size
        dec.set("vn_records", form)
        pair.append(dec)
    return pair


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


def assert_same(got, want, index, what):
    assert np.array_equal(got[1], want[1][index]), ("iterations", what)
    assert np.array_equal(got[0], want[0][index]), ("bits", what)
    assert got[2].dtype == want[2].dtype
    assert np.array_equal(got[2], want[2][index]), ("posterior", what)


CASES = [(rule, batch) for rule in RULES for batch in batches(rule)]


@pytest.mark.parametrize("rule,batch", CASES)
def test_record_source_is_invisible(oracle, rule, batch):
    """every pack width, with and without checkpoints, a one-iteration call, both entries: the two forms return the
    reference's bits, iteration counts and posterior, and each says which form it ran"""
    wmax = 12
    pair = decoder_pair(staircase_code(wmax)[2], rule)
    for dec in pair:
        assert dec.get("row_records") == 3 and dec.get("record_flag_bits") == 16
        dec.set("group_size", batch)
    llrs = gpu_input(rule, frames(wmax)[:batch])
    index = slice(0, batch)
    for limit in LIMITS:
        want = reference(oracle, wmax, rule, limit)
        if limit == 20 and batch >= 127:
            spread = want[1][index][want[1][index] >= 0]
            assert spread.max() - spread.min() >= 8     # convergences spread over the iterations: a premise of the frames
        for vec, device_entry in itertools.product(vecs(rule), (False, True)):
            for form, dec in enumerate(pair):
                dec.set("vec", vec)
                got = decode(dec, llrs, limit, device_entry)
                assert dec.get("last_vn_records") == form, (limit, vec, device_entry)
                assert_same(got, want, index, (form, limit, vec, device_entry))


@pytest.mark.parametrize("rule", ["Minsumf32", "Minsumf64"])
def test_thirteen_edge_rows_keep_the_message_form(oracle, rule):
    """rows of 13 edges have their flags in the record's third word: the key changes nothing, the read-back says 0"""
    wmax = 13
    pair = decoder_pair(staircase_code(wmax)[2], rule)
    batch = 129
    llrs = gpu_input(rule, frames(wmax)[:batch])
    want = reference(oracle, wmax, rule, 20)
    for form, dec in enumerate(pair):
        assert dec.get("row_records") == 3 and dec.get("record_flag_bits") == (64 if is_f64(rule) else 32)
        for vec in vecs(rule):
            dec.set("vec", vec)
            got = decode(dec, llrs, 20, False)
            assert dec.get("last_vn_records") == 0
            assert_same(got, want, slice(0, batch), (form, vec))


@pytest.mark.parametrize("rule", RULES)
def test_group_that_converges_inside_one_variable_node_launch(oracle, rule):
    """groups of one, two and three frames that all converge at the same iteration: the launch that latches them also
    rebuilds their L-free posteriors from the records of the latched iteration -- the other record buffer than the one
    the kept variables are summed from -- inside the launch ("vn_event" 1) or in a launch of its own (0), with the L-free
    stores deferred ("rec_quiet" 1) or not"""
    wmax = 12
    want = reference(oracle, wmax, rule, 20)
    its = want[1]
    at = max(range(2, 20), key=lambda i: int((its == i).sum()))     # the busiest iteration from 2 on
    same = np.flatnonzero(its == at)
    assert len(same) >= 3
    pair = decoder_pair(staircase_code(wmax)[2], rule)
    for count in (1, 2, 3):
        index = same[:count]
        llrs = gpu_input(rule, frames(wmax)[index])
        for vn_event, quiet, device_entry in itertools.product((1, 0), (1, 0), (False, True)):
            for form, dec in enumerate(pair):
                dec.set("vn_event", vn_event)
                dec.set("rec_quiet", quiet)
                got = decode(dec, llrs, 20, device_entry)
                assert dec.get("last_vn_records") == form
                assert_same(got, want, index, (form, count, vn_event, quiet, device_entry))


@pytest.mark.parametrize("rule", ["Minsumf32", "Minsumf64"])
def test_one_dvbs2_short_frame(oracle, rule):
    """DVB-S2 1/2 short (n = 16200, rows of at most 7 edges, kept variables of weight 3 and 8): one frame"""
    spec = "dvbs2:R1_2short"
    _, llrs, full = awgn_frames(spec, 1, 1.7, 4242)
    obits, oits, opost = oracle.decode_batch(oracle.Graph(alist(spec)), rule, full, 20, threads=1)
    want = (obits, oits, opost if is_f64(rule) else opost.astype(np.float32))
    assert oits[0] > 1
    for form, dec in enumerate(decoder_pair(alist(spec), rule)):
        assert dec.get("record_flag_bits") == 16
        for device_entry in (False, True):
            got = decode(dec, gpu_input(rule, llrs), 20, device_entry)
            assert dec.get("last_vn_records") == form
            assert_same(got, want, slice(0, 1), (form, device_entry))
