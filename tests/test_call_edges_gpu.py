"""The launches around a decode call's iterations with "call_edges" = 1 (csrc/device_decoder.h, opt_call_edges_) against the
same decoder with "call_edges" = 0 and against the CPU reference: hard decisions, iteration counts and, where asked for,
posterior LLRs with np.array_equal, no tolerance.  "last_call_edges" says in every call which shortcuts ran:

  1  the ingest launch stored no copy of the input in the posterior array
  2  the last pack covered the kept rows and the closing launch packed the L-free variables' decisions, storing no posterior
  4  the final emit launch was given the packed decisions
  8  a compaction checkpoint was enqueued as two launches behind its plan

1, 2 and 4 are for a call of the flooding record path that asks for no posterior; with a posterior the old launches must run and
the mask must say so.  With "call_edges" = 0 the mask is 0.

Codes: test_vn_bundles_gpu.py's `mixed` and `staircase7` (about a hundred columns) with that module's frames at its calm and
busy noise levels, and the smallest built-in code that is decoded punctured, CCSDS AR4JA rate 4/5 k = 1024 (n = 1408, its last
128 columns not transmitted).  At the calm level frames converge inside the run: frozen and live codewords share a slice in
the closing launch, and at 20 iterations the checkpoints (iterations 6 to 16) find a group worth re-packing and later one
that is not.  The references are computed once per (code, rule, limit) on the CPU and shared; a GPU decode is a
sub-millisecond job."""
import functools
import itertools

import numpy as np
import pytest

import ldpc_toolbox_amd as lt
from frames import alist, awgn_frames
from test_vn_bundles_gpu import BATCH, cases, code

pytestmark = pytest.mark.gpu

INGEST, CLOSE, EMIT, CHECKPOINT = 1, 2, 4, 8
NAMES = ("mixed", "staircase7")
RULES = ("Minsumf32", "Minsumf64")
LIMITS = (20, 8, 1, 0)   # checkpoints (12 and more) / none / only the FIRST launches / no iteration at all
AR4JA, AR4JA_PATTERN = "ar4ja:4/5:1024", "1,1,1,1,1,1,1,1,1,1,0"


def is_f64(rule):
    return rule.endswith("f64")


def vecs(rule):
    return (2, 1) if is_f64(rule) else (4, 2, 1)


@functools.lru_cache(maxsize=None)
def frames_of(oracle, name, rule, level):
    """the frames of test_vn_bundles_gpu at `level`; "clean": the busy frames with two noise-free all-zero codewords among them,
    which pass the pre-check (iterations = 0), one in the first tile and one in the tail"""
    llrs = cases(oracle, name, rule)["busy" if level == "clean" else level][0]
    if level == "clean":
        llrs = llrs.copy()
        llrs[1] = 4.0
        llrs[BATCH - 1] = 4.0
        llrs.setflags(write=False)
    return llrs


@functools.lru_cache(maxsize=None)
def reference(oracle, name, rule, level, limit):
    """(bits, iterations, posterior) of the CPU reference for all BATCH frames"""
    graph = oracle.Graph(code(name)[2])
    bits, its, post = oracle.decode_batch(graph, rule, frames_of(oracle, name, rule, level), limit, threads=8)
    post = post if is_f64(rule) else post.astype(np.float32)
    for x in (bits, its, post):
        x.setflags(write=False)
    return bits, its, post


def decoder_pair(a, rule, puncturing=""):
    """the same code twice, on the flooding record path: "call_edges" = 0 and 1"""
    pair = []
    for on in (0, 1):
        dec = lt.LdpcDecoder(a, rule, puncturing)
        dec.set("latency", 0)   # the batched kernels at every batch size
        dec.set("records", 2)
        assert dec.get("row_records") in (3, 4)
        assert dec.get("call_edges") == 1   # the default
        dec.set("call_edges", on)
        assert dec.get("call_edges") == on
        pair.append(dec)
    return pair


def expected_mask(limit, posterior, its):
    """what a call of the record path must report, from its arguments and the reference's iteration counts.  Returns
    (mask, bits of it that must match): the checkpoint bit is compared where the reference settles it -- a checkpoint is
    enqueued before iteration 7 if a frame is still running then, and none is with fewer than 12 iterations"""
    mask = 0 if posterior else (INGEST | (CLOSE | EMIT if limit > 0 else 0))
    care = INGEST | CLOSE | EMIT
    if limit < 12:
        care |= CHECKPOINT
    elif ((its < 0) | (its >= 7)).any():
        mask |= CHECKPOINT
        care |= CHECKPOINT
    return mask, care


def run(dec, llrs, limit, out_len, posterior, device_entry=False, shift=0):
    """one call -> (bits, iterations, posterior or None); shift: bytes between a dword boundary and the output's first byte"""
    batch = llrs.shape[0]
    if not device_entry:
        store = np.full(batch * out_len + 8, 0xAA, dtype=np.uint8)
        bits = store[shift:shift + batch * out_len].reshape(batch, out_len)
        its = np.zeros(batch, dtype=np.int32)
        out = (bits, its, np.zeros((batch, dec.n), dtype=llrs.dtype)) if posterior else (bits, its)
        got = dec.decode_batch(llrs, limit, output_len=out_len, want_posterior=posterior, out=out)
        assert (store[:shift] == 0xAA).all() and (store[shift + batch * out_len:] == 0xAA).all(), "bytes around the output"
        return got
    import torch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_llrs = torch.from_numpy(np.array(llrs)).cuda()   # (a copy: the shared frames are read-only)
        d_store = torch.full((batch * out_len + 8,), 0xAA, dtype=torch.uint8, device="cuda")
        d_its = torch.zeros(batch, dtype=torch.int32, device="cuda")
        d_post = torch.zeros((batch, dec.n), dtype=d_llrs.dtype, device="cuda") if posterior else None
        stream.synchronize()
        assert d_store.data_ptr() % 4 == 0
        dec.decode_batch_device(d_llrs.data_ptr(), llrs.dtype == np.float64, batch, limit, d_store.data_ptr() + shift, out_len,
                                d_its.data_ptr(), d_post.data_ptr() if posterior else 0, stream.cuda_stream)
        stream.synchronize()
        store = d_store.cpu().numpy()
    assert (store[:shift] == 0xAA).all() and (store[shift + batch * out_len:] == 0xAA).all(), "bytes around the output"
    return (store[shift:shift + batch * out_len].reshape(batch, out_len), d_its.cpu().numpy(),
            d_post.cpu().numpy() if posterior else None)


def check(pair, llrs, want, limit, out_len, posterior, what, **how):
    """both decoders against the reference (`want`, for exactly these frames) and against each other; the masks"""
    got = {}
    for on, dec in enumerate(pair):
        got[on] = run(dec, llrs, limit, out_len, posterior, **how)
        mask, care = expected_mask(limit, posterior, want[1])
        seen = dec.get("last_call_edges")
        assert seen == 0 if not on else (seen & care) == (mask & care), ("last_call_edges", seen, mask, on, what)
        assert np.array_equal(got[on][1], want[1]), ("iterations", on, what)
        assert np.array_equal(got[on][0], want[0][:, :out_len]), ("bits", on, what)
        if posterior:
            assert got[on][2].dtype == want[2].dtype
            assert np.array_equal(got[on][2], want[2]), ("posterior", on, what)
        else:
            assert got[on][2] is None
    assert np.array_equal(got[1][0], got[0][0]) and np.array_equal(got[1][1], got[0][1]), ("against call_edges = 0", what)


def sliced(want, count):
    return tuple(x[:count] for x in want)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", NAMES)
def test_trimmed_launches_are_invisible(oracle, name, rule):
    """every pack width, noise level and iteration limit, with and without a posterior; then the small batches, the output
    lengths, the entries and an output that starts off a dword boundary"""
    n, _, a = code(name)
    pair = decoder_pair(a, rule)
    k = pair[0].k
    assert 5 < k < n
    # premises, from the reference alone: at the calm level frames freeze inside a 20-iteration run while others go on past
    # the first checkpoints; a clean frame passes the pre-check
    calm20 = reference(oracle, name, rule, "calm", 20)[1]
    inside = calm20[(calm20 >= 1) & (calm20 < 20)]
    print(f"{name} {rule}: calm, 20 iterations: {len(inside)} frames converge inside, at {sorted(set(inside.tolist()))}; "
          f"{(calm20 < 0).sum()} do not")
    assert len(inside) >= 20 and (((calm20 < 0) | (calm20 >= 7)).any())
    clean8 = reference(oracle, name, rule, "clean", 8)[1]
    assert clean8[1] == 0 and clean8[BATCH - 1] == 0 and (clean8 < 0).sum() >= BATCH - 2

    for level, vec, limit, posterior in itertools.product(("calm", "busy"), vecs(rule), LIMITS, (False, True)):
        for dec in pair:
            dec.set("vec", vec)
        llrs, want = frames_of(oracle, name, rule, level), reference(oracle, name, rule, level, limit)
        check(pair, llrs, want, limit, n, posterior, (level, vec, limit, posterior))
    for dec in pair:
        dec.set("vec", 4)
    if not is_f64(rule):
        # f64 input to the f32 decoder (the values are f32 values: the same reference)
        for level, limit in itertools.product(("calm", "busy"), (20, 8)):
            llrs = frames_of(oracle, name, rule, level).astype(np.float64)
            check(pair, llrs, reference(oracle, name, rule, level, limit), limit, n, False, ("f64 input", level, limit))
    # a noise-free frame beside noisy ones: reported from the raw input's decisions, whatever the packed words hold
    for limit, out_len in itertools.product((20, 8, 1, 0), (n, 5)):
        llrs, want = frames_of(oracle, name, rule, "clean"), reference(oracle, name, rule, "clean", limit)
        check(pair, llrs, want, limit, out_len, False, ("clean", limit, out_len))
    # one tile and a tail above; one codeword and three; the output lengths; both entries; every start inside a dword
    for batch, out_len, limit, device_entry in itertools.product((1, 3, BATCH), (5, k, n), (20, 1), (False, True)):
        llrs = np.ascontiguousarray(frames_of(oracle, name, rule, "calm")[:batch])
        want = sliced(reference(oracle, name, rule, "calm", limit), batch)
        shift = (batch + out_len + limit) % 4 if device_entry else 0
        check(pair, llrs, want, limit, out_len, False, (batch, out_len, limit, device_entry, shift),
              device_entry=device_entry, shift=shift)
    for shift in (1, 2, 3):
        llrs, want = frames_of(oracle, name, rule, "calm"), reference(oracle, name, rule, "calm", 8)
        check(pair, llrs, want, 8, k, False, ("shift", shift), device_entry=True, shift=shift)
        check(pair, llrs, want, 8, n, True, ("shift, posterior", shift), device_entry=True, shift=shift)


@functools.lru_cache(maxsize=None)
def ar4ja_case(oracle, rule, limit):
    _, llrs, full = awgn_frames(AR4JA, BATCH, 3.9, 77, AR4JA_PATTERN)
    llrs, full = llrs.copy(), full.copy()
    dtype = np.float64 if is_f64(rule) else np.float32
    bits, its, post = oracle.decode_batch(oracle.Graph(alist(AR4JA)), rule, full.astype(dtype), limit, threads=8)
    return np.ascontiguousarray(llrs, dtype=dtype), (bits, its, post if is_f64(rule) else post.astype(np.float32))


@pytest.mark.parametrize("rule", RULES)
def test_punctured_code(oracle, rule):
    """depuncturing in the ingest launch that stores the input once; f32 and f64 input; a code whose L-free variables join
    distant rows and lie among the kept ones"""
    pair = decoder_pair(alist(AR4JA), rule, AR4JA_PATTERN)
    n, k = pair[0].n, pair[0].k
    assert pair[0].input_len == n - n // 11
    for limit in (20, 1, 0):
        llrs, want = ar4ja_case(oracle, rule, limit)
        if limit == 20:
            spread = want[1][want[1] >= 0]
            print(f"{AR4JA} {rule}: {len(spread)} of {BATCH} frames converge, at {sorted(set(spread.tolist()))}")
            assert len(spread) >= 20 and len(set(spread.tolist())) >= 3 and ((want[1] < 0) | (want[1] >= 7)).any()
        for out_len, posterior in ((n, False), (k, False), (5, False), (n, True)):
            check(pair, llrs, want, limit, out_len, posterior, (limit, out_len, posterior))
        check(pair, llrs, want, limit, k, False, (limit, "device"), device_entry=True, shift=3)
