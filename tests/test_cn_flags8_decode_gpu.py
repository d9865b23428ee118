"""The byte form of the flooding min-sum check-node kernel (cn_minsum_rec_kernel with F8: seven loads in flight, the signs and
the running argmin in one register, a loaded record's argmins decoded once -- csrc/record_flags8.h, record_flags8_value)
against the CPU reference and against the same decoder with "flags8" 0, bit for bit: hard decisions, iteration counts and
posterior LLRs with np.array_equal, no tolerance, and "last_record_flag_bytes" says in every call that the byte form ran.

Codes and frames: cn_flags8_decode_cases.py -- staircase codes whose longest rows have 3, 4, 5, 6 and 7 edges (rows shorter
than the seven slots, and rows that fill them) and a hand-built code of 7-edge rows with a degree-1 variable, pairs of
degree-2 variables on the same two rows, far peers, and five runs of the kernel's walk.  Every batch mixes frames that
converge early with frames that never do (lanes with some codewords frozen; slices that start storing the L-free posteriors)
and has ties, zeros, NaNs and, at w = 7, infinities.  The references are computed once per (code, rule, iteration limit)."""
import functools
import itertools

import numpy as np
import pytest

import corrected_minsum_restatement as cm
import ldpc_toolbox_amd as lt
from cn_flags8_decode_cases import CODES, ORACLE_ALWAYS, ORACLE_ONCE, code, frames

pytestmark = pytest.mark.gpu

RULES = ("Minsumf32", "Minsumf64", "NormMinsumf32", "OffsetMinsumf32")
BATCHES = (1, 65, 257)
LIMITS = (1, 2, 5, 40)          # 40: enough for every frame that converges at all (asserted from the reference)


def is_f64(rule):
    return rule.endswith("f64")


def vecs(rule):
    return (1, 2) if is_f64(rule) else (1, 2, 4)


@functools.lru_cache(maxsize=None)
def reference(oracle, name, rule, limit):
    """(frame indices, bits, iterations, posterior) of the frames the CPU reference holds for at this limit"""
    llrs, kind = frames(name)
    index = np.flatnonzero((kind == ORACLE_ALWAYS) | ((kind == ORACLE_ONCE) & (limit == 1)))
    a = code(name)[2]
    if rule.startswith(("Norm", "Offset")):
        bits, its, post = cm.decode(a, rule, llrs[index], limit)
    else:
        bits, its, post = oracle.decode_batch(oracle.Graph(a), rule, llrs[index], limit, threads=8)
    assert not np.isnan(post).any()
    return index, bits, its, (post if is_f64(rule) else post.astype(np.float32))


def decoder(name, rule, flags8, vn_records):
    dec = lt.LdpcDecoder(code(name)[2], rule)
    dec.set("latency", 0)              # the batched kernels at every batch size
    dec.set("flags8", flags8)
    dec.set("vn_records", vn_records)
    assert dec.get("flags8") == flags8 and dec.get("row_records") == 3
    return dec


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", CODES)
def test_byte_form_decodes_as_the_reference_and_as_the_half_word_form(oracle, name, rule):
    llrs, kind = frames(name)
    llrs = np.array(llrs, dtype=np.float64 if is_f64(rule) else np.float32)
    word = np.uint64 if is_f64(rule) else np.uint32
    # premises of the frames, from the reference alone: early convergences, later ones, failures
    its = reference(oracle, name, rule, LIMITS[-1])[2]
    early, late, failed = int(((its > 0) & (its <= 3)).sum()), int((its > 3).sum()), int((its < 0).sum())
    print(f"{name} {rule}: {early} frames converge within 3 iterations, {late} later (last at {its.max()}), {failed} never")
    assert early >= 20 and failed >= 20
    for vn_records in (0, 1):
        byte, half = decoder(name, rule, 1, vn_records), decoder(name, rule, 0, vn_records)
        for batch, limit, vec in itertools.product(BATCHES, LIMITS, vecs(rule)):
            what = (vn_records, batch, limit, vec)
            got = {}
            for flags8, dec in ((1, byte), (0, half)):
                dec.set("vec", vec)
                got[flags8] = dec.decode_batch(llrs[:batch], limit, want_posterior=True)
                assert dec.get("last_record_flag_bytes") == (1 if flags8 else 2), what
                assert dec.get("last_vn_records") == vn_records, what
            # the same decoder with half-word flags: every frame, NaNs included, bit pattern for bit pattern
            assert np.array_equal(got[1][1], got[0][1]), ("iterations, against flags8 = 0", what)
            assert np.array_equal(got[1][0], got[0][0]), ("bits, against flags8 = 0", what)
            assert np.array_equal(got[1][2].view(word), got[0][2].view(word)), ("posterior, against flags8 = 0", what)
            # the CPU reference
            index, bits, its, post = reference(oracle, name, rule, limit)
            here = index < batch
            at = index[here]
            assert np.array_equal(got[1][1][at], its[here]), ("iterations", what)
            assert np.array_equal(got[1][0][at], bits[here]), ("bits", what)
            assert got[1][2].dtype == post.dtype
            assert np.array_equal(got[1][2][at], post[here]), ("posterior", what)
