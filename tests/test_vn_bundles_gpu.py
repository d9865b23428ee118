"""The record form of the variable-node launch with its kept list in BUNDLES ("vn_bundles" = 1: the list entries the waves of a
workgroup sum in the same step share rows -- csrc/graph_tables.h, build_vn_bundles) against the same decoder with the list in
variable order ("vn_bundles" = 0) and against the CPU reference: hard decisions, iteration counts and posterior LLRs with
np.array_equal, no tolerance.  "last_vn_bundles" says in every call which order ran, "vn_bundle_saved_permille" what it is
worth at that call's bundle width.

Codes: cn_flags8_decode_cases.py's staircase codes whose longest rows have 3 to 7 edges, and a code dealt here with kept
variables of weight 3, 4 and 8 -- 53 of them: no multiple of a bundle, and no weight class is one.  300 frames (a full
256-codeword tile and a tail) and 8 iterations at two noise levels: one at which frames converge inside the run, spread over
its iterations (the latch, the event block that rebuilds the L-free posteriors, slices that start storing them), and one at
which none does (chosen by the reference).  f32 and f64, byte and half-word record flags, and every pack width: it sets how
many list entries a workgroup's waves share -- 4, 2 or 1.  (staircase3's rows but the first hold one kept variable each:
next to nothing to share there.)"""
import functools
import itertools

import numpy as np
import pytest

import ldpc_toolbox_amd as lt
from cn_flags8_decode_cases import staircase
from encoder_reference import alist_from_rows

pytestmark = pytest.mark.gpu

RULES = ("Minsumf32", "Minsumf64")
CODES = ("staircase3", "staircase4", "staircase5", "staircase6", "staircase7", "mixed")
BATCH, LIMIT = 300, 8
SEED = 40389
SIGMA_CALM, SIGMA_BUSY = 0.7, 2.5
MIXED_ROWS = 48


def is_f64(rule):
    return rule.endswith("f64")


def vecs(rule):
    return (2, 1) if is_f64(rule) else (4, 2, 1)


def bundle_width(rule, vec):
    """list entries the waves of a 256-thread workgroup sum side by side: its four waves over the slices of a tile (256
    codewords of f32, 128 of f64; a slice is 64 * vec of them)"""
    slices = (128 if is_f64(rule) else 256) // (64 * vec)
    return max(1, 4 // slices)


@functools.lru_cache(maxsize=None)
def mixed_code():
    """(n, rows, alist): [H0 | bidiagonal] on 48 rows of 5 to 7 edges; information columns of weight 8 (five), 4 and 3, the
    heaviest dealt first, each to the rows with the most room left"""
    cycle = (7, 5, 6, 7, 6, 5)
    lengths = [cycle[r % len(cycle)] for r in range(MIXED_ROWS)]
    slots = [w - (2 if r else 1) for r, w in enumerate(lengths)]
    rest = sum(slots) - 5 * 8
    fours = next(a for a in range(6, 12) if (rest - 4 * a) % 3 == 0 and (5 + a + (rest - 4 * a) // 3) % 4 != 0)
    weights = [8] * 5 + [4] * fours + [3] * ((rest - 4 * fours) // 3)
    K = len(weights)
    assert K % 4 != 0 and all(weights.count(w) % 4 != 0 for w in (3, 4, 8))
    # interleave the weights along the variable order: the list's first order has no degree runs
    order = np.random.default_rng(SEED).permutation(K).tolist()
    rng = np.random.default_rng(SEED + 1)
    h0, left = [[] for _ in range(MIXED_ROWS)], list(slots)
    for j in sorted(range(K), key=lambda j: -weights[j]):
        rows = rng.permutation(MIXED_ROWS).tolist()
        rows.sort(key=lambda r: -left[r])
        take = rows[:weights[j]]
        assert all(left[r] > 0 for r in take), "the rows cannot take this column"
        for r in take:
            h0[r].append(order[j])
            left[r] -= 1
    assert not any(left)
    rows = [sorted(h0[r]) + ([K + r - 1] if r else []) + [K + r] for r in range(MIXED_ROWS)]
    assert [len(r) for r in rows] == lengths
    col_w = np.bincount([c for r in rows for c in r], minlength=K + MIXED_ROWS)
    assert sorted(set(col_w[:K].tolist())) == [3, 4, 8] and set(col_w[K:].tolist()) == {1, 2}
    return K + MIXED_ROWS, rows, alist_from_rows(K + MIXED_ROWS, rows)


def code(name):
    return mixed_code() if name == "mixed" else staircase(int(name[-1]))


@functools.lru_cache(maxsize=None)
def sharing(name):
    """(some row holds two kept variables, the first kept variable shares a row with another of its own weight) -- from the
    rows alone.  The second: the first bundle's seed is the list's first entry and every other entry is still free, so the
    bundle's second entry shares a row with it -- the first aligned pair spares a fetch, at every bundle width from 2 on."""
    n, rows, _ = code(name)
    weight = np.bincount([c for r in rows for c in r], minlength=n)
    kept = [[c for c in r if weight[c] >= 3] for r in rows]
    first = min(c for r in kept for c in r)
    return (any(len(r) >= 2 for r in kept),
            any(first in r and any(c != first and weight[c] == weight[first] for c in r) for r in kept))


def awgn(rng, count, n, sigma):
    y = 1.0 + sigma * rng.standard_normal((count, n))
    return (2.0 * y / sigma ** 2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases(oracle, name, rule):
    """{noise level: (llrs [BATCH][n], bits, iterations, posterior)}: the frames and the CPU reference's outputs.  The busy
    level's frames are the first BATCH of a larger draw that the reference does not decode within LIMIT iterations."""
    n, _, a = code(name)
    graph = oracle.Graph(a)
    rng = np.random.default_rng([SEED, CODES.index(name)])
    out = {}
    for level, sigma, draw in (("calm", SIGMA_CALM, BATCH), ("busy", SIGMA_BUSY, 4 * BATCH)):
        llrs = awgn(rng, draw, n, sigma)
        bits, its, post = oracle.decode_batch(graph, rule, llrs, LIMIT, threads=8)
        if level == "busy":
            keep = np.flatnonzero(its < 0)[:BATCH]
            assert len(keep) == BATCH, "too few frames fail at the busy level"
            llrs, bits, its, post = llrs[keep], bits[keep], its[keep], post[keep]
        llrs = np.ascontiguousarray(llrs, dtype=np.float64 if is_f64(rule) else np.float32)
        post = post if is_f64(rule) else post.astype(np.float32)
        for x in (llrs, bits, its, post):
            x.setflags(write=False)
        out[level] = (llrs, bits, its, post)
    return out


def decoder(name, rule, flags8, bundles):
    dec = lt.LdpcDecoder(code(name)[2], rule)
    dec.set("latency", 0)              # the batched kernels at every batch size
    dec.set("vn_records", 1)
    dec.set("flags8", flags8)
    dec.set("vn_bundles", bundles)
    assert dec.get("row_records") == 3 and dec.get("record_flag_bits") == 16
    return dec


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", CODES)
def test_bundled_list_is_invisible(oracle, name, rule):
    ref = cases(oracle, name, rule)
    # premises of the frames, from the reference alone
    calm, busy = ref["calm"][2], ref["busy"][2]
    inside = calm[(calm >= 1) & (calm < LIMIT)]
    print(f"{name} {rule}: calm level: {len(inside)} frames converge inside the run, at iterations "
          f"{sorted(set(inside.tolist()))}, {(calm < 0).sum()} do not; busy level: {(busy >= 0).sum()} converge")
    assert len(inside) >= 20 and len(set(inside.tolist())) >= 3 and (calm < 0).sum() >= 1
    assert (busy < 0).all()
    word = np.uint64 if is_f64(rule) else np.uint32
    for flags8 in (1, 0):
        plain, bundled = decoder(name, rule, flags8, 0), decoder(name, rule, flags8, 1)
        saved_at = {}
        for level, vec in itertools.product(("calm", "busy"), vecs(rule)):
            what = (flags8, level, vec)
            llrs, bits, its, post = ref[level]
            got = {}
            for on, dec in ((0, plain), (1, bundled)):
                dec.set("vec", vec)
                got[on] = dec.decode_batch(llrs, LIMIT, want_posterior=True)
                assert dec.get("last_vn_records") == 1, what
                assert dec.get("last_record_flag_bytes") == (1 if flags8 else 2), what
                assert dec.get("last_vn_bundles") == on, what
                saved = dec.get("vn_bundle_saved_permille")
                if on:
                    saved_at[bundle_width(rule, vec)] = saved
                else:
                    assert saved == 0, what
            for on in (0, 1):
                assert np.array_equal(got[on][1], its), ("iterations", on, what)
                assert np.array_equal(got[on][0], bits), ("bits", on, what)
                assert got[on][2].dtype == post.dtype
                assert np.array_equal(got[on][2], post), ("posterior", on, what)
            assert np.array_equal(got[1][2].view(word), got[0][2].view(word)), ("posterior, against vn_bundles = 0", what)
        # what the order spares: nothing where a workgroup's waves all see other codewords, and a bundle of four spares at
        # least what its two pairs do (the distinct rows of a union are at most the sum over its parts)
        print(f"{name} {rule} flags8 {flags8}: saved per thousand record fetches, by bundle width: {saved_at}")
        any_shared, first_shares = sharing(name)
        assert saved_at.get(1, 0) == 0
        assert 0 <= saved_at[2] <= saved_at[4] < 1000
        if first_shares:
            assert saved_at[2] > 0
        if not any_shared:
            assert saved_at[4] == 0
