"""The record form of the variable-node launch with its kept list in CHAINS ("vn_chains" = 1: a wave sums "vn_chain_len"
list entries one after the other and, where two consecutive ones share a row, takes that row's record from its registers and
not from memory -- csrc/graph_tables.h, build_vn_chains) against the same decoder with "vn_chains" = 0 and against the CPU
reference: hard decisions, iteration counts and posterior LLRs with np.array_equal, no tolerance.  "last_vn_chains" says in
every call which walk ran.

Codes, the smallest at which the carry can go wrong: test_vn_bundles_gpu.py's 48-row "mixed" code (53 kept variables of
weight 3, 4 and 8: no multiple of any block), staircase3 (next to nothing to chain) and staircase7.  300 frames (one full
tile and a tail) and 8 iterations at that module's two noise levels -- at the calm one frames converge inside the run, so the
latch and the event block run beside the carry; at the busy one none does -- in batches of 1, 3 and 300, f32 with packs of
4, 2 and 1 and f64 with packs of 2 and 1, byte and half-word record flags, chains of 4 and of 8.

chain_marks() walks the graph as build_vn_chains does, from the alist alone; what it counts must be what the decoder reports
("vn_chain_saved_permille"), and on the mixed code with chains of 8 it must mark, as the edge taken from the carry, a first,
a middle and a last edge of a variable's cols[v] order: the premise of that case, asserted."""
import functools
import heapq
import itertools

import numpy as np
import pytest

import ldpc_toolbox_amd as lt
from test_vn_bundles_gpu import BATCH, LIMIT, cases, code, is_f64, vecs

pytestmark = pytest.mark.gpu

RULES = ("Minsumf32", "Minsumf64")
CODES = ("mixed", "staircase3", "staircase7")
LENGTHS = (4, 8)
BATCHES = (1, 3, BATCH)
WIDTH, CHAIN_EDGES = 4, 8    # csrc: kVnBundleW, kChainEdges


@functools.lru_cache(maxsize=None)
def chain_marks(name, length):
    """(fetches, carried, issued, positions): the chained list of build_vn_chains(..., WIDTH, length), rebuilt here from the
    code's columns: the counts of count_vn_chain_fetches, and for every edge taken from the carry (its position in the
    variable's cols[v] order, the variable's weight)"""
    n, rows, _ = code(name)
    cols = [[] for _ in range(n)]
    for r, cs in enumerate(rows):        # cols[v] order: the alist's column lines, rows ascending
        for c in cs:
            cols[c].append(r)
    kept = [cols[v] for v in range(n) if len(cols[v]) >= 3]
    on_row = {}
    for i, rs in enumerate(kept):
        for r in rs[:CHAIN_EDGES]:
            on_row.setdefault(r, []).append(i)
    free = [sum(len(on_row[r]) - 1 for r in rs[:CHAIN_EDGES]) for rs in kept]
    heap = [(free[i], i) for i in range(len(kept))]
    heapq.heapify(heap)
    placed, seq, link = [False] * len(kept), [], []

    def place(i, via):
        placed[i] = True
        seq.append(i)
        link.append(via)
        for r in kept[i][:CHAIN_EDGES]:
            for c in on_row[r]:
                if not placed[c]:
                    free[c] -= 1
                    heapq.heappush(heap, (free[c], c))

    while len(seq) < len(kept):
        while True:
            f, i = heapq.heappop(heap)
            if not placed[i] and f == free[i]:
                break
        place(i, None)
        cur = i
        while True:
            best = None
            for r in kept[cur][:CHAIN_EDGES]:
                for c in on_row[r]:
                    if not placed[c] and (best is None or (free[c], c) < (free[best[0]], best[0])):
                        best = (c, r)
            if best is None:
                break
            place(*best)
            cur = best[0]
    # the runs: run block * WIDTH + w takes the next entries of the walk, position (t, w) at block * WIDTH * length + t * WIDTH + w
    per_block, n_keep = WIDTH * length, len(kept)
    order, from_row = [None] * n_keep, [None] * n_keep
    k = 0
    for base in range(0, n_keep, per_block):
        room = min(per_block, n_keep - base)
        for w in range(min(WIDTH, room)):
            for s in range(-(-(room - w) // WIDTH)):
                order[base + s * WIDTH + w] = seq[k]
                if s > 0 and link[k] is not None:
                    from_row[base + s * WIDTH + w] = link[k]
                k += 1
    assert sorted(order) == list(range(n_keep))
    fetches = carried = issued = 0
    positions = []
    for i0 in range(0, n_keep, WIDTH):
        loads = set()
        for at in range(i0, min(n_keep, i0 + WIDTH)):
            rs = kept[order[at]]
            fetches += len(rs)
            loads |= {r for r in rs if r != from_row[at]}
            if from_row[at] is not None:
                carried += 1
                positions.append((rs.index(from_row[at]), len(rs)))
        issued += len(loads)
    return fetches, carried, issued, tuple(positions)


def mates(rule, vec, group):
    """waves of a 256-thread workgroup that walk a block together: its four waves over the slices of a tile (at most 256
    codewords of f32, 128 of f64, a multiple of 64 that divides the call's group; a slice is 64 * vec of them)"""
    tile = 128 if is_f64(rule) else 256
    while group % tile:
        tile -= 64
    slices = max(1, tile // (64 * vec))
    return 4 // slices if 4 % slices == 0 else 1


def decoder(name, rule, flags8, chains, length=8):
    dec = lt.LdpcDecoder(code(name)[2], rule)
    dec.set("latency", 0)              # the batched kernels at every batch size
    dec.set("vn_records", 1)
    dec.set("flags8", flags8)
    dec.set("vn_bundles", 1)
    dec.set("vn_chains", chains)
    dec.set("vn_chain_len", length)
    assert dec.get("row_records") == 3 and dec.get("record_flag_bits") == 16
    return dec


def test_the_carried_edge_is_a_first_a_middle_and_a_last_edge():
    """the premise of the mixed code with chains of 8, from the code's columns alone"""
    fetches, carried, issued, positions = chain_marks("mixed", 8)
    first = [d for p, d in positions if p == 0]
    last = [d for p, d in positions if p == d - 1]
    middle = [d for p, d in positions if 0 < p < d - 1]
    print(f"mixed, chains of 8: {fetches} fetches, {carried} carried ({len(first)} first, {len(middle)} middle, {len(last)} last "
          f"edges), {issued} issued")
    assert first and middle and last
    assert carried + issued <= fetches and carried >= 53 * 7 // 8 - 12   # 53 kept variables, a connected graph: few breaks


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", CODES)
def test_chained_list_is_invisible(oracle, name, rule):
    ref = cases(oracle, name, rule)
    calm, busy = ref["calm"][2], ref["busy"][2]
    inside = calm[(calm >= 1) & (calm < LIMIT)]
    assert len(inside) >= 20 and len(set(inside.tolist())) >= 3 and (calm < 0).sum() >= 1
    assert (busy < 0).all()
    word = np.uint64 if is_f64(rule) else np.uint32
    for flags8 in (1, 0):
        decs = {0: decoder(name, rule, flags8, 0)}
        for length in LENGTHS:
            decs[length] = decoder(name, rule, flags8, 1, length)
        for level, vec, nb in itertools.product(("calm", "busy"), vecs(rule), BATCHES):
            what = (flags8, level, vec, nb)
            llrs, bits, its, post = (x[:nb] for x in ref[level])
            got = {}
            for length, dec in decs.items():
                dec.set("vec", vec)
                got[length] = dec.decode_batch(llrs, LIMIT, want_posterior=True)
                assert dec.get("last_vn_records") == 1, what
                assert dec.get("last_record_flag_bytes") == (1 if flags8 else 2), what
                assert dec.get("last_vn_bundles") == 1, what
                assert dec.get("last_vn_chains") == (1 if length else 0), (length, what)
                saved = dec.get("vn_chain_saved_permille")
                if length:
                    fetches, carried, issued, _ = chain_marks(name, length)
                    spared = fetches - issued if mates(rule, vec, dec.get("last_group")) == WIDTH else carried
                    assert saved == spared * 1000 // fetches, (length, what)
                else:
                    assert saved == 0, what
            for length in decs:
                assert np.array_equal(got[length][1], its), ("iterations", length, what)
                assert np.array_equal(got[length][0], bits), ("bits", length, what)
                assert got[length][2].dtype == post.dtype
                assert np.array_equal(got[length][2], post), ("posterior", length, what)
                assert np.array_equal(got[length][2].view(word), got[0][2].view(word)), ("posterior, against vn_chains = 0", length, what)
    if name == "mixed":
        _, _, _, positions = chain_marks("mixed", 8)
        assert {0 if p == 0 else (2 if p == d - 1 else 1) for p, d in positions} == {0, 1, 2}
