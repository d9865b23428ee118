"""GPU: the device entries of the NR rate matcher and the NR transport block handle on calls that need more than one pass
(include/ldpc_toolbox.h, PART 6 and 7), bit for bit against the numpy restatements (tests/nr_rate_match_reference.py,
tests/nr_transport_block_reference.py).  A pass is 2^30 elements or 2^22 code block rows, so the calls are large; they are
tiled from P + a few restated rows (tests/tiled_cases.py), built and compared on the device.  What only a later pass runs:
the pointer offsets b0 * row, the `shift` of the dword-store kernels recomputed per pass, RowArgs::b0 / Packing::b0 inside
block-major addressing, part[r * frames + f] with frames != batch, and the flag offsets tb_ok + b0, cb_ok + b0 * C."""
import numpy as np
import pytest
import torch

import ldpc_toolbox_amd as lt
import nr_rate_match_reference as rr
import nr_transport_block_reference as tr
import tiled_cases as tc
from test_nr_rate_match_gpu import soft_values
from test_nr_transport_block_gpu import dirty
from tiled_cases import BYTES, flip

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# mirrored from device_nr_rm.h / device_nr_tb.h; every test asserts its own against the handle's getter
RM_PASS_ELEMENTS = 1 << 30
TB_PASS_ROWS = 1 << 22
TB_PASS_ELEMENTS = 1 << 30
GUARD = 0xEE


def cut_of(limit, row):
    """the frames of a pass as the entries compute them, and a batch of one pass and a ragged rest of three"""
    cut = max(limit // row, 1)
    assert cut * row <= limit < (cut + 1) * row
    return cut, cut + 3


def run_on_a_stream(fn):
    """fn(stream handle) enqueued on a stream of the test's, after everything torch has queued; then waited for"""
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    fn(stream.cuda_stream)
    stream.synchronize()


def guarded(count, offset_bytes=1):
    """a byte buffer of `count` bytes between two guard bytes; the output pointer one byte into the allocation"""
    buf = torch.full((count + 2,), GUARD, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 4 == 0
    return buf, buf.data_ptr() + offset_bytes


def report_peak(what):
    print(f"{what}: peak device memory {torch.cuda.max_memory_allocated(DEV) / 2 ** 30:.2f} GiB")


@pytest.fixture(autouse=True)
def fresh_device_memory():
    torch.cuda.init()            # (the allocator's statistics exist only once the device is initialised)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(DEV)
    yield
    torch.cuda.empty_cache()


@pytest.mark.parametrize("e,qm,shift_differs", [(6656, 8, False), (6654, 2, True)])
def test_match_device_over_two_passes(e, qm, shift_differs):
    """nr5g:2:2:4:93 (n = 104, fillers and a limited buffer), rv 1; about 1.1 GB out, 17 MB in.  E = 6656, Qm 8: every
    column repeats about 74 times; both passes begin one byte into a dword (a pass of E = 6656 is a multiple of four
    bytes).  E = 6654, Qm 2: an odd number of frames of 2 mod 4 bytes, so the second pass begins three bytes into one and
    `shift` differs between the passes."""
    ref = rr.Config(2, 2, 4, 93)
    rm = lt.NrRateMatcher(ref.spec, device=0)
    assert rm.get("pass_elements") == RM_PASS_ELEMENTS and (rm.n, ref.n) == (104, 104)
    rv = 1
    cut, batch = cut_of(RM_PASS_ELEMENTS, e)
    t = tc.Tiling(batch, [cut])
    assert ref.repeats(e, rv).max() >= 70
    rng = np.random.default_rng(e)
    cws = rng.choice(BYTES, (t.patterns, ref.n))
    want = tc.to_device(ref.match(cws, e, rv, qm), DEV)
    ids = t.device_ids(DEV)
    d_cws = tc.tile(tc.to_device(cws, DEV), ids)
    d_buf, out = guarded(batch * e)
    shifts = [(out + b0 * e) & 3 for b0 in (0, cut)]
    assert shifts[0] == 1 and (shifts[1] != shifts[0]) == shift_differs, shifts
    run_on_a_stream(lambda st: rm.match_device(d_cws.data_ptr(), out, batch, e, rv, qm, stream=st))
    assert int(d_buf[0]) == GUARD and int(d_buf[-1]) == GUARD, "the bytes around the output stay untouched"
    tc.assert_tiled(d_buf[1:-1].view(batch, e), want, ids, "match_device")
    report_peak("match_device")
    del d_buf, d_cws
    rm.close()


def test_recover_device_over_passes_and_combined():
    """f32 on nr5g:2:2:4:93.  E = 104 = n, Qm 2, rv 2 with combine = 0 into a buffer full of a sentinel: two passes, about
    4.3 GB in and out.  Then a second transmission, rv 0, Qm 4, E = 208, with combine = 1 into the same buffer: three
    passes of rows of 208, 8.6 GB in.  Peak about 13 GB."""
    ref = rr.Config(2, 2, 4, 93)
    rm = lt.NrRateMatcher(ref.spec, device=0)
    n = ref.n
    assert rm.get("pass_elements") == RM_PASS_ELEMENTS and n == 104
    (e1, rv1, qm1, fill1), (e2, rv2, qm2, fill2) = (104, 2, 2, np.inf), (208, 0, 4, 9.0)
    cut1, batch = cut_of(RM_PASS_ELEMENTS, max(n, e1))
    cut2 = RM_PASS_ELEMENTS // max(n, e2)
    cuts2 = list(range(cut2, batch, cut2))
    assert len(cuts2) == 2, "the second transmission takes three passes"
    t = tc.Tiling(batch, [cut1] + cuts2)
    rng = np.random.default_rng(104)
    rx1, rx2 = soft_values(rng, (t.patterns, e1), np.float32), soft_values(rng, (t.patterns, e2), np.float32)
    want1 = ref.recover(rx1, rv1, qm1, fill1)
    want2 = ref.recover(rx2, rv2, qm2, fill2, old=want1)
    assert (ref.repeats(e1, rv1) == 0).sum() > ref.fillers and ref.repeats(e1, rv1).max() == 2
    ids = t.device_ids(DEV)
    d_llrs = torch.full((batch, n), -7.5, dtype=torch.float32, device=DEV)
    d_rx = tc.tile(tc.to_device(rx1, DEV), ids)
    run_on_a_stream(lambda st: rm.recover_device(d_rx.data_ptr(), d_llrs.data_ptr(), False, batch, e1, rv1, qm1, filler_llr=fill1, stream=st))
    tc.assert_tiled(d_llrs, tc.to_device(want1, DEV), ids, "recover_device, combine = 0")
    del d_rx
    d_rx = tc.tile(tc.to_device(rx2, DEV), ids)
    run_on_a_stream(lambda st: rm.recover_device(d_rx.data_ptr(), d_llrs.data_ptr(), False, batch, e2, rv2, qm2, filler_llr=fill2,
                                                 combine=True, stream=st))
    tc.assert_tiled(d_llrs, tc.to_device(want2, DEV), ids, "recover_device, combine = 1")
    report_peak("recover_device")
    del d_rx, d_llrs
    rm.close()


def expect_cleared(d_tb, d_cb, c, tbs, cbs):
    """the flags that are not 1 are exactly the given ones, and they are 0"""
    tb_off = (d_tb != 1).nonzero().reshape(-1).tolist()
    cb_off = [(i // c, i % c) for i in (d_cb.reshape(-1) != 1).nonzero().reshape(-1).tolist()]
    assert tb_off == sorted(tbs) and cb_off == sorted(cbs), (tb_off, cb_off)
    assert all(int(d_tb[b]) == 0 for b in tbs) and all(int(d_cb.reshape(-1, c)[b, r]) == 0 for b, r in cbs)


def test_one_block_segment_and_desegment_over_two_passes():
    """nr5g-tb:2:1: C = 1, K = 30, CRC16; 2^22 + 3 transport blocks, about 130 MB of rows.  A payload of one bit has two
    patterns only, so the special rows cannot be unique here; the 61 random patterns still differ from row to row.  One
    flipped bit in each of the rows pass - 1, pass and pass + 2 clears tb_ok and cb_ok there (finish_kernel's l_cb == 0
    path) and nowhere else."""
    ref = tr.Config(2, 1)
    tb = lt.NrTransportBlock(ref.spec, device=0)
    assert tb.get("pass_rows") == TB_PASS_ROWS and (ref.c, ref.k, ref.l_tb, tb.c, tb.k) == (1, 30, 16, 1, 30)
    cut, batch = cut_of(TB_PASS_ROWS, ref.c)
    t = tc.Tiling(batch, [cut])
    rng = np.random.default_rng(30)
    raw = rng.choice(BYTES, (t.patterns, ref.a))
    rows = ref.segment(raw)
    assert 0 < rows[:tc.P, 0].sum() < tc.P, "both payloads occur among the tiled patterns"
    ids = t.device_ids(DEV)
    d_raw = tc.tile(tc.to_device(raw, DEV), ids)
    d_rows = torch.full((batch, ref.k), GUARD, dtype=torch.uint8, device=DEV)
    run_on_a_stream(lambda st: tb.segment_device(d_raw.data_ptr(), d_rows.data_ptr(), batch, stream=st))
    tc.assert_tiled(d_rows, tc.to_device(rows, DEV), ids, "segment_device")
    received = dirty(rows, ref, rng)
    bad = [cut - 1, cut, cut + 2]
    assert bad[-1] == batch - 1
    for b, pos in zip(bad, (0, 5, 16)):
        flip(received, t.pattern_of(b), pos)
    want_payload, want_tb, want_cb = ref.desegment(received)
    assert [i for i in range(t.patterns) if not want_tb[i]] == [t.pattern_of(b) for b in bad]
    tc.tile_into(d_rows, tc.to_device(received, DEV), ids)
    d_payload, d_tb, d_cb = (torch.full(shape, GUARD, dtype=torch.uint8, device=DEV) for shape in ((batch, ref.a), (batch,), (batch, 1)))
    run_on_a_stream(lambda st: tb.desegment_device(d_rows.data_ptr(), d_payload.data_ptr(), d_tb.data_ptr(), d_cb.data_ptr(), batch, stream=st))
    tc.assert_tiled(d_payload, tc.to_device(want_payload, DEV), ids, "desegment_device: payload")
    tc.assert_tiled(d_tb.view(batch, 1), tc.to_device(want_tb.reshape(-1, 1), DEV), ids, "desegment_device: tb_ok")
    tc.assert_tiled(d_cb, tc.to_device(want_cb, DEV), ids, "desegment_device: cb_ok")
    expect_cleared(d_tb, d_cb, 1, bad, [(b, 0) for b in bad])
    report_peak("one block")
    tb.close()


def two_block_case():
    """(2, 3826): C = 2, K = 2080, the smallest two-block configuration, over one pass and three transport blocks"""
    cut, batch = cut_of(TB_PASS_ROWS, 2)
    t = tc.Tiling(batch, [cut])
    ref, raw, rows = tc.two_block_patterns(t.patterns)
    return ref, t, raw, rows


def blocks_of(x, c):
    """[C * batch][K] block-major -> [C][batch][K]"""
    return x.view(c, x.shape[0] // c, x.shape[1])


def test_two_block_segment_over_two_passes():
    """2^21 + 3 transport blocks of two blocks: about 8.7 GB of rows and 8.0 GB of payload on the device, 17 GB at the
    peak; freed at the end.  Block-major addressing with b0 > 0 differs from pass 0 only when C > 1."""
    ref, t, raw, rows = two_block_case()
    tb = lt.NrTransportBlock(ref.spec, device=0)
    assert tb.get("pass_rows") == TB_PASS_ROWS and (tb.c, tb.k) == (2, 2080)
    batch, c = t.batch, ref.c
    ids = t.device_ids(DEV)
    d_raw = tc.tile(tc.to_device(raw, DEV), ids)
    d_rows = torch.full((c * batch, ref.k), GUARD, dtype=torch.uint8, device=DEV)
    run_on_a_stream(lambda st: tb.segment_device(d_raw.data_ptr(), d_rows.data_ptr(), batch, stream=st))
    want = blocks_of(tc.to_device(rows, DEV), c)
    for r in range(c):
        tc.assert_tiled(blocks_of(d_rows, c)[r], want[r], ids, f"segment_device: block {r}")
    report_peak("two blocks, segment")
    del d_raw, d_rows
    tb.close()


def test_two_block_desegment_over_two_passes():
    """the same sizes.  Flipped: a payload bit in block 0 of transport block pass - 1, one in block 1 of transport block
    pass, and a CRC24B bit of block 0 of the last: tb_ok is cleared for the first two, cb_ok for these three blocks."""
    ref, t, raw, rows = two_block_case()
    tb = lt.NrTransportBlock(ref.spec, device=0)
    assert tb.get("pass_rows") == TB_PASS_ROWS
    batch, c, cut, pats = t.batch, ref.c, t.boundaries[0], t.patterns
    take = ref.k_prime - ref.l_cb
    received = dirty(rows, ref, np.random.default_rng(2080))
    flip(received, 0 * pats + t.pattern_of(cut - 1), 700)
    flip(received, 1 * pats + t.pattern_of(cut), 1900)
    flip(received, 0 * pats + t.pattern_of(batch - 1), take + 3)
    want_payload, want_tb, want_cb = ref.desegment(received)
    assert want_tb.sum() == pats - 2 and want_cb.sum() == c * pats - 3
    ids = t.device_ids(DEV)
    d_rows = torch.empty((c * batch, ref.k), dtype=torch.uint8, device=DEV)
    d_received = blocks_of(tc.to_device(received, DEV), c)
    for r in range(c):
        tc.tile_into(blocks_of(d_rows, c)[r], d_received[r], ids)
    d_payload, d_tb, d_cb = (torch.full(shape, GUARD, dtype=torch.uint8, device=DEV) for shape in ((batch, ref.a), (batch,), (batch, c)))
    run_on_a_stream(lambda st: tb.desegment_device(d_rows.data_ptr(), d_payload.data_ptr(), d_tb.data_ptr(), d_cb.data_ptr(), batch, stream=st))
    tc.assert_tiled(d_payload, tc.to_device(want_payload, DEV), ids, "desegment_device: payload")
    tc.assert_tiled(d_tb.view(batch, 1), tc.to_device(want_tb.reshape(-1, 1), DEV), ids, "desegment_device: tb_ok")
    tc.assert_tiled(d_cb, tc.to_device(want_cb, DEV), ids, "desegment_device: cb_ok")
    expect_cleared(d_tb, d_cb, c, [cut - 1, cut], [(cut - 1, 0), (cut, 1), (batch - 1, 0)])
    report_peak("two blocks, desegment")
    del d_rows, d_payload, d_tb, d_cb
    tb.close()


@pytest.mark.parametrize("g,lengths,shift_differs", [(14, [6, 8], False), (18, [8, 10], True)])
def test_concatenate_device_over_two_passes(g, lengths, shift_differs):
    """the C = 2 handle, q = 2, both block lengths (c_lo = 1); about 1.1 GB per array.  G = 14: both passes begin one byte
    into a dword (an even number of transport blocks of 14 bytes).  G = 18: an odd number of 18 bytes, the second pass
    begins three bytes into one and `shift` differs between the passes."""
    ref = tr.Config(2, 3826)
    tb = lt.NrTransportBlock(ref.spec, device=0)
    q = 2
    assert tb.get("pass_elements") == TB_PASS_ELEMENTS and ref.block_lengths(g, q) == lengths and tb.block_lengths(g, q) == (lengths[0], lengths[1], 1)
    cut, batch = cut_of(TB_PASS_ELEMENTS, g)
    t = tc.Tiling(batch, [cut])
    packed = np.random.default_rng(g).choice(BYTES, t.patterns * g)
    want = tc.to_device(ref.concatenate(packed, t.patterns, g, q), DEV)
    ids = t.device_ids(DEV)
    d_packed = torch.empty(batch * g, dtype=torch.uint8, device=DEV)
    for view, block in zip(tc.packed_views(d_packed, lengths, batch), ref.unpack(packed, t.patterns, g, q)):
        tc.tile_into(view, tc.to_device(block, DEV), ids)
    d_buf, out = guarded(batch * g)
    shifts = [(out + b0 * g) & 3 for b0 in (0, cut)]
    assert shifts[0] == 1 and (shifts[1] != shifts[0]) == shift_differs, shifts
    run_on_a_stream(lambda st: tb.concatenate_device(d_packed.data_ptr(), out, batch, g, q, stream=st))
    assert int(d_buf[0]) == GUARD and int(d_buf[-1]) == GUARD, "the bytes around the output stay untouched"
    tc.assert_tiled(d_buf[1:-1].view(batch, g), want, ids, "concatenate_device")
    report_peak("concatenate_device")
    del d_buf, d_packed
    tb.close()


def test_split_device_over_two_passes():
    """f32, G = 14, q = 2 on the C = 2 handle: about 4.3 GB in and out"""
    ref = tr.Config(2, 3826)
    tb = lt.NrTransportBlock(ref.spec, device=0)
    g, q, lengths = 14, 2, [6, 8]
    assert tb.get("pass_elements") == TB_PASS_ELEMENTS and ref.block_lengths(g, q) == lengths
    cut, batch = cut_of(TB_PASS_ELEMENTS, g)
    t = tc.Tiling(batch, [cut])
    rng = np.random.default_rng(14)
    rx = soft_values(rng, (t.patterns, g), np.float32)
    rx[0, 0] = np.nan
    want = ref.unpack(ref.split(rx, q), t.patterns, g, q)
    ids = t.device_ids(DEV)
    d_rx = tc.tile(tc.to_device(rx, DEV), ids)
    d_packed = torch.full((batch * g,), -7.5, dtype=torch.float32, device=DEV)
    run_on_a_stream(lambda st: tb.split_device(d_rx.data_ptr(), d_packed.data_ptr(), False, batch, g, q, stream=st))
    for r, view in enumerate(tc.packed_views(d_packed, lengths, batch)):
        tc.assert_tiled(view, tc.to_device(want[r], DEV), ids, f"split_device: block {r}")
    report_peak("split_device")
    del d_rx, d_packed
    tb.close()
