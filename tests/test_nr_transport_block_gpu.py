"""GPU: batched NR transport block CRC, segmentation and concatenation (include/ldpc_toolbox.h, PART 7) byte for byte
against the numpy restatement of TS 38.212 (tests/nr_transport_block_reference.py): every row of the hand-computed table,
the CRC verdicts on corrupted blocks, the device entries on a stream, and the chain from payload bits through the encoder,
the rate matcher, the channel and the decoder back to a payload with its verdict."""
import functools

import numpy as np
import pytest
import torch

import ldpc_toolbox_amd as lt
import nr_rate_match_reference as rr
import nr_transport_block_reference as tr
import oracle_binding as ob
from ldpc_toolbox_amd import simulation as sim
from test_nr_transport_block_reference import TABLE

pytestmark = pytest.mark.gpu

BYTES = np.array([0, 1, 1, 2, 255], dtype=np.uint8)
NOT_ONE = np.array([0, 2, 255], dtype=np.uint8)
BIG = (1, 1277992)


def bits_of(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def batches_of(bg, a):
    return (1, 2) if (bg, a) == BIG else (1, 3, 67)


def block_major(rows, c, of, batch):
    """the rows of the first `batch` transport blocks out of `of`"""
    return rows.reshape(c, of, -1)[:, :batch].reshape(c * batch, -1)


@functools.lru_cache(maxsize=None)
def reference(bg, a):
    """computed once per configuration, for its largest batch; transport blocks are independent, so a smaller batch is a
    slice.  Returns (config, raw payload bytes, segmented rows); the arrays are read-only."""
    ref = tr.Config(bg, a)
    batch = batches_of(bg, a)[-1]
    raw = np.random.default_rng(100 * a + bg).choice(BYTES, (batch, a))
    rows = ref.segment(raw)
    raw.setflags(write=False)
    rows.setflags(write=False)
    return ref, raw, rows


def dirty(rows, ref, rng):
    """the same bits in other bytes: zeros become 0, 2 or 255, and the filler columns anything -- ones included"""
    out = np.where(rows == 1, np.uint8(1), rng.choice(NOT_ONE, rows.shape))
    out[:, ref.k_prime:] = rng.choice(BYTES, (rows.shape[0], ref.k - ref.k_prime))
    return out


@pytest.mark.parametrize("bg,a", sorted(TABLE))
def test_segment_and_desegment_equal_the_restatement(bg, a):
    ref, raw, rows = reference(bg, a)
    of = raw.shape[0]
    tb = lt.NrTransportBlock(ref.spec, device=0)
    assert (tb.c, tb.k, tb.k_prime, tb.fillers) == (ref.c, ref.k, ref.k_prime, ref.fillers)
    rng = np.random.default_rng(a)
    for batch in batches_of(bg, a):
        want = block_major(rows, ref.c, of, batch)
        got = tb.segment(raw[:batch])
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), batch
        received = dirty(want, ref, rng)
        payload, tb_ok, cb_ok = tb.desegment(received)
        want_payload, want_tb, want_cb = ref.desegment(received)
        assert np.array_equal(payload, want_payload) and np.array_equal(payload, (raw[:batch] == 1).astype(np.uint8)), batch
        assert np.array_equal(tb_ok, want_tb) and np.array_equal(cb_ok, want_cb) and tb_ok.all() and cb_ok.all(), batch
    assert tb.get("device") == 0
    tb.close()


@pytest.mark.parametrize("bg,a", sorted(TABLE))
def test_concatenate_and_split_equal_the_restatement(bg, a):
    ref = tr.Config(bg, a)
    tb = lt.NrTransportBlock(ref.spec, device=0)
    rng = np.random.default_rng(7 * a + bg)
    batches = batches_of(bg, a)
    case = 0
    for rem in sorted({0, 1 % ref.c, ref.c - 1}):
        for q in (1, 2, 6, 8):
            batch = batches[case % len(batches)]
            case += 1
            g = (ref.c * (2 + case % 3) + rem) * q
            e = ref.block_lengths(g, q)
            e_lo, e_hi, c_lo = tb.block_lengths(g, q)
            assert [e_lo] * c_lo + [e_hi] * (ref.c - c_lo) == e and sum(e) == g
            packed = rng.choice(BYTES, batch * g)
            got = tb.concatenate(packed, g, q)
            assert got.dtype == np.uint8 and np.array_equal(got, ref.concatenate(packed, batch, g, q)), (rem, q, batch)
            for dtype in (np.float32, np.float64):
                rx = (rng.standard_normal((batch, g)) * 10.0 ** rng.integers(-3, 5, (batch, g))).astype(dtype)
                rx[rng.random((batch, g)) < 0.05] = -0.0
                rx[0, 0] = np.nan
                sp = tb.split(rx, q)
                assert sp.dtype == dtype and np.array_equal(bits_of(sp), bits_of(ref.split(rx, q))), (rem, q, batch, dtype)
    tb.close()


@pytest.mark.parametrize("bg,a", [(2, 3826), BIG])
def test_concatenate_and_split_at_standard_sizes(bg, a):
    """G = 11704 coded bits at q = 4 (the chain test's size: blocks of thousands of bits, divisors to match), and the G
    below it at which all blocks but the first get the longer length (c_lo = C - 1); two blocks and 152 blocks"""
    ref = tr.Config(bg, a)
    tb = lt.NrTransportBlock(ref.spec, device=0)
    rng = np.random.default_rng(a + bg)
    q, batch, c = 4, 3, ref.c
    g_one = q * ((11704 // q) // c * c + 1)
    for g in (11704, g_one):
        e = ref.block_lengths(g, q)
        e_lo, e_hi, c_lo = tb.block_lengths(g, q)
        assert [e_lo] * c_lo + [e_hi] * (c - c_lo) == e and sum(e) == g and (g != g_one or (c_lo == c - 1 and e_hi == e_lo + q))
        packed = rng.choice(BYTES, batch * g)
        assert np.array_equal(tb.concatenate(packed, g, q), ref.concatenate(packed, batch, g, q)), g
        for dtype in (np.float32, np.float64):
            rx = (rng.standard_normal((batch, g)) * 10.0 ** rng.integers(-3, 5, (batch, g))).astype(dtype)
            rx[rng.random((batch, g)) < 0.05] = -0.0
            rx[0, 0] = np.nan
            sp = tb.split(rx, q)
            assert sp.dtype == dtype and np.array_equal(bits_of(sp), bits_of(ref.split(rx, q))), (g, dtype)
    tb.close()


def expect_flags(tb, ref, rows, cleared_cb, cleared_tb, what):
    """the entry equals the restatement, and the cleared flags are exactly the given ones"""
    payload, tb_ok, cb_ok = tb.desegment(rows)
    want_payload, want_tb, want_cb = ref.desegment(rows)
    assert np.array_equal(payload, want_payload) and np.array_equal(tb_ok, want_tb) and np.array_equal(cb_ok, want_cb), what
    assert sorted(zip(*np.nonzero(cb_ok == 0))) == sorted(cleared_cb), what
    assert sorted(np.nonzero(tb_ok == 0)[0]) == sorted(cleared_tb), what


@pytest.mark.parametrize("bg,a", [(2, 7641), (1, 8426), (2, 176), (1, 3825)])
def test_crc_flags_on_corrupted_blocks(bg, a):
    """(2, 7641): three blocks; (1, 8426): two blocks of 4249 bits, more than one pass of the workgroup over its row;
    (2, 176): one block under CRC16; (1, 3825): one block under CRC24A"""
    ref = tr.Config(bg, a)
    tb = lt.NrTransportBlock(ref.spec, device=0)
    rng = np.random.default_rng(a)
    batch, c = 5, ref.c
    payload = rng.integers(0, 2, (batch, a), dtype=np.uint8)
    clean = tb.segment(payload)
    assert np.array_equal(clean, ref.segment(payload))
    expect_flags(tb, ref, clean, [], [], "clean")
    take = ref.k_prime - ref.l_cb                      # the bits of B a block carries
    # one flipped bit: the ends of a block, and where the kernel's runs meet -- the 32 bits of a lane, the 64 bytes of a
    # ballot, the 256 bytes of a pass of the workgroup
    positions = sorted({0, 31, 32, 63, 64, 255, 256, take // 2, take - 1} & set(range(take)))
    for i, pos in enumerate(positions):
        b, r = i % batch, i % c
        rows = clean.copy()
        rows[r * batch + b, pos] ^= 1
        expect_flags(tb, ref, rows, [(b, r)], [b], ("bit", pos))
    # in the CRC bits themselves: the transport block's (the end of the last block's share of B) clear both flags, a code
    # block's clear that block's flag only -- they are no part of B
    for pos in (take - ref.l_tb, take - 1):
        rows = clean.copy()
        rows[(c - 1) * batch + 2, pos] ^= 1
        expect_flags(tb, ref, rows, [(2, c - 1)], [2], ("tb crc bit", pos))
    if c > 1:
        for r, pos in ((0, take), (c - 1, ref.k_prime - 1)):
            rows = clean.copy()
            rows[r * batch + 1, pos] ^= 1
            expect_flags(tb, ref, rows, [(1, r)], [], ("cb crc bit", pos))
    # a burst no longer than the CRC is always detected: 24 bits, 16 under CRC16
    for i in range(6):
        b, r = int(rng.integers(batch)), int(rng.integers(c))
        length = int(rng.integers(2, ref.l_tb + 1))
        start = int(rng.integers(0, take - length + 1))
        burst = rng.integers(0, 2, length, dtype=np.uint8)
        burst[0] = burst[-1] = 1
        rows = clean.copy()
        rows[r * batch + b, start:start + length] ^= burst
        expect_flags(tb, ref, rows, [(b, r)], [b], ("burst", start, length))
    # the filler columns are not read
    if ref.fillers:
        rows = clean.copy()
        rows[:, ref.k_prime:] = rng.choice(BYTES, (c * batch, ref.fillers))
        expect_flags(tb, ref, rows, [], [], "fillers")
    # a block of another transport block, with its own valid CRC24B: only the CRC across the blocks can tell
    if c > 1:
        for r in (0, c - 1):
            rows = clean.copy()
            rows[r * batch + 3] = clean[r * batch + 4]
            payload_got, tb_ok, cb_ok = tb.desegment(rows)
            expect_flags(tb, ref, rows, [], [3], ("foreign block", r))
    tb.close()


def test_device_entries_on_a_stream():
    """(2, 7641), five transport blocks, every buffer one byte (or one element) into its allocation"""
    ref = tr.Config(2, 7641)
    tb = lt.NrTransportBlock(ref.spec, device=0)
    rng = np.random.default_rng(31)
    batch, c, k, a = 5, ref.c, ref.k, ref.a
    g, q = (3 * 40 + 2) * 6, 6
    dev = torch.device("cuda", 0)
    raw = rng.choice(BYTES, (batch, a))
    received = dirty(ref.segment(raw), ref, rng)
    received[1 * batch + 2, 100] = 0 if received[1 * batch + 2, 100] == 1 else 1
    packed = rng.choice(BYTES, batch * g)
    rx32 = rng.standard_normal((batch, g)).astype(np.float32)
    rx64 = rng.standard_normal((batch, g))

    def sentinel(count, dtype=torch.uint8, value=0xEE):
        return torch.full((count + 2,), value, dtype=dtype, device=dev)

    d_raw, d_received, d_packed = (torch.from_numpy(np.concatenate([[9], x.reshape(-1)]).astype(np.uint8)).to(dev) for x in (raw, received, packed))
    d_rx32, d_rx64 = torch.from_numpy(rx32).to(dev), torch.from_numpy(rx64).to(dev)
    d_rows, d_payload, d_tb, d_cb, d_cat = sentinel(c * batch * k), sentinel(batch * a), sentinel(batch), sentinel(batch * c), sentinel(batch * g)
    d_sp32, d_sp64 = sentinel(batch * g, torch.float32, -7.5), sentinel(batch * g, torch.float64, -7.5)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    st = stream.cuda_stream
    tb.segment_device(d_raw.data_ptr() + 1, d_rows.data_ptr() + 1, batch, stream=st)
    tb.desegment_device(d_received.data_ptr() + 1, d_payload.data_ptr() + 1, d_tb.data_ptr() + 1, d_cb.data_ptr() + 1, batch, stream=st)
    tb.concatenate_device(d_packed.data_ptr() + 1, d_cat.data_ptr() + 1, batch, g, q, stream=st)
    tb.split_device(d_rx32.data_ptr(), d_sp32.data_ptr() + 4, False, batch, g, q, stream=st)
    tb.split_device(d_rx64.data_ptr(), d_sp64.data_ptr() + 8, True, batch, g, q, stream=st)
    stream.synchronize()
    for d_x in (d_rows, d_payload, d_tb, d_cb, d_cat):
        x = d_x.cpu().numpy()
        assert x[0] == 0xEE and x[-1] == 0xEE
    for d_x in (d_sp32, d_sp64):
        x = d_x.cpu().numpy()
        assert x[0] == -7.5 and x[-1] == -7.5
    rows = d_rows.cpu().numpy()[1:-1].reshape(c * batch, k)
    assert np.array_equal(rows, tb.segment(raw)) and np.array_equal(rows, ref.segment(raw))
    payload, tb_ok, cb_ok = tb.desegment(received)
    assert np.array_equal(d_payload.cpu().numpy()[1:-1].reshape(batch, a), payload)
    assert np.array_equal(d_tb.cpu().numpy()[1:-1], tb_ok) and list(tb_ok) == [1, 1, 0, 1, 1]
    assert np.array_equal(d_cb.cpu().numpy()[1:-1].reshape(batch, c), cb_ok) and cb_ok.sum() == batch * c - 1 and cb_ok[2, 1] == 0
    assert np.array_equal(d_cat.cpu().numpy()[1:-1].reshape(batch, g), tb.concatenate(packed, g, q))
    assert np.array_equal(bits_of(d_sp32.cpu().numpy()[1:-1]), bits_of(tb.split(rx32, q)))
    assert np.array_equal(bits_of(d_sp64.cpu().numpy()[1:-1]), bits_of(tb.split(rx64, q)))
    # cb_ok is optional; NULL stream: the handle's own, synchronous
    d_tb2, d_payload2 = sentinel(batch), sentinel(batch * a)
    torch.cuda.synchronize()
    tb.desegment_device(d_received.data_ptr() + 1, d_payload2.data_ptr() + 1, d_tb2.data_ptr() + 1, 0, batch)
    assert np.array_equal(d_tb2.cpu().numpy()[1:-1], tb_ok) and np.array_equal(d_payload2.cpu().numpy(), d_payload.cpu().numpy())
    # an empty batch is no error
    assert tb.segment(np.zeros((0, a), dtype=np.uint8)).shape == (0, k)
    tb.close()


def run_chain(bg, a, frames, g, q, ebn0_db, noise_seed, payload_seed, max_iter=30, filler_llr=20.0):
    """payload -> segment -> encoder -> two match calls -> concatenate -> QPSK -> AWGN -> demapper -> split -> two recover
    calls -> decoder -> desegment, all device entries on one stream.  The same LLRs go to the CPU oracle.  Returns
    (sent payload, received payload, tb_ok, cb_ok, the oracle's payload per the restatement)."""
    assert q == 2
    tb = lt.NrTransportBlock(f"nr5g-tb:{bg}:{a}", device=0)
    ref = tr.Config(bg, a)
    alist = lt.code_alist(tb.code_spec)
    enc = lt.Encoder(alist)
    dec = lt.LdpcDecoder(alist, "Minsumf32", device=0)
    rm = lt.NrRateMatcher(tb.rate_match_spec, device=0)
    d = lt.Demodulator("QPSK", device=0)
    c, k, n = tb.c, tb.k, tb.n
    assert (dec.n, dec.k, rm.n, rm.fillers) == (n, k, n, tb.fillers)
    e_lo, e_hi, c_lo = tb.block_lengths(g, q)
    sent = np.random.default_rng(payload_seed).integers(0, 2, (frames, a), dtype=np.uint8)
    sigma = sim.noise_sigma(a / g, ebn0_db, 2)
    dev = torch.device("cuda", 0)
    u8 = dict(dtype=torch.uint8, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    d_sent = torch.from_numpy(sent).to(dev)
    d_rows, d_cws = torch.zeros((c * frames, k), **u8), torch.zeros((c * frames, n), **u8)
    d_packed, d_tx = torch.zeros(frames * g, **u8), torch.zeros((frames, g), **u8)
    d_sym, d_rx, d_split = torch.zeros((frames, g // 2, 2), **f32), torch.zeros((frames, g), **f32), torch.zeros(frames * g, **f32)
    d_llrs, d_bits = torch.zeros((c * frames, n), **f32), torch.zeros((c * frames, k), **u8)
    d_its = torch.zeros(c * frames, dtype=torch.int32, device=dev)
    d_payload, d_tb, d_cb = torch.zeros((frames, a), **u8), torch.zeros(frames, **u8), torch.zeros((frames, c), **u8)
    lo_rows, hi_rows = c_lo * frames, (c - c_lo) * frames
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    st = stream.cuda_stream
    tb.segment_device(d_sent.data_ptr(), d_rows.data_ptr(), frames, stream=st)
    enc.encode_batch_device(d_rows.data_ptr(), d_cws.data_ptr(), c * frames, st)
    rm.match_device(d_cws.data_ptr(), d_packed.data_ptr(), lo_rows, e_lo, 0, q, stream=st)
    rm.match_device(d_cws.data_ptr() + lo_rows * n, d_packed.data_ptr() + lo_rows * e_lo, hi_rows, e_hi, 0, q, stream=st)
    tb.concatenate_device(d_packed.data_ptr(), d_tx.data_ptr(), frames, g, q, stream=st)
    d.modulate_device(d_tx.data_ptr(), d_sym.data_ptr(), False, frames, g, 0, st)
    d.add_noise_device(d_sym.data_ptr(), False, frames, g // 2, sigma, noise_seed, 1000, st)
    d.demodulate_device(d_sym.data_ptr(), d_rx.data_ptr(), False, frames, g // 2, sigma, 0, False, st)
    tb.split_device(d_rx.data_ptr(), d_split.data_ptr(), False, frames, g, q, stream=st)
    rm.recover_device(d_split.data_ptr(), d_llrs.data_ptr(), False, lo_rows, e_lo, 0, q, filler_llr=filler_llr, stream=st)
    rm.recover_device(d_split.data_ptr() + 4 * lo_rows * e_lo, d_llrs.data_ptr() + 4 * lo_rows * n, False, hi_rows, e_hi, 0, q,
                      filler_llr=filler_llr, stream=st)
    dec.decode_batch_device(d_llrs.data_ptr(), False, c * frames, max_iter, d_bits.data_ptr(), k, d_its.data_ptr(), 0, st)
    tb.desegment_device(d_bits.data_ptr(), d_payload.data_ptr(), d_tb.data_ptr(), d_cb.data_ptr(), frames, stream=st)
    stream.synchronize()
    # the transmit side is the restatements'
    rows = d_rows.cpu().numpy()
    cws = d_cws.cpu().numpy()
    assert np.array_equal(rows, ref.segment(sent)) and np.array_equal(cws[:, :k], rows)
    rmref = rr.Config(bg, ref.zc, ref.fillers)
    e = ref.block_lengths(g, q)
    want_tx = ref.concatenate(ref.pack([rmref.match(cws[r * frames:(r + 1) * frames], e[r], 0, q) for r in range(c)]), frames, g, q)
    assert np.array_equal(d_tx.cpu().numpy(), want_tx)
    blocks = ref.unpack(ref.split(d_rx.cpu().numpy(), q), frames, g, q)
    want_llrs = np.concatenate([rmref.recover(blocks[r], 0, q, filler_llr) for r in range(c)])
    llrs = d_llrs.cpu().numpy()
    assert np.array_equal(bits_of(llrs), bits_of(want_llrs))
    # the GPU's hard decisions are the oracle's
    obits, oits, _ = ob.decode_batch(ob.Graph(alist), "Minsumf32", llrs, max_iter, threads=4, want_posterior=False)
    bits, its = d_bits.cpu().numpy(), d_its.cpu().numpy()
    assert np.array_equal(bits, obits[:, :k]) and np.array_equal(its, oits)
    oracle_payload, want_tb, want_cb = ref.desegment(obits[:, :k])
    payload, tb_ok, cb_ok = d_payload.cpu().numpy(), d_tb.cpu().numpy(), d_cb.cpu().numpy()
    assert np.array_equal(payload, oracle_payload) and np.array_equal(tb_ok, want_tb) and np.array_equal(cb_ok, want_cb)
    for x in (tb, enc, dec, rm, d):
        x.close()
    return sent, payload, tb_ok, cb_ok, oracle_payload


def test_chain_of_two_blocks_where_every_frame_decodes():
    """(2, 3826): two blocks of n = 10816, G = 11702 over QPSK (E = 5850 and 5852, rate about 1/3), Eb/N0 4 dB: the oracle
    decodes all eight transport blocks (it does so from 3 dB on)"""
    sent, payload, tb_ok, cb_ok, oracle_payload = run_chain(2, 3826, 8, 11702, 2, 4.0, 7, 11)
    assert tb_ok.all() and cb_ok.all() and np.array_equal(payload, sent)


def test_chain_of_one_block_tells_the_frames_that_failed():
    """(2, 176): one block, n = 1664, 96 frames, G = 600 over QPSK, Eb/N0 1.5 dB, noise seed 6: chosen on the CPU with the
    oracle and the channel and demapper restatements, where 57 of the 96 frames decode to the message and 39 do not
    converge.  No frame converges to another codeword and none of the 39 passes the CRC16: the recorded outcome holds no
    false pass, so tb_ok equals "the payload is the sent one" for every frame."""
    sent, payload, tb_ok, cb_ok, oracle_payload = run_chain(2, 176, 96, 600, 2, 1.5, 6, 12)
    right = (oracle_payload == sent).all(axis=1)
    print(f"96 frames: {int(right.sum())} decoded to the message, {int(tb_ok.sum())} pass the CRC")
    assert 24 <= right.sum() <= 72, "both kinds occur"
    assert np.array_equal(tb_ok == 1, right) and np.array_equal(cb_ok[:, 0], tb_ok)
