"""GPU: the NR link handle (include/ldpc_toolbox.h, PART 11) against the composition that defines it -- the chain of the
stage handles NrTransportBlock, Encoder, NrRateMatcher, NrQam and LdpcDecoder, which are pinned to their numpy restatements
and to the oracle by their own tests.  Every comparison is bit for bit.  The received symbols come from the restatements and
a seeded noise (tests/nr_link_cases.py), not from the code under test."""
import functools

import numpy as np
import pytest
import torch

import ldpc_toolbox_amd as lt
import nr_link_cases as cases

pytestmark = pytest.mark.gpu

SPEC3 = "nr5g-link:2:8016:18004:4"     # three blocks of n = 14976, K = 2880 with 176 fillers; E = 6000, 6000, 6004 over 16QAM
SPEC1 = "nr5g-link:2:176:600:2"        # one block, n = 1664, QPSK
FILLER, MAX_ITER = 20.0, 30
# the case of the reception tests, chosen on the CPU with the restatements and the oracle (see test_first_reception_...)
BATCH, PAYLOAD_SEED, EBN0, SEED_RV0, SEED_RV2 = 5, 21, 3.2, 1, 101


def bits_of(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Chain:
    """the stage handles of one link spec, driven by hand: what `run_chain` of tests/test_nr_transport_block_gpu.py does,
    through the host entries"""

    def __init__(self, spec):
        self.bg, self.a, self.g, self.qm = cases.parse(spec)
        self.tb = lt.NrTransportBlock(f"nr5g-tb:{self.bg}:{self.a}", device=0)
        alist = lt.code_alist(self.tb.code_spec)
        self.enc = lt.Encoder(alist)
        self.dec = lt.LdpcDecoder(alist, "Minsumf32", device=0)
        self.rm = lt.NrRateMatcher(self.tb.rate_match_spec, device=0)
        self.qam = lt.NrQam(self.qm, device=0)
        self.c, self.k, self.n = self.tb.c, self.tb.k, self.tb.n
        self.e_lo, self.e_hi, self.c_lo = self.tb.block_lengths(self.g, self.qm)

    def transmit(self, payload, rv, c_init):
        batch = payload.shape[0]
        lo = self.c_lo * batch
        cws = self.enc.encode_batch(self.tb.segment(payload))
        packed = np.concatenate([self.rm.match(cws[:lo], self.e_lo, rv, self.qm).reshape(-1), self.rm.match(cws[lo:], self.e_hi, rv, self.qm).reshape(-1)])
        return self.qam.modulate(self.tb.concatenate(packed, self.g, self.qm), c_init, f64=False)

    def soft_rows(self, symbols, sigma, rv, c_init=-1, old=None, scale=None, max_log=False):
        """demap, split and the two recover calls: [C * batch][n]; old: the rows to combine into (left as they are)"""
        batch = symbols.shape[0]
        lo = self.c_lo * batch
        llrs = self.qam.demodulate(symbols, sigma, max_log, c_init) if scale is None else self.qam.demodulate_csi(symbols, scale, max_log, c_init)
        packed = self.tb.split(llrs, self.qm)
        into = (None, None) if old is None else (old[:lo].copy(), old[lo:].copy())
        rows = [self.rm.recover(packed[:lo * self.e_lo].reshape(lo, self.e_lo), rv, self.qm, FILLER, into[0])]
        if lo < self.c * batch:
            rows.append(self.rm.recover(packed[lo * self.e_lo:].reshape(-1, self.e_hi), rv, self.qm, FILLER, into[1]))
        return llrs, np.concatenate(rows)

    def decode(self, soft):
        """(hard decisions [rows][K], iterations [rows]) of soft rows"""
        bits, its, _ = self.dec.decode_batch(soft, MAX_ITER, output_len=self.k)
        return bits, its

    def block_major_to_tb(self, per_row, batch):
        """[C * batch] block-major -> [batch][C]"""
        return np.ascontiguousarray(per_row.reshape(self.c, batch).T)


@functools.lru_cache(maxsize=None)
def chain(spec):
    return Chain(spec)


def new_link(spec, slots):
    link = lt.NrLink(spec, "Minsumf32", slots, device=0)
    link.set_filler_llr(FILLER)
    return link


def rows_of(flags_tb, batch):
    """[batch][C] -> [C * batch] block-major"""
    return np.ascontiguousarray(flags_tb.T).reshape(-1)


@functools.lru_cache(maxsize=None)
def scenario():
    """Three calls on one handle with 8 slots, the transport blocks in slots 2 .. 6 -- a first reception at rv 0, a
    retransmission at rv 2 with combining, the same retransmission again -- and what the chain gives for each.  Computed
    once; the arrays are not written afterwards."""
    ch = chain(SPEC3)
    sigma = cases.sigma_of(SPEC3, EBN0)
    rx0 = cases.received(SPEC3, BATCH, PAYLOAD_SEED, 0, EBN0, SEED_RV0)
    rx2 = cases.received(SPEC3, BATCH, PAYLOAD_SEED, 2, EBN0, SEED_RV2)
    link = new_link(SPEC3, 8)
    out = {"link": link, "sigma": sigma, "rx0": rx0, "rx2": rx2}
    out["first"] = link.receive(rx0, sigma, rv=0, first_slot=2, combine=False, max_iterations=MAX_ITER)
    out["first_counts"] = (link.decoded_rows, link.skipped_rows)
    out["first_state"] = link.slot_state(2, BATCH)
    out["outside_first"] = link.slot_state(0, 2) + link.slot_state(7, 1)
    out["second"] = link.receive(rx2, sigma, rv=2, first_slot=2, combine=True, max_iterations=MAX_ITER)
    out["second_counts"] = (link.decoded_rows, link.skipped_rows)
    out["second_state"] = link.slot_state(2, BATCH)
    out["third"] = link.receive(rx2, sigma, rv=2, first_slot=2, combine=True, max_iterations=MAX_ITER)
    out["third_counts"] = (link.decoded_rows, link.skipped_rows)
    out["third_state"] = link.slot_state(2, BATCH)
    # the chain
    out["llrs0"], soft0 = ch.soft_rows(rx0, sigma, 0)
    bits0, its0 = ch.decode(soft0)
    out["chain_first"] = (soft0, bits0, its0) + ch.tb.desegment(bits0)
    out["llrs2"], combined = ch.soft_rows(rx2, sigma, 2, old=soft0)
    out["chain_combined"] = (combined,) + ch.decode(combined)
    return out


@pytest.mark.parametrize("spec,batch,rv,c_init", [(SPEC3, 3, 0, -1), (SPEC3, 3, 2, 0x1234), (SPEC3, 3, 0, 0x1234), (SPEC3, 3, 2, -1), (SPEC1, 5, 0, -1),
                                                  (SPEC1, 5, 3, 77)])
def test_transmit_equals_the_chain_every_float_bit(spec, batch, rv, c_init):
    payload, _ = cases.codewords(spec, batch, PAYLOAD_SEED)
    link = scenario()["link"] if spec == SPEC3 else new_link(spec, 1)
    got = link.transmit(payload, rv=rv, c_init=c_init)
    want = chain(spec).transmit(payload, rv, c_init)
    assert got.dtype == np.complex64 and got.shape == (batch, link.symbols) == want.shape
    assert np.array_equal(bits_of(got.view(np.float32)), bits_of(want.view(np.float32)))
    assert np.array_equal(bits_of(got.view(np.float32)), bits_of(cases.transmission(spec, batch, PAYLOAD_SEED, rv, c_init).view(np.float32)))
    assert link.transmit(np.zeros((0, link.a), dtype=np.uint8)).shape == (0, link.symbols), "an empty batch"
    if spec != SPEC3:
        link.close()


def test_first_reception_equals_the_chain():
    """2:8016:18004:4, five transport blocks in slots 2 .. 6 of 8, Eb/N0 3.2 dB, noise seed 1: chosen on the CPU with the
    restatements of the demapper, split and recover and the oracle's Minsumf32 at 30 iterations, where 6 of the 15 code
    blocks pass their CRC24B and 9 do not converge, and one transport block of the five passes as a whole.  The band
    asserted is the issue's: at least 3 pass and at least 3 fail."""
    s = scenario()
    payload, tb_ok, cb_ok, its = s["first"]
    soft, done, rows = s["first_state"]
    want_soft, want_bits, want_its, want_payload, want_tb, want_cb = s["chain_first"]
    passed = int(cb_ok.sum())
    print(f"15 code blocks: {passed} pass their CRC, {15 - passed} fail; {int(tb_ok.sum())} of 5 transport blocks pass")
    assert 3 <= passed <= 12, "both kinds occur"
    assert np.array_equal(payload, want_payload) and np.array_equal(tb_ok, want_tb) and np.array_equal(cb_ok, want_cb)
    assert its.dtype == np.int32 and np.array_equal(its, chain(SPEC3).block_major_to_tb(want_its, BATCH))
    assert np.array_equal(bits_of(soft), bits_of(want_soft))
    assert np.array_equal(rows, want_bits) and np.array_equal(done, cb_ok)
    assert s["first_counts"] == (15, 0)
    sent, _ = cases.codewords(SPEC3, BATCH, PAYLOAD_SEED)
    assert np.array_equal(tb_ok == 1, (payload == sent).all(axis=1)), "no false pass in the recorded outcome"
    # the slots outside the range have not been written
    for x in s["outside_first"]:
        assert not x.any()


def test_retransmission_decodes_only_the_blocks_that_have_not_passed():
    """the same slots again at rv 2 with combining (noise seed 101): on the CPU all 9 remaining blocks then decode"""
    s = scenario()
    ch = chain(SPEC3)
    was_done = rows_of(s["first"][2], BATCH) == 1            # block-major, before the call
    soft1, _, rows1 = s["first_state"]
    its1 = rows_of(s["first"][3], BATCH)
    payload, tb_ok, cb_ok, its = s["second"]
    soft2, done2, rows2 = s["second_state"]
    combined, bits, dec_its = s["chain_combined"]
    assert s["second_counts"] == (int((~was_done).sum()), int(was_done.sum())) and 3 <= was_done.sum() <= 12
    # not done: recover with combine = 1 into the row the slot held, then a decode with the full budget
    assert np.array_equal(bits_of(soft2[~was_done]), bits_of(combined[~was_done]))
    assert np.array_equal(rows2[~was_done], bits[~was_done]) and np.array_equal(rows_of(its, BATCH)[~was_done], dec_its[~was_done])
    # done: nothing of the slot has changed
    assert np.array_equal(bits_of(soft2[was_done]), bits_of(soft1[was_done])) and not np.array_equal(bits_of(soft2[was_done]), bits_of(combined[was_done]))
    assert np.array_equal(rows2[was_done], rows1[was_done]) and np.array_equal(rows_of(its, BATCH)[was_done], its1[was_done])
    # the verdicts are those of desegment over the slots' hard decisions as they stand
    want_payload, want_tb, want_cb = ch.tb.desegment(rows2)
    assert np.array_equal(payload, want_payload) and np.array_equal(tb_ok, want_tb) and np.array_equal(cb_ok, want_cb) and np.array_equal(done2, cb_ok)
    assert (cb_ok >= s["first"][2]).all(), "a done block stays done"
    newly = int(cb_ok.sum() - was_done.sum())
    print(f"retransmission: {int((~was_done).sum())} blocks decoded, {newly} of them pass now; {int(tb_ok.sum())} of 5 transport blocks pass")
    assert newly >= 1
    # a third call: the blocks that are done by now are skipped; where all of a call's blocks are done the decoder is not called
    all_done = rows_of(cb_ok, BATCH) == 1
    assert s["third_counts"] == (int((~all_done).sum()), int(all_done.sum()))
    soft3, done3, rows3 = s["third_state"]
    assert np.array_equal(bits_of(soft3[all_done]), bits_of(soft2[all_done])) and np.array_equal(rows3[all_done], rows2[all_done])
    assert np.array_equal(s["third"][3][cb_ok == 1], its[cb_ok == 1])
    whole = np.nonzero(cb_ok.all(axis=1))[0]
    assert len(whole) >= 1, "a transport block whose blocks are all done"
    b = int(whole[0])
    link = s["link"]
    again = link.receive(s["rx2"][b:b + 1], s["sigma"], rv=2, first_slot=2 + b, combine=True, max_iterations=MAX_ITER)
    assert (link.decoded_rows, link.skipped_rows) == (0, ch.c)
    assert np.array_equal(again[0], payload[b:b + 1]) and again[1][0] == 1 and again[2].all() and np.array_equal(again[3], s["third"][3][b:b + 1])
    state = link.slot_state(2 + b, 1)
    assert np.array_equal(bits_of(state[0]), bits_of(soft3[b::BATCH])) and np.array_equal(state[2], rows3[b::BATCH])


def test_slots_are_independent_and_a_first_reception_resets_them():
    s = scenario()
    sigma, rx0 = s["sigma"], s["rx0"]
    soft, done, rows = s["first_state"]
    link = new_link(SPEC3, 8)

    def slice_of(x, frames):
        return x.reshape(3, BATCH, -1)[:, frames].reshape(3 * len(frames), -1)

    a = link.receive(rx0[:2], sigma, first_slot=0, max_iterations=MAX_ITER)
    state_a = link.slot_state(0, 2)
    b = link.receive(rx0[2:], sigma, first_slot=5, max_iterations=MAX_ITER)
    # the two calls give what the one call of five gave, each in its slots, and the second has not touched the first's
    for got, frames in ((a, [0, 1]), (b, [2, 3, 4])):
        for x, want in zip(got, s["first"]):
            assert np.array_equal(x, want[frames])
    for first, count, frames in ((0, 2, [0, 1]), (5, 3, [2, 3, 4])):
        got = link.slot_state(first, count)
        assert np.array_equal(bits_of(got[0]), bits_of(slice_of(soft, frames))) and np.array_equal(got[1], done[frames])
        assert np.array_equal(got[2], slice_of(rows, frames))
    for x, y in zip(state_a, link.slot_state(0, 2)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert not any(x.any() for x in link.slot_state(2, 3)), "slots 2 .. 4 have not been used"
    # refusals: past the last slot, and combining with a slot that holds no reception -- nothing changes
    before = link.slot_state()
    with pytest.raises(ValueError, match="slots"):
        link.receive(rx0[:2], sigma, first_slot=7, max_iterations=MAX_ITER)
    with pytest.raises(ValueError, match="never been received"):
        link.receive(rx0[:2], sigma, rv=2, first_slot=1, combine=True, max_iterations=MAX_ITER)
    with pytest.raises(ValueError, match="never been received"):
        link.receive(rx0[:3], sigma, rv=2, first_slot=2, combine=True, max_iterations=MAX_ITER)
    for x, y in zip(before, link.slot_state()):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # combine = 0 clears the done flags: noise alone into slots 5 .. 7, where blocks were done
    assert done[[2, 3, 4]].any()
    rng = np.random.default_rng(5)
    junk = (rng.standard_normal((3, link.symbols, 2)).astype(np.float32)).view(np.complex64)[..., 0]
    payload, tb_ok, cb_ok, its = link.receive(junk, sigma, first_slot=5, max_iterations=MAX_ITER)
    assert not cb_ok.any() and not tb_ok.any() and (its == -1).all() and (link.decoded_rows, link.skipped_rows) == (9, 0)
    assert not link.slot_state(5, 3)[1].any()
    for x, y in zip(state_a, link.slot_state(0, 2)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    link.close()


def test_passes_that_end_inside_a_transport_block_change_nothing():
    """a transport block is 3 * 14976 = 44928 elements of the fused kernel and the call 224640: 70001 per pass makes four
    passes, none of which ends where a transport block does"""
    s = scenario()
    link = new_link(SPEC3, 8)
    link.set("pass_elements", 70001)
    assert -(-5 * 3 * link.n // 70001) == 4 and all((p * 70001) % (3 * link.n) for p in (1, 2, 3))
    first = link.receive(s["rx0"], s["sigma"], rv=0, first_slot=2, max_iterations=MAX_ITER)
    state1 = link.slot_state(2, BATCH)
    second = link.receive(s["rx2"], s["sigma"], rv=2, first_slot=2, combine=True, max_iterations=MAX_ITER)
    state2 = link.slot_state(2, BATCH)
    for got, want in ((first, s["first"]), (state1, s["first_state"]), (second, s["second"]), (state2, s["second_state"])):
        for x, y in zip(got, want):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert (link.decoded_rows, link.skipped_rows) == s["second_counts"]
    link.close()


def test_a_scale_per_symbol_equals_the_chain_with_the_csi_demapper():
    """three blocks with a scale per symbol, scrambled; and the max-log demapper on the one-block code"""
    s = scenario()
    ch = chain(SPEC3)
    rx = s["rx0"][:2]
    rng = np.random.default_rng(9)
    scale = ((1.0 / s["sigma"] ** 2) * rng.uniform(0.25, 1.75, rx.shape)).astype(np.float32)
    scale[0, :7] = 0.0                                   # erased symbols
    link = new_link(SPEC3, 2)
    payload, tb_ok, cb_ok, its = link.receive(rx, scale=scale, c_init=0x1234, max_iterations=MAX_ITER)
    _, soft = ch.soft_rows(rx, None, 0, c_init=0x1234, scale=scale)
    bits, want_its = ch.decode(soft)
    want = ch.tb.desegment(bits)
    state = link.slot_state()
    assert np.array_equal(bits_of(state[0]), bits_of(soft)) and np.array_equal(state[2], bits)
    assert np.array_equal(payload, want[0]) and np.array_equal(tb_ok, want[1]) and np.array_equal(cb_ok, want[2])
    assert np.array_equal(its, ch.block_major_to_tb(want_its, 2))
    link.close()
    ch1 = chain(SPEC1)
    link = new_link(SPEC1, 5)
    link.set("max_log", 1)
    sigma = cases.sigma_of(SPEC1, 1.5)
    rx = cases.received(SPEC1, 5, PAYLOAD_SEED, 0, 1.5, 6, c_init=77)
    payload, tb_ok, cb_ok, its = link.receive(rx, sigma, c_init=77, max_iterations=MAX_ITER)
    _, soft = ch1.soft_rows(rx, sigma, 0, c_init=77, max_log=True)
    _, exact = ch1.soft_rows(rx, sigma, 0, c_init=77)
    assert not np.array_equal(bits_of(soft), bits_of(exact)), "the two demappers differ on this input"
    bits, want_its = ch1.decode(soft)
    want = ch1.tb.desegment(bits)
    state = link.slot_state()
    assert np.array_equal(bits_of(state[0]), bits_of(soft)) and np.array_equal(state[2], bits) and np.array_equal(its[:, 0], want_its)
    assert np.array_equal(payload, want[0]) and np.array_equal(tb_ok, want[1]) and np.array_equal(cb_ok[:, 0], tb_ok) and np.array_equal(state[1], cb_ok)
    link.close()


def test_device_entries_on_a_stream():
    """the scenario's calls through the _device entries on a caller's stream, every byte buffer one byte into its
    allocation with a sentinel either side (symbols: one (re, im) pair either side; counts: one element)"""
    s = scenario()
    ch = chain(SPEC3)
    link = new_link(SPEC3, 8)
    dev = torch.device("cuda", 0)
    a, c, S = link.a, link.c, link.symbols
    sent, _ = cases.codewords(SPEC3, BATCH, PAYLOAD_SEED)

    def sentinel(count, dtype=torch.uint8, value=0xEE):
        return torch.full((count + 2,), value, dtype=dtype, device=dev)

    def padded(x, dtype, pad):
        return torch.from_numpy(np.concatenate([np.full(pad, 9, dtype=dtype), np.ascontiguousarray(x).view(dtype).reshape(-1)])).to(dev)

    d_sent = padded(sent, np.uint8, 1)
    d_rx0, d_rx2 = padded(s["rx0"], np.float32, 2), padded(s["rx2"], np.float32, 2)
    d_sym = torch.full((2 * (BATCH * S + 2),), -7.5, dtype=torch.float32, device=dev)
    d_payload, d_tb, d_cb = sentinel(BATCH * a), sentinel(BATCH), sentinel(BATCH * c)
    d_its = torch.full((BATCH * c + 2,), -77, dtype=torch.int32, device=dev)
    d_payload2, d_tb2 = sentinel(BATCH * a), sentinel(BATCH)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    st = stream.cuda_stream
    link.transmit_device(d_sent.data_ptr() + 1, d_sym.data_ptr() + 8, BATCH, rv=2, c_init=5, stream=st)
    link.receive_device(d_rx0.data_ptr() + 8, d_payload.data_ptr() + 1, d_tb.data_ptr() + 1, d_cb.data_ptr() + 1, d_its.data_ptr() + 4, BATCH,
                        s["sigma"], rv=0, first_slot=2, combine=False, max_iterations=MAX_ITER, stream=st)
    stream.synchronize()
    sym = d_sym.cpu().numpy()
    assert (sym[:2] == -7.5).all() and (sym[-2:] == -7.5).all()
    assert np.array_equal(bits_of(sym[2:-2]), bits_of(ch.transmit(sent, 2, 5).view(np.float32).reshape(-1)))
    for d_x in (d_payload, d_tb, d_cb):
        x = d_x.cpu().numpy()
        assert x[0] == 0xEE and x[-1] == 0xEE
    its = d_its.cpu().numpy()
    assert its[0] == -77 and its[-1] == -77
    first = (d_payload.cpu().numpy()[1:-1].reshape(BATCH, a), d_tb.cpu().numpy()[1:-1], d_cb.cpu().numpy()[1:-1].reshape(BATCH, c), its[1:-1].reshape(BATCH, c))
    for x, y in zip(first, s["first"]):
        assert np.array_equal(x, y)
    for x, y in zip(link.slot_state(2, BATCH), s["first_state"]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # the retransmission, cb_ok and iterations not wanted
    link.receive_device(d_rx2.data_ptr() + 8, d_payload2.data_ptr() + 1, d_tb2.data_ptr() + 1, 0, 0, BATCH, s["sigma"], rv=2, first_slot=2,
                        combine=True, max_iterations=MAX_ITER, stream=st)
    stream.synchronize()
    assert (link.decoded_rows, link.skipped_rows) == s["second_counts"]
    for d_x, want in ((d_payload2, s["second"][0]), (d_tb2, s["second"][1])):
        x = d_x.cpu().numpy()
        assert x[0] == 0xEE and x[-1] == 0xEE and np.array_equal(x[1:-1], want.reshape(-1))
    for x, y in zip(link.slot_state(2, BATCH), s["second_state"]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # the rate recovery alone, from a caller's own LLRs: slots 0 .. 1, first on the stream and then combined on the handle's own
    d_llrs0 = torch.from_numpy(s["llrs0"]).to(dev)
    d_llrs2 = torch.from_numpy(s["llrs2"]).to(dev)
    torch.cuda.synchronize()
    link.recover_device(d_llrs0.data_ptr(), 2, rv=0, first_slot=0, combine=False, stream=st)
    stream.synchronize()

    def two(x):
        return x.reshape(3, BATCH, -1)[:, :2].reshape(6, -1)

    soft, done, rows = link.slot_state(0, 2)
    assert np.array_equal(bits_of(soft), bits_of(two(s["chain_first"][0]))) and not done.any() and not rows.any()
    link.recover_device(d_llrs2.data_ptr(), 2, rv=2, first_slot=0, combine=True)
    assert np.array_equal(bits_of(link.slot_state(0, 2)[0]), bits_of(two(s["chain_combined"][0])))
    for x, y in zip(link.slot_state(2, BATCH), s["second_state"]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    link.close()
