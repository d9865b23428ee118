"""GPU: the 8-bit mode of the NR link handle (include/ldpc_toolbox.h, PART 12) against the composition that defines it -- the
chain of the stage handles' 8-bit entries: NrQam.demap_i8 / demap_csi_i8, a split of the bytes by numpy slicing,
NrRateMatcher.recover_i8, LdpcDecoder.decode_batch on int8 and NrTransportBlock.desegment, which are pinned to their numpy
restatements and to the oracle by their own tests.  Every comparison is byte for byte.  The received symbols come from the
restatements and a seeded noise (tests/nr_link_cases.py), not from the code under test."""
import functools

import numpy as np
import pytest
import torch

import ldpc_toolbox_amd as lt
import nr_link_cases as cases
import nr_qam_reference as nq
import nr_rate_match_reference as rr
import nr_soft_i8_restatement as sr
import nr_transport_block_reference as tr

pytestmark = pytest.mark.gpu

SPEC3 = "nr5g-link:2:8016:18010:2"     # three blocks of n = 14976, K = 2880 with 176 fillers; E = 6002, 6004, 6004 over QPSK
SPEC_REP = "nr5g-link:2:176:4000:2"    # one block, n = 1664, E = 4000: every sent column is carried two or three times
SPEC_NARROW = "nr5g-link:2:12:122:2"   # one block, n = 260 = 52 * 5: rows on a dword only; G = 122, rows of bytes at 2 mod 4
IMPL3 = "Minstarapproxi8"
FILLER, FILLER_BYTE, MAX_ITER = 20.0, 127, 30
# the case of the reception tests, chosen on the CPU with the restatements and the oracle (see test_first_reception_...)
BATCH, PAYLOAD_SEED, EBN0, SEED_RV0, SEED_RV2 = 5, 21, 0.7, 1, 101


class Chain:
    """the stage handles of one link spec, driven by hand through their 8-bit host entries"""

    def __init__(self, spec, implementation):
        self.spec = spec
        self.bg, self.a, self.g, self.qm = cases.parse(spec)
        self.ref = tr.Config(self.bg, self.a)
        self.tb = lt.NrTransportBlock(f"nr5g-tb:{self.bg}:{self.a}", device=0)
        self.dec = lt.LdpcDecoder(lt.code_alist(self.tb.code_spec), implementation, device=0)
        self.rm = lt.NrRateMatcher(self.tb.rate_match_spec, device=0)
        self.qam = lt.NrQam(self.qm, device=0)
        self.c, self.k, self.n = self.tb.c, self.tb.k, self.tb.n
        self.e = self.ref.block_lengths(self.g, self.qm)
        self.starts = [sum(self.e[:r]) for r in range(self.c)]

    def demap(self, symbols, sigma, c_init=-1, scale=None, max_log=False):
        return self.qam.demap_i8(symbols, sigma, max_log, c_init) if scale is None else self.qam.demap_csi_i8(symbols, scale, max_log, c_init)

    def blocks(self, rx):
        """[batch][G] -> per block r the [batch][E_r] bytes at start(r): a copy, as tests/nr_transport_block_reference.py splits"""
        return [np.ascontiguousarray(rx[:, s:s + e]) for s, e in zip(self.starts, self.e)]

    def recover(self, rx, rv, old=None):
        """split and one recover_i8 call per block length: [C * batch][n] int8, block-major; old: the rows to combine into (left
        as they are)"""
        batch = rx.shape[0]
        parts = self.blocks(rx)
        out = np.zeros((self.c * batch, self.n), dtype=np.int8) if old is None else old.copy()
        for e in sorted(set(self.e)):
            rs = [r for r in range(self.c) if self.e[r] == e]
            rows = np.concatenate([np.arange(r * batch, (r + 1) * batch) for r in rs])
            into = None if old is None else np.ascontiguousarray(old[rows])
            out[rows] = self.rm.recover_i8(np.concatenate([parts[r] for r in rs]), rv, self.qm, filler=FILLER_BYTE, into=into)
        return out

    def soft_rows(self, symbols, sigma, rv, c_init=-1, old=None, scale=None, max_log=False):
        llrs = self.demap(symbols, sigma, c_init, scale, max_log)
        assert llrs.dtype == np.int8 and llrs.shape == (symbols.shape[0], self.g)
        return llrs, self.recover(llrs, rv, old)

    def decode(self, soft):
        """(hard decisions [rows][K], iterations [rows]) of int8 soft rows"""
        assert soft.dtype == np.int8
        bits, its, _ = self.dec.decode_batch(np.ascontiguousarray(soft), MAX_ITER, output_len=self.k)
        return bits, its

    def block_major_to_tb(self, per_row, batch):
        """[C * batch] block-major -> [batch][C]"""
        return np.ascontiguousarray(per_row.reshape(self.c, batch).T)

    def reception(self, link, rx, sigma, rv, first_slot, old=None, was_done=None, **kw):
        """one receive call on `link` against the chain: a first reception (old None), or a retransmission combined into the
        rows `old` of which `was_done` (block-major) are done.  Returns the link's results and state and the chain's soft rows."""
        batch = rx.shape[0]
        demap_kw = {k: v for k, v in kw.items() if k in ("c_init", "scale")}
        got = link.receive(rx, sigma, rv=rv, first_slot=first_slot, combine=old is not None, max_iterations=MAX_ITER, **demap_kw)
        counts = (link.decoded_rows, link.skipped_rows)
        state = link.slot_state(first_slot, batch)
        llrs, soft = self.soft_rows(rx, sigma, rv, old=old, max_log=kw.get("max_log", False), **demap_kw)
        return got, counts, state, llrs, soft


@functools.lru_cache(maxsize=None)
def chain(spec, implementation=IMPL3):
    return Chain(spec, implementation)


def new_link(spec, slots, implementation=IMPL3):
    link = lt.NrLink(spec, implementation, slots, device=0, soft_bits=8)
    link.set_filler_llr(FILLER)
    return link


def rows_of(flags_tb):
    """[batch][C] -> [C * batch] block-major"""
    return np.ascontiguousarray(flags_tb.T).reshape(-1)


def noisy(spec, batch, rv, sigma, seed, c_init=-1):
    """the restated transmission plus float32(sigma * normal) per coordinate, sigma given directly"""
    symbols = cases.transmission(spec, batch, PAYLOAD_SEED, rv, c_init)
    noise = (sigma * np.random.default_rng(seed).standard_normal(symbols.shape + (2,))).astype(np.float32)
    out = symbols.copy()
    out.real += noise[..., 0]
    out.imag += noise[..., 1]
    return out


def same_bytes(got, want):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(got, want))


@functools.lru_cache(maxsize=None)
def scenario():
    """Three calls on one 8-bit handle with 8 slots, the transport blocks in slots 2 .. 6 -- a first reception at rv 0, a
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
    out["outside_third"] = link.slot_state(0, 2) + link.slot_state(7, 1)
    # the chain
    out["llrs0"], soft0 = ch.soft_rows(rx0, sigma, 0)
    bits0, its0 = ch.decode(soft0)
    out["chain_first"] = (soft0, bits0, its0) + ch.tb.desegment(bits0)
    out["llrs2"], combined = ch.soft_rows(rx2, sigma, 2, old=soft0)
    out["chain_combined"] = (combined,) + ch.decode(combined)
    return out


def test_the_geometry_of_the_cases():
    """by tests/nr_transport_block_reference.py: received rows and blocks begin at both even byte alignments"""
    ch = chain(SPEC3)
    assert (ch.c, ch.n, ch.k, ch.ref.fillers) == (3, 14976, 2880, 176) and ch.e == [6002, 6004, 6004] and ch.starts == [0, 6002, 12006]
    assert {(b * ch.g + s) % 4 for b in range(BATCH) for s in ch.starts} == {0, 2}
    link = scenario()["link"]
    assert (link.soft_bits, link.soft_bytes, link.block_lengths) == (8, 3 * 8 * 14976, (6002, 6004, 1))
    rep = tr.Config(2, 176)
    assert (rep.c, rep.n) == (1, 1664) and rep.block_lengths(4000, 2) == [4000]
    repeats = rr.Config(2, rep.zc, rep.fillers).repeats(4000, 0)
    assert set(np.unique(repeats[repeats > 0])) == {2, 3}, "every sent column is carried two or three times"
    narrow = tr.Config(2, 12)
    assert (narrow.c, narrow.zc, narrow.n, narrow.n % 16) == (1, 5, 260, 4) and narrow.block_lengths(122, 2) == [122] and 122 % 4 == 2


def test_first_reception_equals_the_chain():
    """2:8016:18010:2, five transport blocks in slots 2 .. 6 of 8, Eb/N0 0.7 dB, noise seed 1: chosen on the CPU with the
    numpy restatements of the 8-bit demapper and recovery and the oracle's Minstarapproxi8 on clip(v) / 8 at 30 iterations,
    where 10 of the 15 code blocks pass their CRC24B and 5 do not converge, one transport block of the five passes as a whole
    and there is no false pass.  The band asserted is the issue's."""
    s = scenario()
    payload, tb_ok, cb_ok, its = s["first"]
    soft, done, rows = s["first_state"]
    want_soft, want_bits, want_its, want_payload, want_tb, want_cb = s["chain_first"]
    passed = int(cb_ok.sum())
    print(f"15 code blocks: {passed} pass their CRC, {15 - passed} fail; {int(tb_ok.sum())} of 5 transport blocks pass")
    assert 3 <= passed <= 12, "both kinds occur"
    assert np.array_equal(payload, want_payload) and np.array_equal(tb_ok, want_tb) and np.array_equal(cb_ok, want_cb)
    assert its.dtype == np.int32 and np.array_equal(its, chain(SPEC3).block_major_to_tb(want_its, BATCH))
    assert soft.dtype == np.int8 and soft.shape == want_soft.shape and np.array_equal(soft, want_soft)
    assert (soft[:, 2880 - 176:2880] == FILLER_BYTE).all() and soft.min() >= -127
    assert np.array_equal(rows, want_bits) and np.array_equal(done, cb_ok)
    assert s["first_counts"] == (15, 0)
    sent, _ = cases.codewords(SPEC3, BATCH, PAYLOAD_SEED)
    assert np.array_equal(tb_ok == 1, (payload == sent).all(axis=1)), "no false pass in the recorded outcome"
    # the slots outside the range have not been written
    for x in s["outside_first"]:
        assert not x.any()


def test_retransmission_decodes_only_the_blocks_that_have_not_passed():
    """the same slots again at rv 2 with combining (noise seed 101): on the CPU all 15 blocks then pass"""
    s = scenario()
    ch = chain(SPEC3)
    was_done = rows_of(s["first"][2]) == 1            # block-major, before the call
    soft1, _, rows1 = s["first_state"]
    its1 = rows_of(s["first"][3])
    payload, tb_ok, cb_ok, its = s["second"]
    soft2, done2, rows2 = s["second_state"]
    combined, bits, dec_its = s["chain_combined"]
    assert s["second_counts"] == (int((~was_done).sum()), int(was_done.sum())) and 3 <= was_done.sum() <= 12
    # not done: recover_i8 with combine = 1 into the row the slot held, then a decode with the full budget
    assert np.array_equal(soft2[~was_done], combined[~was_done])
    assert np.array_equal(rows2[~was_done], bits[~was_done]) and np.array_equal(rows_of(its)[~was_done], dec_its[~was_done])
    # done: nothing of the slot has changed, byte for byte
    assert np.array_equal(soft2[was_done], soft1[was_done]) and not np.array_equal(soft2[was_done], combined[was_done])
    assert np.array_equal(rows2[was_done], rows1[was_done]) and np.array_equal(rows_of(its)[was_done], its1[was_done])
    # the verdicts are those of desegment over the slots' hard decisions as they stand
    want_payload, want_tb, want_cb = ch.tb.desegment(rows2)
    assert np.array_equal(payload, want_payload) and np.array_equal(tb_ok, want_tb) and np.array_equal(cb_ok, want_cb) and np.array_equal(done2, cb_ok)
    assert (cb_ok >= s["first"][2]).all(), "a done block stays done"
    newly = int(cb_ok.sum() - was_done.sum())
    print(f"retransmission: {int((~was_done).sum())} blocks decoded, {newly} of them pass now; {int(tb_ok.sum())} of 5 transport blocks pass")
    assert newly >= 1
    # a third call: the blocks that are done by now are skipped, and nothing of them changes
    all_done = rows_of(cb_ok) == 1
    assert s["third_counts"] == (int((~all_done).sum()), int(all_done.sum()))
    soft3, done3, rows3 = s["third_state"]
    assert np.array_equal(soft3[all_done], soft2[all_done]) and np.array_equal(rows3[all_done], rows2[all_done])
    assert np.array_equal(s["third"][3][cb_ok == 1], its[cb_ok == 1])
    # the recorded outcome: all 15 blocks are done after the retransmission, so the third call decodes nothing and changes nothing
    assert all_done.all()
    assert s["third_counts"] == (0, 15) and same_bytes(s["third"], s["second"]) and same_bytes(s["third_state"], s["second_state"])
    # a call on slots that are all done: (0, C * batch), the decoder is not called, nothing changes
    whole = np.nonzero(cb_ok.all(axis=1))[0]
    assert len(whole) >= 1, "a transport block whose blocks are all done"
    b = int(whole[0])
    link = s["link"]
    again = link.receive(s["rx2"][b:b + 1], s["sigma"], rv=2, first_slot=2 + b, combine=True, max_iterations=MAX_ITER)
    assert (link.decoded_rows, link.skipped_rows) == (0, ch.c)
    assert np.array_equal(again[0], payload[b:b + 1]) and again[1][0] == 1 and again[2].all() and np.array_equal(again[3], s["third"][3][b:b + 1])
    state = link.slot_state(2 + b, 1)
    assert np.array_equal(state[0], soft3[b::BATCH]) and np.array_equal(state[2], rows3[b::BATCH])
    for x in s["outside_third"]:
        assert not x.any(), "slots outside the range read as zeros"


def test_saturating_sums_of_repeats_and_of_the_retransmission():
    """2:176:4000:2, batch 4, sigma 0.5 given directly: no demapper byte is at +-127, and by the restatement 921 of the 6656
    columns saturate while the repeats are summed (14 %) and 4658 once the rv 3 retransmission is combined (70 %) -- the
    order of the sums is exercised"""
    ch = chain(SPEC_REP, "Minsumi8")
    ref = rr.Config(2, ch.ref.zc, ch.ref.fillers)
    sigma, batch = 0.5, 4
    link = new_link(SPEC_REP, batch, "Minsumi8")
    sat = np.zeros((batch, ch.n), dtype=bool)
    rx0, rx3 = noisy(SPEC_REP, batch, 0, sigma, 1), noisy(SPEC_REP, batch, 3, sigma, 2)
    got, counts, state, llrs0, soft0 = ch.reception(link, rx0, sigma, 0, 0)
    assert np.abs(llrs0.astype(np.int32)).max() < 127, "no demapper byte is at +-127"
    assert np.array_equal(soft0, sr.recover_i8(ref, llrs0, 0, 2, FILLER_BYTE, saturated=sat)), "the chain is the restatement"
    print(f"first reception: {int(sat.sum())} of {sat.size} columns saturate")
    assert sat.mean() >= 0.1
    assert state[0].dtype == np.int8 and np.array_equal(state[0], soft0)
    bits0, its0 = ch.decode(soft0)
    assert np.array_equal(state[2], bits0) and np.array_equal(got[3][:, 0], its0) and counts == (batch, 0)
    # the retransmission into the rows as the chain holds them; a block that is done is left alone by both
    was_done = got[2][:, 0] == 1
    got3, counts3, state3, llrs3, combined = ch.reception(link, rx3, sigma, 3, 0, old=soft0)
    assert np.abs(llrs3.astype(np.int32)).max() < 127
    assert np.array_equal(combined, sr.recover_i8(ref, llrs3, 3, 2, FILLER_BYTE, old=soft0, saturated=sat))
    print(f"after the rv 3 retransmission: {int(sat.sum())} of {sat.size} columns have saturated; {int(was_done.sum())} blocks were done")
    assert sat.mean() >= 0.1
    assert np.array_equal(state3[0][~was_done], combined[~was_done]) and np.array_equal(state3[0][was_done], soft0[was_done])
    assert counts3 == (int((~was_done).sum()), int(was_done.sum()))
    link.close()
    # the same two rows of demapper bytes through the recover entry, where nothing is decoded and so no block is done: the
    # fused kernel's saturating combine on every row
    link = new_link(SPEC_REP, batch, "Minsumi8")
    dev = torch.device("cuda", 0)
    for llrs, rv, want in ((llrs0, 0, soft0), (llrs3, 3, combined)):
        d_llrs = torch.from_numpy(llrs).to(dev)
        torch.cuda.synchronize()
        link.recover_i8_device(d_llrs.data_ptr(), batch, rv=rv, combine=rv == 3)
        assert np.array_equal(link.slot_state()[0], want), rv
    link.close()


def all_bytes(rng, shape):
    """int8 values drawn uniformly from all 256 bytes, every one of them present"""
    v = rng.integers(-128, 128, shape).astype(np.int8)
    v.reshape(-1)[:256] = np.arange(-128, 128).astype(np.int8)
    return v


@pytest.mark.parametrize("spec,implementation,batch,slots,first", [(SPEC3, IMPL3, 3, 5, 1), (SPEC_REP, "Minsumi8", 4, 4, 0)])
def test_recover_i8_device_on_a_callers_bytes(spec, implementation, batch, slots, first):
    """[batch][G] bytes of all 256 values one byte into their allocation, sentinels either side: combine 0, then twice
    combine 1; the slots are recover_i8 of the sliced bytes after every call"""
    ch = chain(spec, implementation)
    link = new_link(spec, slots, implementation)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(33)
    want = None
    stream = torch.cuda.Stream(device=dev)
    for call, rv in enumerate((0, 2, 3)):
        rx = all_bytes(rng, (batch, ch.g))
        assert (rx == -128).any()
        d_rx = torch.full((batch * ch.g + 2,), 0x6E, dtype=torch.int8, device=dev)
        d_rx[1:-1] = torch.from_numpy(rx).to(dev).reshape(-1)
        assert d_rx.data_ptr() % 4 == 0
        torch.cuda.synchronize()
        link.recover_i8_device(d_rx.data_ptr() + 1, batch, rv=rv, first_slot=first, combine=call > 0, stream=stream.cuda_stream if call != 1 else 0)
        stream.synchronize()
        want = ch.recover(rx, rv, old=want)
        soft, done, rows = link.slot_state(first, batch)
        assert soft.dtype == np.int8 and np.array_equal(soft, want), (spec, call)
        assert soft.min() >= -127 and not done.any() and not rows.any(), "no verdict and no hard decision changes"
        back = d_rx.cpu().numpy()
        assert back[0] == 0x6E and back[-1] == 0x6E and np.array_equal(back[1:-1].reshape(batch, ch.g), rx), "the caller's buffer is intact"
    assert (link.decoded_rows, link.skipped_rows) == (0, 0)
    for lo, count in ((0, first), (first + batch, slots - first - batch)):
        assert not any(x.any() for x in link.slot_state(lo, count)), "slots outside the range read as zeros"
    link.close()


@pytest.mark.parametrize("pass_elements", [70001, 5])
def test_passes_change_nothing(pass_elements):
    """a transport block is 3 * 14976 = 44928 elements of the fused kernel and the call 224640: 70001 per pass is rounded to
    70000 -- four passes, none of which ends where a transport block does; 5 is rounded to 4, one dword per launch"""
    s = scenario()
    link = new_link(SPEC3, 8)
    link.set("pass_elements", pass_elements)
    assert link.get("pass_elements") == pass_elements, "the key keeps the value it was given"
    assert all((p * 70000) % (3 * link.n) for p in (1, 2, 3))
    first = link.receive(s["rx0"], s["sigma"], rv=0, first_slot=2, max_iterations=MAX_ITER)
    state1 = link.slot_state(2, BATCH)
    second = link.receive(s["rx2"], s["sigma"], rv=2, first_slot=2, combine=True, max_iterations=MAX_ITER)
    state2 = link.slot_state(2, BATCH)
    for got, want in ((first, s["first"]), (state1, s["first_state"]), (second, s["second"]), (state2, s["second_state"])):
        assert same_bytes(got, want)
    assert (link.decoded_rows, link.skipped_rows) == s["second_counts"]
    link.close()


def test_rows_on_a_dword_only():
    """2:12:122:2: n = 260 is no multiple of 16 -- the narrow gather -- and the received rows of 122 bytes begin at 0 and 2
    mod 4; three transport blocks in slots 1 .. 3 of 5, Minsumi8Offset, a first reception and a retransmission"""
    ch = chain(SPEC_NARROW, "Minsumi8Offset")
    link = new_link(SPEC_NARROW, 5, "Minsumi8Offset")
    assert (link.n, link.g, link.soft_bytes) == (260, 122, 5 * 260)
    sigma = 1.1
    rx0, rx2 = noisy(SPEC_NARROW, 3, 0, sigma, 7), noisy(SPEC_NARROW, 3, 2, sigma, 8)
    got, counts, state, _, soft0 = ch.reception(link, rx0, sigma, 0, 1)
    bits0, its0 = ch.decode(soft0)
    want = ch.tb.desegment(bits0)
    assert np.array_equal(state[0], soft0) and np.array_equal(state[2], bits0) and np.array_equal(got[3][:, 0], its0) and counts == (3, 0)
    assert all(np.array_equal(x, y) for x, y in zip(got[:3], want)) and np.array_equal(state[1], got[2])
    was_done = got[2][:, 0] == 1
    got2, counts2, state2, _, combined = ch.reception(link, rx2, sigma, 2, 1, old=soft0)
    bits2, its2 = ch.decode(combined)
    print(f"n = 260: {int(was_done.sum())} of 3 blocks pass at once, {int(got2[2].sum())} after the retransmission")
    assert counts2 == (int((~was_done).sum()), int(was_done.sum()))
    assert np.array_equal(state2[0][~was_done], combined[~was_done]) and np.array_equal(state2[0][was_done], soft0[was_done])
    assert np.array_equal(state2[2][~was_done], bits2[~was_done]) and np.array_equal(state2[2][was_done], bits0[was_done])
    assert np.array_equal(got2[3][:, 0][~was_done], its2[~was_done]) and np.array_equal(got2[3][:, 0][was_done], its0[was_done])
    want2 = ch.tb.desegment(state2[2])
    assert all(np.array_equal(x, y) for x, y in zip(got2[:3], want2))
    assert not any(x.any() for x in link.slot_state(0, 1) + link.slot_state(4, 1))
    link.close()


def test_a_scale_per_symbol_and_the_max_log_demapper():
    """two transport blocks of the scenario with a scale per symbol, scrambled; and the max-log demapper on the one-block
    code at Eb/N0 -7 dB, noise seed 262 -- over QPSK the two demappers differ by rounding alone, and this input was found on
    the CPU with the restatements as one on which a quantised soft bit differs"""
    s = scenario()
    ch = chain(SPEC3)
    rx = s["rx0"][:2]
    rng = np.random.default_rng(9)
    scale = ((1.0 / s["sigma"] ** 2) * rng.uniform(0.25, 1.75, rx.shape)).astype(np.float32)
    scale[0, :7] = 0.0                                   # erased symbols
    link = new_link(SPEC3, 2)
    payload, tb_ok, cb_ok, its = link.receive(rx, scale=scale, c_init=0x1234, max_iterations=MAX_ITER)
    llrs, soft = ch.soft_rows(rx, None, 0, c_init=0x1234, scale=scale)
    assert not llrs[0, :14].any(), "a scale of 0 erases the symbol's soft bits"
    bits, want_its = ch.decode(soft)
    want = ch.tb.desegment(bits)
    state = link.slot_state()
    assert state[0].dtype == np.int8 and np.array_equal(state[0], soft) and np.array_equal(state[2], bits)
    assert np.array_equal(payload, want[0]) and np.array_equal(tb_ok, want[1]) and np.array_equal(cb_ok, want[2])
    assert np.array_equal(its, ch.block_major_to_tb(want_its, 2))
    link.close()
    ch1 = chain(SPEC_REP, "Minsumi8")
    link = new_link(SPEC_REP, 5, "Minsumi8")
    link.set("max_log", 1)
    sigma = cases.sigma_of(SPEC_REP, -7.0)
    rx = cases.received(SPEC_REP, 5, PAYLOAD_SEED, 0, -7.0, 262, c_init=77)
    payload, tb_ok, cb_ok, its = link.receive(rx, sigma, c_init=77, max_iterations=MAX_ITER)
    llrs, soft = ch1.soft_rows(rx, sigma, 0, c_init=77, max_log=True)
    exact, _ = ch1.soft_rows(rx, sigma, 0, c_init=77)
    assert np.array_equal(llrs, sr.quantise(nq.demodulate(rx, sigma, 2, True, 77))) and np.array_equal(exact, sr.quantise(nq.demodulate(rx, sigma, 2, False, 77)))
    assert not np.array_equal(llrs, exact), "the two demappers differ on this input"
    bits, want_its = ch1.decode(soft)
    want = ch1.tb.desegment(bits)
    state = link.slot_state()
    assert np.array_equal(state[0], soft) and np.array_equal(state[2], bits) and np.array_equal(its[:, 0], want_its)
    assert np.array_equal(payload, want[0]) and np.array_equal(tb_ok, want[1]) and np.array_equal(cb_ok[:, 0], tb_ok) and np.array_equal(state[1], cb_ok)
    link.close()


def test_device_entries_on_a_stream():
    """the scenario's two calls through receive_device on a caller's stream, every byte buffer one byte into its allocation
    with a sentinel either side (symbols: one (re, im) pair either side; counts: one element)"""
    s = scenario()
    link = new_link(SPEC3, 8)
    dev = torch.device("cuda", 0)
    a, c = link.a, link.c

    def sentinel(count, dtype=torch.uint8, value=0xEE):
        return torch.full((count + 2,), value, dtype=dtype, device=dev)

    def padded(x):
        return torch.from_numpy(np.concatenate([np.full(2, 9, dtype=np.float32), np.ascontiguousarray(x).view(np.float32).reshape(-1)])).to(dev)

    d_rx0, d_rx2 = padded(s["rx0"]), padded(s["rx2"])
    d_payload, d_tb, d_cb = sentinel(BATCH * a), sentinel(BATCH), sentinel(BATCH * c)
    d_its = torch.full((BATCH * c + 2,), -77, dtype=torch.int32, device=dev)
    d_payload2, d_tb2, d_cb2 = sentinel(BATCH * a), sentinel(BATCH), sentinel(BATCH * c)
    d_its2 = torch.full((BATCH * c + 2,), -77, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    st = stream.cuda_stream
    link.receive_device(d_rx0.data_ptr() + 8, d_payload.data_ptr() + 1, d_tb.data_ptr() + 1, d_cb.data_ptr() + 1, d_its.data_ptr() + 4, BATCH,
                        s["sigma"], rv=0, first_slot=2, combine=False, max_iterations=MAX_ITER, stream=st)
    stream.synchronize()
    assert (link.decoded_rows, link.skipped_rows) == s["first_counts"]
    state1 = link.slot_state(2, BATCH)
    link.receive_device(d_rx2.data_ptr() + 8, d_payload2.data_ptr() + 1, d_tb2.data_ptr() + 1, d_cb2.data_ptr() + 1, d_its2.data_ptr() + 4, BATCH,
                        s["sigma"], rv=2, first_slot=2, combine=True, max_iterations=MAX_ITER, stream=st)
    stream.synchronize()
    assert (link.decoded_rows, link.skipped_rows) == s["second_counts"]
    for bufs, want, state, want_state in (((d_payload, d_tb, d_cb, d_its), s["first"], state1, s["first_state"]),
                                          ((d_payload2, d_tb2, d_cb2, d_its2), s["second"], link.slot_state(2, BATCH), s["second_state"])):
        for d_x, y in zip(bufs, want):
            x = d_x.cpu().numpy()
            guard = -77 if x.dtype == np.int32 else 0xEE
            assert x[0] == guard and x[-1] == guard and np.array_equal(x[1:-1], y.reshape(-1))
        assert same_bytes(state, want_state)
    assert not any(x.any() for x in link.slot_state(0, 2) + link.slot_state(7, 1))
    link.close()


def test_the_float_handle_is_untouched():
    """soft_bits 32 with the same 8-bit implementation: float slots, equal to the float chain bit for bit -- and not the
    dequantised 8-bit rows: the float handle sums and then quantises at the decoder's door, the 8-bit one quantises first"""
    s = scenario()
    ch = chain(SPEC3)
    link = lt.NrLink(SPEC3, IMPL3, 8, device=0)
    link.set_filler_llr(FILLER)
    assert (link.soft_bits, link.soft_bytes) == (32, 4 * 3 * 8 * 14976)
    payload, tb_ok, cb_ok, its = link.receive(s["rx0"], s["sigma"], rv=0, first_slot=2, max_iterations=MAX_ITER)
    with pytest.raises(ValueError, match="slots exist"):
        link.set("soft_bits", 8)
    link.set("soft_bits", 32)
    soft, done, rows = link.slot_state(2, BATCH)
    assert soft.dtype == np.float32
    llrs = ch.qam.demodulate(s["rx0"], s["sigma"], False, -1)
    want_soft = np.concatenate([ch.rm.recover(np.ascontiguousarray(llrs[:, st:st + e]), 0, ch.qm, FILLER) for st, e in zip(ch.starts, ch.e)])
    assert np.array_equal(soft.view(np.uint32), want_soft.view(np.uint32))
    bits, want_its, _ = ch.dec.decode_batch(want_soft, MAX_ITER, output_len=ch.k)
    want = ch.tb.desegment(bits)
    assert np.array_equal(rows, bits) and np.array_equal(its, ch.block_major_to_tb(want_its, BATCH))
    assert np.array_equal(payload, want[0]) and np.array_equal(tb_ok, want[1]) and np.array_equal(cb_ok, want[2]) and np.array_equal(done, cb_ok)
    eight = s["first_state"][0]
    sent = np.ones(ch.n, dtype=bool)
    sent[ch.k - ch.ref.fillers:ch.k] = False
    assert not np.array_equal(soft[:, sent], sr.dequantise(eight)[:, sent]), "the two modes hold different soft rows"
    # the 8-bit handle refuses the change as well once its slots exist
    with pytest.raises(ValueError, match="slots exist"):
        s["link"].set("soft_bits", 32)
    assert s["link"].soft_bits == 8
    link.close()
