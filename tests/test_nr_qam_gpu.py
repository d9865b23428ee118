"""GPU: the NR modulation mapper, soft demapper and scrambling (ldpc_toolbox_nr_qam_*) against the numpy restatement
(tests/nr_qam_reference.py), bit for bit.  Equality is demod_restatement.same_bits: NaN where the reference has NaN, else
the same bits.  Shape 3 x 173 symbols: 519 threads, two full blocks and a partial one; 173 symbols of QM = 6 put windows
of the scrambling sequence across word boundaries (symbol 5: bits 30..35)."""
import numpy as np
import pytest
import torch

import channel_restatement as cr
import demod_restatement as dr
import ldpc_toolbox_amd as lt
import nr_qam_reference as nq

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
B, S = 3, 173
C_INIT = 0x2A5A5A5
RUN = 1024              # bits of the sequence per thread of the Gold kernel (kGoldRunWords * 32)
_GOLD = {}


def gold(c_init, length):
    """the serial LFSR once per c_init, at the longest length any test asks for"""
    if c_init not in _GOLD:
        _GOLD[c_init] = nq.gold(c_init, 70001)
    return _GOLD[c_init][:length]


@pytest.fixture(scope="module")
def qams():
    q = {qm: lt.NrQam(qm, device=0) for qm in (2, 4, 6, 8)}
    yield q
    for x in q.values():
        x.close()


def make_bits(qm, rng, batch=B, symbols=S):
    """0/1 bytes with a sprinkling of other values (zeros, by the encoder's convention)"""
    bits = rng.integers(0, 2, (batch, qm * symbols)).astype(np.uint8)
    other = rng.random(bits.shape) < 0.1
    bits[other] = rng.integers(2, 256, int(other.sum())).astype(np.uint8)
    return bits


@pytest.mark.parametrize("c_init", [0, 1, (1 << 31) - 1, C_INIT])
def test_sequence_equals_the_serial_lfsr(qams, c_init):
    q = qams[4]
    for length in (1, 31, 32, 33, RUN - 1, RUN, RUN + 1, 70001):
        before = q.get("sequence_launches")
        got = q.sequence(length, c_init)
        assert got.dtype == np.uint8 and np.array_equal(got, gold(c_init, length)), (c_init, length)
        assert q.get("sequence_launches") == before + 1
        again = q.sequence(length, c_init)
        assert q.get("sequence_launches") == before + 1, "the second call with the same key hits the cache"
        assert np.array_equal(again, got)


@pytest.mark.parametrize("qm", [2, 4, 6, 8])
def test_mapper_equals_the_restatement(qams, qm):
    q = qams[qm]
    rng = np.random.default_rng(qm)
    bits = make_bits(qm, rng)
    assert (bits > 1).any()
    for f64, real in ((True, np.float64), (False, np.float32)):
        for c_init in (-1, C_INIT):
            want = nq.modulate(bits, qm, c_init, real)
            got = q.modulate(bits, c_init, f64)
            assert got.dtype == want.dtype and dr.same_bits(got.view(real), want.view(real)), (qm, f64, c_init)
            one = q.modulate(bits[:, :qm], c_init, f64)        # symbols_len = 1
            assert dr.same_bits(one.view(real), nq.modulate(bits[:, :qm], qm, c_init, real).view(real))
            # the device entry on a stream of the caller's
            d_bits = torch.from_numpy(bits).to(DEV)
            d_sym = torch.zeros((B, 2 * S), dtype=torch.float64 if f64 else torch.float32, device=DEV)
            stream = torch.cuda.Stream(device=DEV)
            torch.cuda.synchronize()
            q.modulate_device(d_bits.data_ptr(), d_sym.data_ptr(), f64, B, qm * S, c_init, stream.cuda_stream)
            stream.synchronize()
            assert dr.same_bits(d_sym.cpu().numpy(), want.view(real))
    if qm == 2:
        qpsk = lt.Demodulator("QPSK", device=0)
        for f64 in (True, False):
            a, b = q.modulate(bits, -1, f64), qpsk.modulate(bits, 0, f64)
            assert dr.same_bits(a.view(a.real.dtype), b.view(b.real.dtype)), "QM = 2 without scrambling is the library's QPSK"
        qpsk.close()
    assert q.device == 0


_NOISY = {}


def noisy_symbols(q, qm):
    """the mapper's symbols plus restated noise at a sigma where LLRs of both signs occur; row 2 starts with the specials"""
    if qm not in _NOISY:
        rng = np.random.default_rng(10 + qm)
        bits = make_bits(qm, rng)
        sigma = 0.3
        sym = cr.awgn(q.modulate(bits, C_INIT, True), sigma, 77, 5)
        sym[2, :len(dr.SPECIALS)] = dr.SPECIALS
        _NOISY[qm] = (sym, sigma)
    return _NOISY[qm]


def demod_device(q, sym, f64, sigma, max_log, c_init):
    real = np.float64 if f64 else np.float32
    d_sym = torch.from_numpy(np.ascontiguousarray(sym).view(real)).to(DEV)
    d_out = torch.full((sym.shape[0], q.bits_per_symbol * sym.shape[1]), 12345.0, dtype=torch.float64 if f64 else torch.float32, device=DEV)
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    q.demodulate_device(d_sym.data_ptr(), d_out.data_ptr(), f64, sym.shape[0], sym.shape[1], sigma, max_log, c_init, stream.cuda_stream)
    stream.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("max_log", [False, True])
@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("qm", [2, 4, 6, 8])
def test_demapper_equals_the_restatement(qams, qm, f64, max_log):
    q = qams[qm]
    sym64, sigma = noisy_symbols(q, qm)
    with np.errstate(over="ignore"):            # (the special 1e300 becomes inf in float)
        sym = sym64 if f64 else sym64.astype(np.complex64)
    for c_init in (-1, C_INIT):
        want = nq.demodulate(sym, sigma, qm, max_log, c_init)
        finite = want[np.isfinite(want)]
        assert (finite > 0).any() and (finite < 0).any() and np.isnan(want).any()
        got = q.demodulate(sym, sigma, max_log, c_init)
        assert dr.same_bits(got, want), (qm, f64, max_log, c_init, "host entry")
        assert dr.same_bits(demod_device(q, sym, f64, sigma, max_log, c_init), want), (qm, f64, max_log, c_init, "device entry")


def test_transport_block_chain_over_scrambled_16qam_on_one_stream(qams):
    """INTEGRATION.md's chain: payload -> segment -> encoder -> match -> concatenate -> scrambled 16QAM -> AWGN -> demapper
    with descrambling -> split -> recover -> decoder -> desegment, every step a device entry on one stream of the
    caller's.  (2, 3826): two blocks of n = 10816, G = 11704 (rate about 1/3) at Eb/N0 7 dB: every transport block
    decodes.  The symbols and the LLRs on the way are the restatement's."""
    from ldpc_toolbox_amd import simulation as sim
    bg, a, frames, g, q, c_init = 2, 3826, 8, 11704, 4, 0x12345
    tb = lt.NrTransportBlock(f"nr5g-tb:{bg}:{a}", device=0)
    alist = lt.code_alist(tb.code_spec)
    enc, dec = lt.Encoder(alist), lt.LdpcDecoder(alist, "Minsumf32", device=0)
    rm = lt.NrRateMatcher(tb.rate_match_spec, device=0)
    awgn = lt.Demodulator("QPSK", device=0)      # (the channel reads nothing of the handle's table)
    qam = qams[q]
    c, k, n = tb.c, tb.k, tb.n
    e_lo, e_hi, c_lo = tb.block_lengths(g, q)
    sent = np.random.default_rng(3).integers(0, 2, (frames, a), dtype=np.uint8)
    sigma = sim.noise_sigma(a / g, 7.0, q)
    u8, f32 = dict(dtype=torch.uint8, device=DEV), dict(dtype=torch.float32, device=DEV)
    d_sent = torch.from_numpy(sent).to(DEV)
    d_rows, d_cws = torch.zeros((c * frames, k), **u8), torch.zeros((c * frames, n), **u8)
    d_packed, d_tx = torch.zeros(frames * g, **u8), torch.zeros((frames, g), **u8)
    d_sym, d_clean = torch.zeros((frames, g // q, 2), **f32), torch.zeros((frames, g // q, 2), **f32)
    d_rx, d_split = torch.zeros((frames, g), **f32), torch.zeros(frames * g, **f32)
    d_llrs, d_bits = torch.zeros((c * frames, n), **f32), torch.zeros((c * frames, k), **u8)
    d_its = torch.zeros(c * frames, dtype=torch.int32, device=DEV)
    d_payload, d_tb = torch.zeros((frames, a), **u8), torch.zeros(frames, **u8)
    lo_rows, hi_rows = c_lo * frames, (c - c_lo) * frames
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    st = stream.cuda_stream
    tb.segment_device(d_sent.data_ptr(), d_rows.data_ptr(), frames, stream=st)
    enc.encode_batch_device(d_rows.data_ptr(), d_cws.data_ptr(), c * frames, st)
    rm.match_device(d_cws.data_ptr(), d_packed.data_ptr(), lo_rows, e_lo, 0, q, stream=st)
    rm.match_device(d_cws.data_ptr() + lo_rows * n, d_packed.data_ptr() + lo_rows * e_lo, hi_rows, e_hi, 0, q, stream=st)
    tb.concatenate_device(d_packed.data_ptr(), d_tx.data_ptr(), frames, g, q, stream=st)
    qam.modulate_device(d_tx.data_ptr(), d_sym.data_ptr(), False, frames, g, c_init, st)
    with torch.cuda.stream(stream):
        d_clean.copy_(d_sym)
    awgn.add_noise_device(d_sym.data_ptr(), False, frames, g // q, sigma, 9, 1000, st)
    qam.demodulate_device(d_sym.data_ptr(), d_rx.data_ptr(), False, frames, g // q, sigma, False, c_init, st)
    tb.split_device(d_rx.data_ptr(), d_split.data_ptr(), False, frames, g, q, stream=st)
    rm.recover_device(d_split.data_ptr(), d_llrs.data_ptr(), False, lo_rows, e_lo, 0, q, filler_llr=20.0, stream=st)
    rm.recover_device(d_split.data_ptr() + 4 * lo_rows * e_lo, d_llrs.data_ptr() + 4 * lo_rows * n, False, hi_rows, e_hi, 0, q,
                      filler_llr=20.0, stream=st)
    dec.decode_batch_device(d_llrs.data_ptr(), False, c * frames, 30, d_bits.data_ptr(), k, d_its.data_ptr(), 0, st)
    tb.desegment_device(d_bits.data_ptr(), d_payload.data_ptr(), d_tb.data_ptr(), 0, frames, stream=st)
    stream.synchronize()
    tx = d_tx.cpu().numpy()
    clean = nq.modulate(tx, q, c_init, np.float32)
    assert dr.same_bits(d_clean.cpu().numpy().reshape(frames, -1), clean.view(np.float32))
    noisy = d_sym.cpu().numpy().reshape(frames, -1).view(np.complex64)
    assert dr.same_bits(noisy.view(np.float32), cr.awgn(clean, sigma, 9, 1000).view(np.float32))
    assert dr.same_bits(d_rx.cpu().numpy(), nq.demodulate(noisy, sigma, q, False, c_init))
    assert (d_its.cpu().numpy() >= 0).all() and d_tb.cpu().numpy().all() and np.array_equal(d_payload.cpu().numpy(), sent)
    for x in (tb, enc, dec, rm, awgn):
        x.close()


@pytest.mark.parametrize("qm", [2, 4, 6, 8])
def test_round_trip_without_noise(qams, qm):
    q = qams[qm]
    rng = np.random.default_rng(20 + qm)
    bits = rng.integers(0, 2, (B, qm * S)).astype(np.uint8)
    for f64 in (True, False):
        for max_log in (False, True):
            for c_init in (-1, 1):
                llrs = q.demodulate(q.modulate(bits, c_init, f64), 0.05, max_log, c_init)
                assert np.isfinite(llrs).all() and (llrs != 0).all() and np.array_equal((llrs < 0).astype(np.uint8), bits)
    # descrambling with the wrong sequence does not give the bits back
    wrong = q.demodulate(q.modulate(bits, 1, True), 0.05, False, 2)
    assert not np.array_equal((wrong < 0).astype(np.uint8), bits)
