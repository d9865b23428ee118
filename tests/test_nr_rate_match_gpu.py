"""GPU: batched NR rate matching and rate recovery (include/ldpc_toolbox.h, PART 6) byte for byte and bit for bit against
the numpy restatement of the standard's loops (tests/nr_rate_match_reference.py): every path of the index arithmetic on
small configurations, soft combining over four redundancy versions, the device entries on a stream, the refusals, and the
chain from the encoder to the decoder."""
import itertools

import numpy as np
import pytest
import torch

import ldpc_toolbox_amd as lt
import nr_rate_match_reference as rr
import oracle_binding as ob
from ldpc_toolbox_amd import _capi
from ldpc_toolbox_amd import simulation as sim

pytestmark = pytest.mark.gpu

QMS = (1, 2, 4, 6, 8)
BATCHES = (1, 3, 67)


def bits_of(a):
    """the values' bit patterns: -0.0 and +0.0 differ, as do two NaNs"""
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def soft_values(rng, shape, dtype):
    """values whose sum depends on the order of the additions: magnitudes from 1e-3 to 1e4 and full mantissas (the doubles
    are no floats); a few signed zeros"""
    v = rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 5, shape)
    v[rng.random(shape) < 0.02] = -0.0
    v = v.astype(dtype)
    if dtype == np.float64:
        assert (v.astype(np.float32).astype(np.float64) != v)[v != 0].all()
    return v


def e_values(L, qm):
    """3 Qm; about L / 2; the multiple of Qm at or below L; the next one above L; above 2 L (three repeats of some columns)"""
    return [3 * qm, max(L // 2 // qm, 1) * qm, max(L // qm, 1) * qm, (L // qm + 1) * qm, (2 * L // qm + 3) * qm]


@pytest.mark.parametrize("ncb", ["N", "N-7", 56])
@pytest.mark.parametrize("fillers", [0, 4, 5])
@pytest.mark.parametrize("bg", [2, 1])
def test_match_and_recover_equal_the_restatement(bg, fillers, ncb):
    zc = 2
    N = (66 if bg == 1 else 50) * zc
    ref = rr.Config(bg, zc, fillers, {"N": N, "N-7": N - 7}.get(ncb, ncb))
    rm = lt.NrRateMatcher(ref.spec, device=0)
    assert (rm.n, rm.buffer_len) == (ref.n, ref.L) and [rm.k0(rv) for rv in range(4)] == [ref.k0(rv) for rv in range(4)]
    rng = np.random.default_rng(1000 * bg + 10 * fillers + ref.ncb)
    repeats_seen = set()
    for case, (rv, qm) in enumerate(itertools.product(range(4), QMS)):
        for i, e in enumerate(e_values(ref.L, qm)):
            batch = BATCHES[(case + i) % 3]
            cws = rng.choice(np.array([0, 1, 1, 2, 255], dtype=np.uint8), (batch, ref.n))
            got = rm.match(cws, e, rv, qm)
            assert got.dtype == np.uint8 and np.array_equal(got, ref.match(cws, e, rv, qm)), (rv, qm, e, batch)
            repeats_seen.add(int(ref.repeats(e, rv).max()))
            for dtype in (np.float32, np.float64):
                rx = soft_values(rng, (batch, e), dtype)
                want = ref.recover(rx, rv, qm, 20.0)
                llrs = rm.recover(rx, rv, qm, filler_llr=20.0)
                assert llrs.dtype == dtype and np.array_equal(bits_of(llrs), bits_of(want)), (rv, qm, e, batch, dtype)
    assert {1, 2, 3} <= repeats_seen, "the table must reach three repeats of a column"
    rm.close()


@pytest.mark.parametrize("rv", range(4))
@pytest.mark.parametrize("spec", ["nr5g:1:384:40:16896", "nr5g:2:384:0"])
def test_standard_sizes_equal_the_restatement(spec, rv):
    """Zc = 384: BG 1 with 40 fillers and a limited buffer of two thirds of N, and BG 2 whole.  The divisors of the index
    arithmetic are in the ten-thousands and k0 is a multiple of 384.  E = 16896 (QPSK, part of the buffer), E = 60000
    (64QAM, some columns twice or more) and E = 2 L + 64 (256QAM, every column sent at least twice), every byte and bit."""
    ref = rr.Config(*(int(x) for x in spec.split(":")[1:]))
    rm = lt.NrRateMatcher(spec, device=0)
    assert (rm.n, rm.n_cb, rm.buffer_len) == (ref.n, ref.ncb, ref.L) and [rm.k0(v) for v in range(4)] == [ref.k0(v) for v in range(4)]
    assert ref.k0(rv) % 384 == 0 and (rv == 0 or ref.k0(rv) > 0)
    rng = np.random.default_rng(384 * ref.bg + rv)
    batch = 3
    sent = ref.buffer[:ref.ncb][ref.buffer[:ref.ncb] != rr.NULL]
    for e, qm in ((16896, 2), (60000, 6), (2 * ref.L + 8 * 8, 8)):
        if qm == 8:
            assert ref.repeats(e, rv)[sent].min() >= 2, "every column repeats"
        cws = rng.choice(np.array([0, 1, 1, 2, 255], dtype=np.uint8), (batch, ref.n))
        assert np.array_equal(rm.match(cws, e, rv, qm), ref.match(cws, e, rv, qm)), (e, qm)
        for dtype in (np.float32, np.float64):
            rx = soft_values(rng, (batch, e), dtype)
            llrs = rm.recover(rx, rv, qm, filler_llr=20.0)
            assert llrs.dtype == dtype and np.array_equal(bits_of(llrs), bits_of(ref.recover(rx, rv, qm, 20.0))), (e, qm, dtype)
    rm.close()


def test_k0_inside_the_filler_run():
    """BG2, Zc 2, F 4, Ncb 56, rv 1: k0 = 14 lies inside the fillers 12..15"""
    ref = rr.Config(2, 2, 4, 56)
    assert ref.k0(1) == 14 and ref.buffer[14] == rr.NULL
    rm = lt.NrRateMatcher(ref.spec, device=0)
    cws = np.random.default_rng(3).integers(0, 2, (5, ref.n), dtype=np.uint8)
    assert np.array_equal(rm.match(cws, 60, 1, 2), ref.match(cws, 60, 1, 2))
    rm.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("filler_llr", [float("inf"), 20.0])
def test_soft_combining_over_four_redundancy_versions(dtype, filler_llr):
    ref = rr.Config(2, 2, 4, 93)
    rm = lt.NrRateMatcher(ref.spec, device=0)
    rng = np.random.default_rng(77)
    batch = 67
    # a first transmission into a fresh buffer, then three more combined into it
    buf = want = None
    for rv, qm, e in ((0, 2, 40), (2, 4, 64), (3, 1, 30), (1, 8, 200)):
        rx = soft_values(rng, (batch, e), dtype)
        want = ref.recover(rx, rv, qm, filler_llr, old=want)
        buf = rm.recover(rx, rv, qm, filler_llr=filler_llr, into=buf)
        assert np.array_equal(bits_of(buf), bits_of(want)), (rv, qm, e)
    assert (buf[:, ref.k - 4:ref.k] == dtype(filler_llr)).all()
    assert (buf[:, :4] == 0).all() and (buf[:, 4 + 93:] == 0).all(), "columns outside the buffer were never sent"
    # combining into a buffer that holds values: untransmitted columns keep them, fillers are overwritten
    old = soft_values(rng, (batch, ref.n), dtype)
    rx = soft_values(rng, (batch, 24), dtype)
    got = rm.recover(rx, 1, 2, filler_llr=filler_llr, into=old.copy())
    assert np.array_equal(bits_of(got), bits_of(ref.recover(rx, 1, 2, filler_llr, old=old)))
    idle = ref.repeats(24, 1) == 0
    idle[ref.k - 4:ref.k] = False
    assert idle.sum() > 50 and np.array_equal(bits_of(got[:, idle]), bits_of(old[:, idle]))
    assert (got[:, ref.k - 4:ref.k] == dtype(filler_llr)).all()
    rm.close()


def test_device_entries_on_a_stream():
    ref = rr.Config(1, 2, 5, 125)
    rm = lt.NrRateMatcher(ref.spec, device=0)
    rng = np.random.default_rng(9)
    batch, e, rv, qm = 67, 6 * 47, 3, 6
    dev = torch.device("cuda", 0)
    cws = rng.integers(0, 2, (batch, ref.n), dtype=np.uint8)
    d_cws = torch.from_numpy(cws).to(dev)
    # (a row of 282 bytes: the passes' dword stores begin on every byte offset; one byte of slack at each end)
    d_tx = torch.full((batch * e + 2,), 0xEE, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    st = stream.cuda_stream
    rm.match_device(d_cws.data_ptr(), d_tx.data_ptr() + 1, batch, e, rv, qm, stream=st)
    got = {}
    for f64, dtype, tdtype in ((False, np.float32, torch.float32), (True, np.float64, torch.float64)):
        rx0, rx1 = soft_values(rng, (batch, e), dtype), soft_values(rng, (batch, e), dtype)
        d_rx0, d_rx1 = torch.from_numpy(rx0).to(dev), torch.from_numpy(rx1).to(dev)
        d_llrs = torch.full((batch, ref.n), 5.0, dtype=tdtype, device=dev)
        torch.cuda.synchronize()
        rm.recover_device(d_rx0.data_ptr(), d_llrs.data_ptr(), f64, batch, e, rv, qm, filler_llr=float("inf"), stream=st)
        rm.recover_device(d_rx1.data_ptr(), d_llrs.data_ptr(), f64, batch, e, 0, 2, filler_llr=9.0, combine=True, stream=st)
        got[dtype] = (d_llrs, ref.recover(rx1, 0, 2, 9.0, old=ref.recover(rx0, rv, qm, np.inf)))
    stream.synchronize()
    tx = d_tx.cpu().numpy()
    assert tx[0] == 0xEE and tx[-1] == 0xEE and np.array_equal(tx[1:-1].reshape(batch, e), ref.match(cws, e, rv, qm))
    for dtype, (d_llrs, want) in got.items():
        assert np.array_equal(bits_of(d_llrs.cpu().numpy()), bits_of(want)), dtype
    # NULL stream: the handle's own, synchronous
    d_tx2 = torch.zeros((batch, e), dtype=torch.uint8, device=dev)
    rm.match_device(d_cws.data_ptr(), d_tx2.data_ptr(), batch, e, 1, 2)
    assert np.array_equal(d_tx2.cpu().numpy(), ref.match(cws, e, 1, 2)) and rm.get("device") == 0
    rm.close()


def test_argument_errors_leave_the_output_untouched():
    rm = lt.NrRateMatcher("nr5g:2:2", device=0)
    n = rm.n
    dev = torch.device("cuda", 0)
    L = _capi.lib()
    d_cws = torch.zeros((3, n), dtype=torch.uint8, device=dev)
    d_tx = torch.full((3, 64), 0xAB, dtype=torch.uint8, device=dev)
    d_rx = torch.ones((3, 64), dtype=torch.float32, device=dev)
    d_llrs = torch.full((3, n), 7.5, dtype=torch.float32, device=dev)
    d_rx64 = torch.ones((3, 64), dtype=torch.float64, device=dev)
    d_llrs64 = torch.full((3, n), 7.5, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    for e, nn, rv, qm in ((0, n, 0, 1), (24, n - 1, 0, 1), (24, n + 1, 0, 1), (24, n, 4, 1), (24, n, 0, 0), (24, n, 0, 9), (25, n, 0, 2),
                          (1 << 31, n, 0, 1)):
        assert L.ldpc_toolbox_nr_rm_match_device(rm._h, d_tx.data_ptr(), e, d_cws.data_ptr(), nn, 3, rv, qm, None) == -4, (e, nn, rv, qm)
        for f, rx, llrs in ((L.ldpc_toolbox_nr_rm_recover_f32_device, d_rx, d_llrs), (L.ldpc_toolbox_nr_rm_recover_f64_device, d_rx64, d_llrs64)):
            assert f(rm._h, llrs.data_ptr(), nn, rx.data_ptr(), e, 3, rv, qm, 20.0, 0, None) == -4, (e, nn, rv, qm)
    for filler in (0.0, -1.0, float("nan"), float("-inf")):
        assert L.ldpc_toolbox_nr_rm_recover_f32_device(rm._h, d_llrs.data_ptr(), n, d_rx.data_ptr(), 24, 3, 0, 1, filler, 0, None) == -4
        assert L.ldpc_toolbox_nr_rm_recover_f64_device(rm._h, d_llrs64.data_ptr(), n, d_rx64.data_ptr(), 24, 3, 0, 1, filler, 1, None) == -4
    assert L.ldpc_toolbox_nr_rm_match_device(None, d_tx.data_ptr(), 24, d_cws.data_ptr(), n, 3, 0, 1, None) == -4
    assert L.ldpc_toolbox_nr_rm_recover_f32_device(None, d_llrs.data_ptr(), n, d_rx.data_ptr(), 24, 3, 0, 1, 20.0, 0, None) == -4
    assert L.ldpc_toolbox_nr_rm_match_device(rm._h, None, 24, d_cws.data_ptr(), n, 3, 0, 1, None) == -4
    assert L.ldpc_toolbox_nr_rm_recover_f32_device(rm._h, d_llrs.data_ptr(), n, None, 24, 3, 0, 1, 20.0, 0, None) == -4
    torch.cuda.synchronize()
    assert (d_tx == 0xAB).all() and (d_llrs == 7.5).all() and (d_llrs64 == 7.5).all()
    # the same through the host entries
    out = np.full((3, 64), 0xAB, dtype=np.uint8)
    assert L.ldpc_toolbox_nr_rm_match(rm._h, out.ctypes.data, 25, d_cws.cpu().numpy().ctypes.data, n, 3, 0, 2) == -4 and (out == 0xAB).all()
    with pytest.raises(ValueError, match="Qm must divide E"):
        rm.match(np.zeros((3, n), dtype=np.uint8), 25, qm=2)
    with pytest.raises(ValueError, match="filler LLR"):
        rm.recover(np.zeros((3, 24), dtype=np.float32), filler_llr=0.0)
    # an empty batch is no error
    assert rm.match(np.zeros((0, n), dtype=np.uint8), 24).shape == (0, 24)
    assert rm.recover(np.zeros((0, 24), dtype=np.float64)).shape == (0, n)
    rm.close()


def test_chain_from_the_encoder_to_the_decoder_on_one_stream():
    """nr5g:2:16 at E = 480 (rate 1/3), rv 0, Qm 2, QPSK: encode -> match -> modulate -> AWGN -> demap -> recover -> decode"""
    spec, e, rv, qm, frames, max_iter, ebn0_db = "nr5g:2:16", 480, 0, 2, 96, 30, 1.5
    alist = lt.code_alist(spec)
    enc = lt.Encoder(alist)
    dec = lt.LdpcDecoder(alist, "Minsumf32", device=0)
    rm = lt.NrRateMatcher(spec, device=0)
    d = lt.Demodulator("QPSK", device=0)
    ref = rr.Config(2, 16)
    n, k = dec.n, dec.k
    assert (n, k, rm.n) == (832, 160, 832)
    msgs = np.random.default_rng(2025).integers(0, 2, (frames, k), dtype=np.uint8)
    sigma = sim.noise_sigma(k / e, ebn0_db, 2)
    dev = torch.device("cuda", 0)
    d_msgs = torch.from_numpy(msgs).to(dev)
    d_cws = torch.zeros((frames, n), dtype=torch.uint8, device=dev)
    d_tx = torch.zeros((frames, e), dtype=torch.uint8, device=dev)
    d_sym = torch.zeros((frames, e // 2, 2), dtype=torch.float32, device=dev)
    d_rx = torch.zeros((frames, e), dtype=torch.float32, device=dev)
    d_llrs = torch.full((frames, n), 3.0, dtype=torch.float32, device=dev)
    d_bits = torch.zeros((frames, n), dtype=torch.uint8, device=dev)
    d_its = torch.zeros(frames, dtype=torch.int32, device=dev)
    d_post = torch.zeros((frames, n), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    st = stream.cuda_stream
    enc.encode_batch_device(d_msgs.data_ptr(), d_cws.data_ptr(), frames, st)
    rm.match_device(d_cws.data_ptr(), d_tx.data_ptr(), frames, e, rv, qm, stream=st)
    d.modulate_device(d_tx.data_ptr(), d_sym.data_ptr(), False, frames, e, 0, st)
    d.add_noise_device(d_sym.data_ptr(), False, frames, e // 2, sigma, 99, 1000, st)
    d.demodulate_device(d_sym.data_ptr(), d_rx.data_ptr(), False, frames, e // 2, sigma, 0, False, st)
    rm.recover_device(d_rx.data_ptr(), d_llrs.data_ptr(), False, frames, e, rv, qm, stream=st)
    dec.decode_batch_device(d_llrs.data_ptr(), False, frames, max_iter, d_bits.data_ptr(), n, d_its.data_ptr(), d_post.data_ptr(), st)
    stream.synchronize()
    cws = d_cws.cpu().numpy()
    assert np.array_equal(cws[:, :k], msgs) and np.array_equal(d_tx.cpu().numpy(), ref.match(cws, e, rv, qm))
    want_llrs = ref.recover(d_rx.cpu().numpy(), rv, qm, np.inf)
    assert np.array_equal(bits_of(d_llrs.cpu().numpy()), bits_of(want_llrs))
    obits, oits, opost = ob.decode_batch(ob.Graph(alist), "Minsumf32", want_llrs, max_iter, threads=4)
    bits, its, post = d_bits.cpu().numpy(), d_its.cpu().numpy(), d_post.cpu().numpy()
    assert np.array_equal(bits, obits) and np.array_equal(its, oits) and np.array_equal(post.astype(np.float64), opost)
    ok = (its >= 0) & (bits[:, :k] == msgs).all(axis=1)
    print(f"{frames} frames at rate {k}/{e}: {int(ok.sum())} decoded to the message, {int((its < 0).sum())} not converged")
    assert ok.sum() >= 10 and (its < 0).sum() >= 10
    # the host entries give the same
    assert np.array_equal(rm.match(cws, e, rv, qm), d_tx.cpu().numpy())
    assert np.array_equal(bits_of(rm.recover(d_rx.cpu().numpy(), rv, qm)), bits_of(want_llrs))
    for x in (enc, dec, rm, d):
        x.close()
