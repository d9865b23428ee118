"""GPU: the NR demapper with a scale per symbol (ldpc_toolbox_nr_demap_csi_*) and the Rayleigh block-fading channel
(ldpc_toolbox_fading_run_*) against the numpy restatement (tests/nr_csi_restatement.py), bit for bit.  Equality is
demod_restatement.same_bits: NaN where the restatement has NaN, else the same bits; soft bits are compared as bytes.

Shapes: [3][67] symbols (201 threads: one partial block of 256) and [5][131] (655: two full blocks and a ragged third).
Inputs: mapper output plus noise with +-0 coordinates and a coordinate of 1e30 planted; scales 2^U(-10, 10) with 0, a float
subnormal, 1e30 and one NaN planted.  Every restated row is computed once and shared."""
import numpy as np
import pytest
import torch

import channel_restatement as cr
import ldpc_toolbox_amd as lt
import nr_csi_restatement as nc
import nr_qam_reference as nq
import nr_soft_i8_restatement as sr
from demod_restatement import same_bits

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = ((3, 67), (5, 131))
C_INIT = 0x2A5A5A5            # a 31-bit value
GUARD = 0x6E


@pytest.fixture(scope="module")
def qams():
    q = {qm: lt.NrQam(qm, device=0) for qm in (2, 4, 6, 8)}
    yield q
    for x in q.values():
        x.close()


_INPUTS, _WANT = {}, {}


def inputs(qm, shape, f64):
    """(symbols, scales) of one (QM, shape), complex128 / float64 or their roundings to complex64 / float32"""
    key = (qm, shape)
    if key not in _INPUTS:
        B, S = shape
        rng = np.random.default_rng(1000 * qm + S)
        bits = rng.integers(0, 2, (B, qm * S), dtype=np.uint8)
        sym = cr.awgn(nq.modulate(bits, qm, C_INIT), 0.3, 77, 5)
        sym[1, 3] = complex(0.0, -0.0)
        sym[1, 4] = complex(-0.0, sym[1, 4].imag)
        sym[2, 5] = complex(1e30, sym[2, 5].imag)
        scale = np.exp2(rng.uniform(-10.0, 10.0, (B, S)))
        scale[0, 7], scale[0, 8], scale[0, 9], scale[0, 10] = 0.0, 1e-40, 1e30, np.nan
        scale[1, 3], scale[2, 5] = 1e30, 1e30       # (a +-0 symbol and the 1e30 coordinate under a huge scale)
        scale[2, S - 1] = 0.0
        for a in (sym, scale):
            a.setflags(write=False)
        _INPUTS[key] = (sym, scale)
    sym, scale = _INPUTS[key]
    return (sym, scale) if f64 else (sym.astype(np.complex64), scale.astype(np.float32))


def restated(qm, shape, f64, max_log, c_init):
    key = (qm, shape, f64, max_log, c_init)
    if key not in _WANT:
        sym, scale = inputs(qm, shape, f64)
        _WANT[key] = nc.demodulate_csi(sym, scale, qm, max_log, c_init)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def to_dev(a):
    real = a.real.dtype if np.iscomplexobj(a) else a.dtype
    return torch.from_numpy(np.array(a, order="C").view(real)).to(DEV)       # (a copy: the shared inputs are read-only)


def demap_csi_device(q, sym, scale, f64, max_log, c_init):
    """the device entry on a stream of the caller's"""
    d_sym, d_scale = to_dev(sym), to_dev(scale)
    d_out = torch.full((sym.shape[0], q.bits_per_symbol * sym.shape[1]), 12345.0, dtype=torch.float64 if f64 else torch.float32, device=DEV)
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    q.demodulate_csi_device(d_sym.data_ptr(), d_scale.data_ptr(), d_out.data_ptr(), f64, sym.shape[0], sym.shape[1], max_log, c_init,
                            stream.cuda_stream)
    stream.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("max_log", [False, True], ids=["exact", "max-log"])
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("qm", [2, 4, 6, 8])
def test_csi_demapper_equals_the_restatement(qams, qm, f64, max_log):
    q = qams[qm]
    for shape in SHAPES:
        sym, scale = inputs(qm, shape, f64)
        for c_init in (-1, C_INIT):
            want = restated(qm, shape, f64, max_log, c_init)
            finite = want[np.isfinite(want)]
            assert (finite > 0).any() and (finite < 0).any() and np.isnan(want).any()
            erased = want.reshape(shape[0], shape[1], qm)[0, 7]
            assert (erased == 0).all(), "scale 0 erases the symbol"
            got = q.demodulate_csi(sym, scale, max_log, c_init)
            assert same_bits(got, want), (qm, f64, max_log, shape, c_init, "host entry")
            assert same_bits(demap_csi_device(q, sym, scale, f64, max_log, c_init), want), (qm, f64, max_log, shape, c_init, "device entry")


@pytest.mark.parametrize("qm", [2, 4, 6, 8])
def test_constant_scale_is_the_scalar_entry(qams, qm):
    """every s the double 1 / (sigma * sigma): _f64 with either fold step at sigma 0.7, exact _f32 at sigma 0.5 (4.0 is a
    float) -- bit for bit what today's entry with that noise_sigma gives on the GPU"""
    q = qams[qm]
    shape = SHAPES[1]
    sym = inputs(qm, shape, True)[0].copy()
    sym[2, 5] = sym[2, 4]                            # (finite symbols: the identity is about the LLRs, not about NaN)
    for max_log in (False, True):
        scale = np.full(shape, 1.0 / (0.7 * 0.7))
        for c_init in (-1, C_INIT):
            want = q.demodulate(sym, 0.7, max_log, c_init)
            assert np.isfinite(want).all()
            assert same_bits(q.demodulate_csi(sym, scale, max_log, c_init), want), (qm, max_log, c_init)
            assert same_bits(demap_csi_device(q, sym, scale, True, max_log, c_init), want)
    sym32 = sym.astype(np.complex64)
    scale32 = np.full(shape, 4.0, dtype=np.float32)
    want = q.demodulate(sym32, 0.5, False, C_INIT)
    assert want.dtype == np.float32 and same_bits(q.demodulate_csi(sym32, scale32, False, C_INIT), want)
    assert same_bits(demap_csi_device(q, sym32, scale32, False, False, C_INIT), want)


@pytest.mark.parametrize("max_log", [False, True], ids=["exact", "max-log"])
@pytest.mark.parametrize("qm", [2, 4, 6, 8])
def test_soft_bit_demapper_at_every_byte_offset(qams, qm, max_log):
    """Q of the restated float row; the output at byte offsets 0 .. 3 of a 256-byte aligned allocation, so both the wide
    and the byte store paths run; guard bytes on both sides stay"""
    q = qams[qm]
    for shape in SHAPES:
        sym, scale = inputs(qm, shape, False)
        B, S = shape
        n = B * S * qm
        for c_init in (-1, C_INIT):
            want = sr.quantise(restated(qm, shape, False, max_log, c_init))
            assert want.dtype == np.int8 and (want == 127).any() and (want == -127).any() and (np.abs(want) < 127).any()
            if c_init == -1:
                assert np.array_equal(q.demap_csi_i8(sym, scale, max_log, c_init), want), (qm, max_log, shape, "host entry")
            d_sym, d_scale = to_dev(sym), to_dev(scale)
            stream = torch.cuda.Stream(device=DEV)
            outs = []
            for off in range(4):
                d_out = torch.full((n + 8,), GUARD, dtype=torch.int8, device=DEV)
                assert d_out.data_ptr() % 256 == 0
                torch.cuda.synchronize()
                q.demap_csi_i8_device(d_sym.data_ptr(), d_scale.data_ptr(), d_out.data_ptr() + off, B, S, max_log, c_init, stream.cuda_stream)
                outs.append(d_out)
            stream.synchronize()
            for off, d_out in enumerate(outs):
                got = d_out.cpu().numpy()
                assert (got[:off] == GUARD).all() and (got[off + n:] == GUARD).all(), f"guard bytes at offset {off}"
                assert np.array_equal(got[off:off + n].reshape(B, S * qm), want), (qm, max_log, shape, c_init, off)


# ---- the channel -------------------------------------------------------------------------------------------------------

FIRST_FRAME = (1 << 32) + 5     # reaches the counter's high word
ROWS, ROW = 5, 67


@pytest.fixture(scope="module")
def channel():
    d = lt.Demodulator("QPSK", device=0)     # (the channel reads nothing of the handle's table)
    yield d
    d.close()


def clean_symbols(f64):
    bits = np.random.default_rng(3).integers(0, 2, (ROWS, 6 * ROW), dtype=np.uint8)
    return nq.modulate(bits, 6, -1, np.float64 if f64 else np.float32)


@pytest.mark.parametrize("block", [1, 7, 67, 1000])
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
def test_fading_channel_equals_the_restatement(channel, f64, block):
    """no sharing, a block that does not divide the row, the whole row, longer than the row.  In place on the device, the
    scale buffer one element off a 256-byte boundary: only its element's alignment is asked"""
    real = np.float64 if f64 else np.float32
    sigma, seed = 0.37, 0x1234
    clean = clean_symbols(f64)
    want_sym, want_scale = nc.fading(clean, sigma, block, seed, FIRST_FRAME)
    assert want_scale.dtype == real and (want_scale > 0).all()
    shared = len(np.unique(want_scale[0]))
    assert shared == -(-ROW // block), "one gain per block"
    got_sym, got_scale = channel.add_fading(clean, sigma, block, seed, FIRST_FRAME)
    assert same_bits(got_sym.view(real), want_sym.view(real)) and same_bits(got_scale, want_scale), (f64, block, "host entry")
    d_sym = to_dev(clean)
    d_scale = torch.full((ROWS * ROW + 2,), -1.0, dtype=torch.float64 if f64 else torch.float32, device=DEV)
    assert d_scale.data_ptr() % 256 == 0
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    channel.add_fading_device(d_sym.data_ptr(), d_scale.data_ptr() + d_scale.element_size(), f64, ROWS, ROW, sigma, block, seed, FIRST_FRAME,
                              stream.cuda_stream)
    stream.synchronize()
    scale = d_scale.cpu().numpy()
    assert scale[0] == -1.0 and scale[-1] == -1.0
    assert same_bits(d_sym.cpu().numpy(), want_sym.view(real)) and same_bits(scale[1:-1].reshape(ROWS, ROW), want_scale), (f64, block, "device entry")


def test_fading_rows_are_frames(channel):
    """row r is frame first_frame + r: two calls of a part each give the rows of one call"""
    clean = clean_symbols(False)
    whole = channel.add_fading(clean, 0.5, 7, 9, FIRST_FRAME)
    parts = channel.add_fading(clean[:2], 0.5, 7, 9, FIRST_FRAME), channel.add_fading(clean[2:], 0.5, 7, 9, FIRST_FRAME + 2)
    for i in (0, 1):
        assert np.array_equal(np.concatenate([parts[0][i], parts[1][i]]).view(np.float32), whole[i].view(np.float32))


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("qm", [4, 8])
def test_chain_on_one_stream(qams, channel, qm, f64):
    """mapper -> fading channel -> demapper with the channel's scales, device entries on one stream of the caller's, no host
    round trip: the composition of the restatements"""
    q = qams[qm]
    real = np.float64 if f64 else np.float32
    B, S, sigma, block, seed = 5, 131, 0.2, 12, 41
    bits = np.random.default_rng(qm).integers(0, 2, (B, qm * S), dtype=np.uint8)
    want_sym, want_scale = nc.fading(nq.modulate(bits, qm, C_INIT, real), sigma, block, seed, 3)
    t = torch.float64 if f64 else torch.float32
    d_bits = torch.from_numpy(bits).to(DEV)
    d_sym, d_scale = torch.zeros((B, 2 * S), dtype=t, device=DEV), torch.zeros((B, S), dtype=t, device=DEV)
    d_llrs = {ml: torch.zeros((B, qm * S), dtype=t, device=DEV) for ml in (False, True)}
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    st = stream.cuda_stream
    q.modulate_device(d_bits.data_ptr(), d_sym.data_ptr(), f64, B, qm * S, C_INIT, st)
    channel.add_fading_device(d_sym.data_ptr(), d_scale.data_ptr(), f64, B, S, sigma, block, seed, 3, st)
    for ml in (False, True):
        q.demodulate_csi_device(d_sym.data_ptr(), d_scale.data_ptr(), d_llrs[ml].data_ptr(), f64, B, S, ml, C_INIT, st)
    stream.synchronize()
    assert same_bits(d_sym.cpu().numpy(), want_sym.view(real)) and same_bits(d_scale.cpu().numpy(), want_scale)
    for ml in (False, True):
        want = nc.demodulate_csi(want_sym, want_scale, qm, ml, C_INIT)
        assert same_bits(d_llrs[ml].cpu().numpy(), want), (qm, f64, ml)
