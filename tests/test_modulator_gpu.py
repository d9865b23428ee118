"""GPU: the batched modulator (ldpc_toolbox_mod_run_*) and AWGN channel (ldpc_toolbox_awgn_run_*) against
tests/channel_restatement.py (pinned to the oracle by tests/test_channel_restatement.py), against the simulator's own
generators, and chained between the encoder and the demapper on one stream.  Equality is demod_restatement.same_bits."""
import numpy as np
import pytest
import torch

import channel_restatement as cr
import constellation_cases as cc
import demod_restatement as dr
import ldpc_toolbox_amd as lt
from demod_restatement import same_bits
from ldpc_toolbox_amd import simulation as sim

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 8), (3, 171)]      # 171 symbols x 3 rows = 513 threads: past one 256-thread block, no multiple of 64
BIG_FRAME = 2 ** 32 + 12345      # a first_frame whose high counter word is not zero
BIG_SEED = 0xF234567887654321    # a seed with high bits set

_demods = {}


def demod(name):
    if name not in _demods:
        _demods[name] = lt.Demodulator("BPSK", device=0) if name == "BPSK" else cc.make_demodulator(lt, name)
    return _demods[name]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for d in _demods.values():
        d.close()
    _demods.clear()


def points(name):
    return None if name == "BPSK" else cc.TABLES[name][0]


def m_of(name):
    return 1 if name == "BPSK" else cc.bits_of(name)


def interleavings(name, symbols):
    """0, m, -m and another divisor of m * symbols"""
    m = m_of(name)
    return (0, m, -m, 4 if symbols == 8 else -19)


def some_bits(shape, seed):
    """bytes 0, 1, 2 and 255: only a byte equal to 1 is a one"""
    rng = np.random.default_rng(seed)
    b = rng.choice(np.array([0, 1, 1, 1, 2, 255], dtype=np.uint8), shape)
    b.flat[:4] = [0, 1, 2, 255]
    return b


def as_reals(x):
    return x.view(x.real.dtype) if np.iscomplexobj(x) else x


def _complex(real, is_real):
    if is_real:
        return real
    return np.complex128 if real == np.float64 else np.complex64


def to_dev(arr, offset=0):
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    d = torch.full((offset + raw.size,), 0x5A, dtype=torch.uint8, device=DEV)
    d[offset:] = torch.from_numpy(raw).to(DEV)
    return d


def mod_device(name, bits, f64, interleaving, stream=0, in_offset=0, out_offset=0, margin=0):
    """bits [B][n] -> symbols through the device entry; with offsets / margin also the sentinel bytes around the output"""
    d = demod(name)
    B, n = bits.shape
    S = n // m_of(name)
    real = np.float64 if f64 else np.float32
    per = 1 if name == "BPSK" else 2
    out_bytes = B * S * per * np.dtype(real).itemsize
    d_bits = to_dev(bits, in_offset)
    d_out = torch.full((out_offset + out_bytes + margin,), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    d.modulate_device(d_bits.data_ptr() + in_offset, d_out.data_ptr() + out_offset, f64, B, n, interleaving, stream)
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    syms = host[out_offset:out_offset + out_bytes].copy().view(_complex(real, name == "BPSK")).reshape(B, S)
    return (syms, host[:out_offset], host[out_offset + out_bytes:]) if (margin or out_offset) else syms


def awgn_device(name, symbols, sigma, seed, first_frame, stream=0, offset=0, margin=0):
    d = demod(name)
    B, S = symbols.shape
    f64 = symbols.real.dtype == np.float64
    nbytes = symbols.nbytes
    d_sym = torch.full((offset + nbytes + margin,), 0xA5, dtype=torch.uint8, device=DEV)
    d_sym[offset:offset + nbytes] = torch.from_numpy(np.ascontiguousarray(symbols).view(np.uint8).reshape(-1)).to(DEV)
    torch.cuda.synchronize()
    d.add_noise_device(d_sym.data_ptr() + offset, f64, B, S, sigma, seed, first_frame, stream)
    torch.cuda.synchronize()
    host = d_sym.cpu().numpy()
    out = host[offset:offset + nbytes].copy().view(symbols.dtype).reshape(B, S)
    return (out, host[:offset], host[offset + nbytes:]) if (margin or offset) else out


NAMES = ["two", "QPSK", "8PSK", "rings16", "rings32"]


# ---- 1: the modulator ---------------------------------------------------------------------------------

@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", NAMES + ["BPSK"])
def test_modulator_equals_the_restatement(name, shape, f64):
    B, S = shape
    bits = some_bits((B, S * m_of(name)), seed=S + m_of(name))
    real = np.float64 if f64 else np.float32
    for il in interleavings(name, S):
        want = cr.modulate(bits, points(name), il, real)
        assert want.dtype == _complex(real, name == "BPSK")
        host = demod(name).modulate(bits, il, f64)
        assert host.dtype == want.dtype and same_bits(as_reals(host), as_reals(want)), (name, il, "host")
        assert same_bits(as_reals(mod_device(name, bits, f64, il)), as_reals(want)), (name, il, "device")


# ---- 2: the channel -----------------------------------------------------------------------------------

@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", ["8PSK", "rings32", "BPSK"])
def test_awgn_equals_the_restatement(name, shape, f64):
    """complex symbols keyed by symbol, BPSK reals keyed by position pair (171 positions: the last pair half used); a
    first_frame beyond 2^32 and a seed with high bits set reach the upper counter and key words"""
    B, S = shape
    real = np.float64 if f64 else np.float32
    syms = cr.modulate(some_bits((B, S * m_of(name)), seed=S), points(name), 0, real)
    for sigma, seed, first in ((0.5, 7, 0), (0.05, BIG_SEED, BIG_FRAME), (3.0, 2 ** 63, 2 ** 64 - 2)):
        want = cr.awgn(syms, sigma, seed, first)
        assert want.dtype == syms.dtype and not np.array_equal(want, syms)
        host = demod(name).add_noise(syms, sigma, seed, first)
        assert host.dtype == want.dtype and same_bits(as_reals(host), as_reals(want)), (name, sigma, "host")
        assert same_bits(as_reals(awgn_device(name, syms, sigma, seed, first)), as_reals(want)), (name, sigma, "device")
    # frames are keyed by number, not by row: rows 1.. of a call at first_frame are rows 0.. of a call at first_frame + 1
    if B > 1:
        a = demod(name).add_noise(syms, 0.5, BIG_SEED, BIG_FRAME)
        b = demod(name).add_noise(syms[1:], 0.5, BIG_SEED, BIG_FRAME + 1)
        assert same_bits(as_reals(a[1:]), as_reals(b))
    # sigma = 0 returns the input
    assert same_bits(as_reals(demod(name).add_noise(syms, 0.0, 7, 3)), as_reals(syms))
    assert same_bits(as_reals(awgn_device(name, syms, 0.0, 7, 3)), as_reals(syms))


# ---- 3: pointers, margins, empty batches, refused arguments ---------------------------------------------

@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("name", ["8PSK", "BPSK"])
def test_offset_pointers_and_margins(name, f64):
    """bits 3 bytes and symbols one element into their buffers (no alignment beyond the element's is assumed); the bytes
    before and after what a call may write keep their sentinel"""
    real = np.float64 if f64 else np.float32
    off = np.dtype(real).itemsize
    bits = some_bits((3, 171 * m_of(name)), seed=9)
    il = 0 if name == "BPSK" else -3
    got, before, after = mod_device(name, bits, f64, il, in_offset=3, out_offset=off, margin=4096)
    assert (before == 0xA5).all() and (after == 0xA5).all() and len(after) == 4096
    want = cr.modulate(bits, points(name), il, real)
    assert same_bits(as_reals(got), as_reals(want))
    got, before, after = awgn_device(name, want, 0.5, BIG_SEED, BIG_FRAME, offset=off, margin=4096)
    assert (before == 0xA5).all() and (after == 0xA5).all() and len(after) == 4096
    assert same_bits(as_reals(got), as_reals(cr.awgn(want, 0.5, BIG_SEED, BIG_FRAME)))


def test_batch_zero_and_refused_arguments_write_nothing():
    from ldpc_toolbox_amd import _capi
    L = _capi.lib()
    d = demod("8PSK")
    d_out = torch.full((8192,), 0xA5, dtype=torch.uint8, device=DEV)
    d_bits = torch.ones(8192, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.Stream(device=DEV)
    for f64 in (False, True):
        d.modulate_device(d_bits.data_ptr(), d_out.data_ptr(), f64, 0, 24, 3)
        d.add_noise_device(d_out.data_ptr(), f64, 0, 8, 0.5, 1, 0)
        for s in (0, stream.cuda_stream):
            with pytest.raises(ValueError):     # bits_len != m * symbols_len
                d.modulate_device(d_bits.data_ptr(), d_out.data_ptr(), f64, 3, 24, 0, s, symbols_len=7)
            with pytest.raises(ValueError):     # |interleaving| does not divide bits_len
                d.modulate_device(d_bits.data_ptr(), d_out.data_ptr(), f64, 3, 24, 5, s)
            with pytest.raises(ValueError):     # bits_len > 0x7fffffff
                d.modulate_device(d_bits.data_ptr(), d_out.data_ptr(), f64, 1, 3 * 2 ** 30, 0, s)
            for sigma in (-0.5, float("inf"), float("nan")):
                with pytest.raises(ValueError):
                    d.add_noise_device(d_out.data_ptr(), f64, 3, 8, sigma, 1, 0, s)
        mod = L.ldpc_toolbox_mod_run_f64_device if f64 else L.ldpc_toolbox_mod_run_f32_device
        awgn = L.ldpc_toolbox_awgn_run_f64_device if f64 else L.ldpc_toolbox_awgn_run_f32_device
        assert mod(None, d_out.data_ptr(), 8, d_bits.data_ptr(), 24, 3, 0, None) == -4         # null handle
        assert awgn(None, d_out.data_ptr(), 8, 3, 0.5, 1, 0, None) == -4
    stream.synchronize()
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xA5).all()
    # host entries: shapes of an empty batch, and a refused call raises before anything is returned
    assert d.modulate(np.zeros((0, 24), dtype=np.uint8), 3).shape == (0, 8)
    assert d.add_noise(np.zeros((0, 8), dtype=np.complex64), 0.5, 1).shape == (0, 8)
    with pytest.raises(ValueError):
        d.modulate(np.zeros((2, 24), dtype=np.uint8), 5)
    with pytest.raises(ValueError):
        d.add_noise(np.zeros((2, 8), dtype=np.complex128), -1.0, 1)


# ---- 4: the chain against the simulator's generators ------------------------------------------------------

SPEC = "nr5g:2:6"        # n = 312 = 3 * 104
FRAMES, FIRST, SEED, EBN0 = 600, 100, 21, 4.0


@pytest.mark.parametrize("interleaving", [0, 3, -3])
def test_psk8_chain_equals_the_simulator(interleaving):
    """float32(demod_f64(awgn_f64(mod_f64(tx[idx])))) is what Simulator(modulation="8PSK") generates"""
    s = lt.Simulator(lt.code_alist(SPEC), "Minsumf32", device=0, pool_size=5, pool_seed=4, modulation="8PSK",
                     interleaving=interleaving)
    _, tx = s.pool_data()
    want, idx = s.generate(EBN0, SEED, FIRST, FRAMES)
    sigma = sim.noise_sigma(s.rate, EBN0, 3.0)
    d = demod("8PSK")
    rx = d.add_noise(d.modulate(tx[idx], interleaving, True), sigma, SEED, FIRST)
    got = d.demodulate(rx, sigma, interleaving).astype(np.float32)
    assert rx.dtype == np.complex128 and same_bits(got, want)
    s.close()


def test_bpsk_f32_chain_equals_the_simulator():
    s = lt.Simulator(lt.code_alist(SPEC), "Minsumf32", device=0, pool_size=5, pool_seed=4)
    _, tx = s.pool_data()
    want, idx = s.generate(EBN0, SEED, FIRST, FRAMES)
    sigma = sim.noise_sigma(s.rate, EBN0)
    d = demod("BPSK")
    rx = d.add_noise(d.modulate(tx[idx], 0, False), sigma, SEED, FIRST)
    got = d.demodulate(rx, sigma)
    assert rx.dtype == np.float32 and got.dtype == np.float32 and same_bits(got, want)
    s.close()


# ---- 5: encoder -> modulator -> channel -> demapper -> decoder on one stream ---------------------------------

CHAIN_EBN0_DB = 3.0     # dvbs2:R1_2short over 8PSK, plain min-sum, 30 iterations: most frames decode (checked below)


def test_transmit_and_receive_chain_on_one_stream():
    alist = lt.code_alist("dvbs2:R1_2short")
    enc = lt.Encoder(alist)
    dec = lt.LdpcDecoder(alist, "Minsumf32", device=0)
    d = demod("8PSK")
    frames, n, k = 64, dec.n, dec.k
    assert n == 16200 and n % 3 == 0
    msgs = np.random.default_rng(64).integers(0, 2, (frames, k), dtype=np.uint8)
    sigma = sim.noise_sigma(k / n, CHAIN_EBN0_DB, 3.0)
    # the host-side composition, entry by entry
    cws = enc.encode_batch(msgs)
    rx = d.add_noise(d.modulate(cws, 3, False), sigma, BIG_SEED, BIG_FRAME)
    want_llrs = d.demodulate(rx, sigma, 3)
    assert want_llrs.dtype == np.float32
    want_bits, want_its, _ = dec.decode_batch(want_llrs, 30)
    assert (want_its < 0).sum() < frames // 4, "the Eb/N0 of this test no longer lets most frames decode"
    assert np.array_equal(want_bits[want_its >= 0][:, :k], msgs[want_its >= 0])
    # the same on one stream of the caller's, device pointers only, nothing in between
    d_msgs = torch.from_numpy(msgs).to(DEV)
    d_cws = torch.zeros((frames, n), dtype=torch.uint8, device=DEV)
    d_sym = torch.zeros((frames, n // 3, 2), dtype=torch.float32, device=DEV)
    d_llrs = torch.zeros((frames, n), dtype=torch.float32, device=DEV)
    d_bits = torch.zeros((frames, n), dtype=torch.uint8, device=DEV)
    d_its = torch.zeros(frames, dtype=torch.int32, device=DEV)
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    st = stream.cuda_stream
    enc.encode_batch_device(d_msgs.data_ptr(), d_cws.data_ptr(), frames, st)
    d.modulate_device(d_cws.data_ptr(), d_sym.data_ptr(), False, frames, n, 3, st)
    d.add_noise_device(d_sym.data_ptr(), False, frames, n // 3, sigma, BIG_SEED, BIG_FRAME, st)
    d.demodulate_device(d_sym.data_ptr(), d_llrs.data_ptr(), False, frames, n // 3, sigma, 3, False, st)
    dec.decode_batch_device(d_llrs.data_ptr(), False, frames, 30, d_bits.data_ptr(), n, d_its.data_ptr(), 0, st)
    stream.synchronize()
    assert np.array_equal(d_cws.cpu().numpy(), cws)
    assert same_bits(d_sym.cpu().numpy().reshape(frames, -1), rx.view(np.float32))
    assert same_bits(d_llrs.cpu().numpy(), want_llrs)
    assert np.array_equal(d_bits.cpu().numpy(), want_bits) and np.array_equal(d_its.cpu().numpy(), want_its)
    enc.close()
    dec.close()
