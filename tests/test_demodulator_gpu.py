"""GPU: the batched soft demapper (ldpc_toolbox_demod_run_*) against the oracle's 8PSK demodulator and deinterleaver and
against tests/demod_restatement.py (pinned to the oracle by tests/test_demodulator_reference.py), and chained in front of
the decoder on one stream.  Equality is demod_restatement.same_bits: NaN where the reference has NaN, else the same bits."""
import numpy as np
import pytest
import torch

import demod_restatement as dr
import ldpc_toolbox_amd as lt
from ldpc_toolbox_amd import simulation as sim

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIGMAS = (0.05, 0.5, 3.0)


def same_bits(got, want):
    """demod_restatement.same_bits; a mismatch prints where it is and both values"""
    ok = dr.same_bits(got, want)
    if not ok and got.shape == want.shape and got.dtype == want.dtype:
        u = np.uint32 if got.dtype == np.float32 else np.uint64
        bad = np.flatnonzero(~(((got.view(u) == want.view(u)) & ~np.isnan(want)) | (np.isnan(got) & np.isnan(want))))
        print(f"{bad.size} of {got.size} differ; first at {bad[:8]}: got {got.flat[bad[:8]]!r}, want {want.flat[bad[:8]]!r}")
    return ok


def _real(f64):
    return np.float64 if f64 else np.float32


def run_device(demod, symbols, sigma, interleaving=0, max_log=False, stream=0, sym_offset=0, out_offset=0, margin=0):
    """symbols [B][S] complex (real for BPSK) numpy -> LLRs [B][m S] through the device entry.  The symbols start
    sym_offset bytes into their buffer and the LLRs out_offset bytes into theirs, followed by `margin` sentinel bytes
    (returned too)."""
    real = symbols.real.dtype if np.iscomplexobj(symbols) else symbols.dtype
    B, S = symbols.shape
    n = S * demod.bits_per_symbol
    raw = np.ascontiguousarray(symbols).view(np.uint8).reshape(-1)
    d_sym = torch.zeros(sym_offset + raw.size, dtype=torch.uint8, device=DEV)
    d_sym[sym_offset:] = torch.from_numpy(raw).to(DEV)
    out_bytes = B * n * real.itemsize
    d_out = torch.full((out_offset + out_bytes + margin,), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    demod.demodulate_device(d_sym.data_ptr() + sym_offset, d_out.data_ptr() + out_offset, real == np.float64, B, S, sigma,
                            interleaving, max_log, stream)
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    llrs = host[out_offset:out_offset + out_bytes].copy().view(real).reshape(B, n)
    return (llrs, host[:out_offset], host[out_offset + out_bytes:]) if (margin or out_offset) else llrs


def noisy(points, shape, sigma, seed):
    rng = np.random.default_rng(seed)
    return points[rng.integers(0, len(points), shape)] + sigma * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))


_demods = {}


def demod(key, make):
    if key not in _demods:
        _demods[key] = make()
    return _demods[key]


def psk8():
    return demod("8PSK", lambda: lt.Demodulator("8PSK", device=0))


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for d in _demods.values():
        d.close()
    _demods.clear()


def oracle_llrs(oracle, symbols, sigma, interleaving):
    """psk8_demodulate then deinterleave, frame by frame"""
    rows = [oracle.psk8_demodulate(row, sigma) for row in symbols]
    if interleaving:
        rows = [oracle.deinterleave(r, abs(interleaving), interleaving < 0) for r in rows]
    return np.stack(rows)


# ---- 1, 2: 8PSK, exact, against the oracle -----------------------------------------------------------

# (batch, symbols): 8 symbols; 513 threads = past one 256-thread block and no multiple of 64; the DVB-S2 normal frame
SHAPES = [((1, 8), il) for il in (0, 3, -3, 4, -6)] + [((3, 171), il) for il in (0, 3, -3)] + [((5, 21600), 3)]


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("shape,interleaving", SHAPES)
def test_psk8_f64_exact_equals_the_oracle(oracle, shape, interleaving, sigma):
    syms = noisy(dr.PSK8, shape, sigma, seed=shape[1])
    got = run_device(psk8(), syms, sigma, interleaving)
    assert same_bits(got, oracle_llrs(oracle, syms, sigma, interleaving))


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("interleaving", [0, 3, -3])
def test_psk8_specials_equal_the_oracle(oracle, interleaving, sigma):
    syms = dr.SPECIALS[None, :]
    want = oracle_llrs(oracle, syms, sigma, interleaving)
    assert np.isnan(want).any() and np.isfinite(want).any()
    assert same_bits(run_device(psk8(), syms, sigma, interleaving), want)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("shape,interleaving", [((1, 8), -6), ((3, 171), -3), ((5, 21600), 3)])
def test_psk8_f32_exact_is_the_rounded_f64_result(oracle, shape, interleaving, sigma):
    syms = noisy(dr.PSK8, shape, sigma, seed=7 + shape[1]).astype(np.complex64)
    syms[0, :3] = np.array([complex(np.inf, 1), complex(np.nan, 0), complex(-0.0, 1e-42)], dtype=np.complex64)
    want = oracle_llrs(oracle, syms.astype(np.complex128), sigma, interleaving).astype(np.float32)
    assert same_bits(run_device(psk8(), syms, sigma, interleaving), want)


# ---- 3: BPSK ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_bpsk_is_scale_times_x(f64, sigma):
    d = demod("BPSK", lambda: lt.Demodulator("BPSK", device=0))
    rng = np.random.default_rng(3)
    x = (rng.choice([-1.0, 1.0], (3, 172)) + sigma * rng.standard_normal((3, 172))).astype(_real(f64))
    with np.errstate(all="ignore"):      # (1e300 is inf in float32)
        x[1, :7] = dr._SPECIAL_VALUES
    scale = _real(f64)(-2.0 / (sigma * sigma))
    for interleaving in (0, -4):
        got = run_device(d, x, sigma, interleaving)
        with np.errstate(all="ignore"):
            assert same_bits(got, dr.deinterleave(scale * x, interleaving))
        assert same_bits(got, dr.bpsk(x, sigma, interleaving))


# ---- 4: other tables, both fold steps, both types, against the restatement ----------------------------------

def rings16():
    k = np.arange(8)
    return np.concatenate([np.exp(2j * np.pi * k / 8), 2.7 * np.exp(2j * np.pi * (k + 0.5) / 8)])


def rings32():
    pts = np.concatenate([1.0 * np.exp(2j * np.pi * (np.arange(4) + 0.5) / 4), 2.0 * np.exp(2j * np.pi * np.arange(12) / 12),
                          3.3 * np.exp(2j * np.pi * (np.arange(16) + 0.25) / 16)])
    return pts[np.random.default_rng(32).permutation(32)]      # labels: a fixed random permutation


TABLES = {
    "QPSK": (lambda: dr.QPSK, False, -2),
    "rings16": (rings16, True, 4),
    "rings16_no_energy": (rings16, False, 0),
    "rings32": (rings32, True, -5),
}


def table_demod(name):
    make, energy, _ = TABLES[name]
    if name == "QPSK":
        return demod(name, lambda: lt.Demodulator("QPSK", device=0))
    return demod(name, lambda: lt.Demodulator(make(), energy_term=energy, device=0))


@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("max_log", [False, True])
@pytest.mark.parametrize("name", list(TABLES))
def test_tables_equal_the_restatement(name, max_log, f64):
    make, energy, interleaving = TABLES[name]
    pts = make()
    syms = noisy(pts, (3, 171), 0.5, seed=len(name)).astype(np.complex128 if f64 else np.complex64)
    with np.errstate(all="ignore"):      # (1e300 is inf in complex64)
        syms[2, :len(dr.SPECIALS)] = dr.SPECIALS
    for il in (0, interleaving):
        want = dr.demodulate(syms, 0.5, pts, energy, max_log, il)
        assert want.dtype == _real(f64) and np.isfinite(want).sum() > want.size // 2
        assert same_bits(run_device(table_demod(name), syms, 0.5, il, max_log), want)


def test_energy_term_changes_the_result():
    syms = noisy(rings16(), (3, 171), 0.5, seed=16)
    with_e, without = (run_device(table_demod(n), syms, 0.5) for n in ("rings16", "rings16_no_energy"))
    assert not np.array_equal(with_e, without)
    assert same_bits(with_e, dr.demodulate(syms, 0.5, rings16(), True)) and same_bits(without, dr.demodulate(syms, 0.5, rings16(), False))


# ---- 5: entry forms -----------------------------------------------------------------------------------

@pytest.mark.parametrize("f64", [True, False])
def test_host_entry_equals_device_entry(f64):
    syms = noisy(dr.PSK8, (3, 171), 0.5, seed=5).astype(np.complex128 if f64 else np.complex64)
    for max_log in (False, True):
        host = psk8().demodulate(syms, 0.5, interleaving=-3, max_log=max_log)
        assert host.dtype == _real(f64) and same_bits(host, run_device(psk8(), syms, 0.5, -3, max_log))
    assert psk8().device == 0
    # the host entry again with a larger batch (its staging buffers grow) and on a handle made without a device index
    big = noisy(dr.PSK8, (7, 300), 0.5, seed=6).astype(syms.dtype)
    d = lt.Demodulator("8PSK")
    assert same_bits(d.demodulate(big, 0.5, 3), run_device(psk8(), big, 0.5, 3))
    d.close()


@pytest.mark.parametrize("f64", [True, False])
def test_offset_pointers_and_margin(oracle, f64):
    """LLRs 4 bytes and symbols 8 bytes into their buffers (no alignment beyond a float's is assumed); the bytes before
    and after the output keep their sentinel"""
    syms = noisy(dr.PSK8, (3, 171), 0.5, seed=8).astype(np.complex128 if f64 else np.complex64)
    want = oracle_llrs(oracle, syms.astype(np.complex128), 0.5, 3).astype(_real(f64))
    for max_log in (False, True):
        got, before, after = run_device(psk8(), syms, 0.5, 3, max_log, sym_offset=8, out_offset=4, margin=4096)
        assert (before == 0xA5).all() and (after == 0xA5).all() and len(after) == 4096
        if not max_log:
            assert same_bits(got, want)
        else:
            assert same_bits(got, dr.demodulate(syms, 0.5, dr.PSK8, max_log=True, interleaving=3))


def test_batch_zero_writes_nothing():
    d_out = torch.full((4096,), 0xA5, dtype=torch.uint8, device=DEV)
    d_sym = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    for f64 in (False, True):
        psk8().demodulate_device(d_sym.data_ptr(), d_out.data_ptr(), f64, 0, 8, 0.5, 3)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0xA5).all()
    assert psk8().demodulate(np.zeros((0, 8), dtype=np.complex64), 0.5).shape == (0, 24)


# ---- 6: the receive chain -------------------------------------------------------------------------------

CHAIN_EBN0_DB = 3.0     # dvbs2:R1_2short over 8PSK, plain min-sum, 30 iterations: most frames decode (checked below)


def test_chain_demodulate_then_decode_on_one_stream(oracle):
    alist = lt.code_alist("dvbs2:R1_2short")
    enc = lt.Encoder(alist)
    dec = lt.LdpcDecoder(alist, "Minsumf32", device=0)
    frames, n, k = 64, dec.n, dec.k
    assert n == 16200 and n % 3 == 0
    rng = np.random.default_rng(64)
    cws = enc.encode_batch(rng.integers(0, 2, (frames, k), dtype=np.uint8))
    tx = np.stack([oracle.psk8_modulate(oracle.interleave(cw, 3)) for cw in cws])
    sigma = sim.noise_sigma(k / n, CHAIN_EBN0_DB, 3.0)
    syms = (tx + sigma * (rng.standard_normal(tx.shape) + 1j * rng.standard_normal(tx.shape))).astype(np.complex64)
    # the same decoder fed the oracle's LLRs
    want_llrs = oracle_llrs(oracle, syms.astype(np.complex128), sigma, 3).astype(np.float32)
    want_bits, want_its, _ = dec.decode_batch(want_llrs, 30)
    obits, oits, _ = oracle.decode_batch(oracle.Graph(alist), "Minsumf32", want_llrs, 30, threads=4)
    assert (oits < 0).sum() < frames // 4, "the Eb/N0 of this test no longer lets most frames decode"
    assert np.array_equal(want_bits, obits) and np.array_equal(want_its, oits)
    # demodulate -> decode on one stream of the caller's, nothing in between
    d_sym = torch.from_numpy(syms.view(np.float32)).to(DEV)
    d_llrs = torch.zeros((frames, n), dtype=torch.float32, device=DEV)
    d_bits = torch.zeros((frames, n), dtype=torch.uint8, device=DEV)
    d_its = torch.zeros(frames, dtype=torch.int32, device=DEV)
    stream = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    psk8().demodulate_device(d_sym.data_ptr(), d_llrs.data_ptr(), False, frames, n // 3, sigma, 3, False, stream.cuda_stream)
    dec.decode_batch_device(d_llrs.data_ptr(), False, frames, 30, d_bits.data_ptr(), n, d_its.data_ptr(), 0, stream.cuda_stream)
    stream.synchronize()
    assert same_bits(d_llrs.cpu().numpy(), want_llrs)
    assert np.array_equal(d_bits.cpu().numpy(), want_bits) and np.array_equal(d_its.cpu().numpy(), want_its)
    enc.close()
    dec.close()
