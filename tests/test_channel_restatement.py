"""CPU: tests/channel_restatement.py (the numpy modulator and AWGN channel the GPU tests compare against) pinned to the
oracle's Philox, 8PSK modulator, interleaver and frame generators and to the reference's own 8PSK vector; and the pure host
argument checks of the new entries through a stand-alone driver built under ASan/UBSan."""
import json
import os
import subprocess

import numpy as np
import pytest

import channel_restatement as cr
import demod_restatement as dr
import ldpc_toolbox_amd as lt
from demod_restatement import same_bits
from ldpc_toolbox_amd import simulation as sim

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")))
SPEC = "nr5g:2:6"        # n = 312 = 3 * 104


def test_philox_equals_the_oracle_on_1000_counters(oracle):
    rng = np.random.default_rng(1000)
    ctr = rng.integers(0, 1 << 32, (1000, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, (1000, 2), dtype=np.uint64)
    ctr[:4] = [[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0xFFFFFFFF, 0xFFFFFFFF, 5, 0], [1, 0, 0, 0xFFFFFFFF]]
    key[:2] = [[0, 0], [0xFFFFFFFF, 0xFFFFFFFF]]
    got = cr.philox4x32_10(ctr, key)
    assert got.dtype == np.uint32
    for i in range(1000):
        assert np.array_equal(got[i], oracle.philox4x32_10(ctr[i], key[i])), i


def test_unit_is_exact_and_in_range():
    w = np.array([0, 255, 256, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
    assert list(cr.unit(w)) == [-1.0, -1.0, -1.0 + 2.0 ** -23, 0.0, 1.0 - 2.0 ** -23]


@pytest.mark.parametrize("columns", [0, 3, -3, 4, -6])
def test_modulate_equals_the_oracle_modulator_and_interleaver(oracle, columns):
    bits = np.random.default_rng(24).integers(0, 2, (5, 24), dtype=np.uint8)
    want = np.stack([oracle.psk8_modulate(oracle.interleave(b, abs(columns), columns < 0) if columns else b) for b in bits])
    assert same_bits(cr.modulate(bits, dr.PSK8, columns).view(np.float64), want.view(np.float64))
    # bytes other than 1 are zeros (the encoder's convention)
    odd = bits.copy()
    odd[bits == 0] = np.resize(np.array([0, 2, 255, 3], dtype=np.uint8), int((bits == 0).sum()))
    assert np.array_equal(cr.modulate(odd, dr.PSK8, columns), cr.modulate(bits, dr.PSK8, columns))


def test_modulate_reproduces_the_reference_vector():
    t = KATS["psk8"]                                   # modulation.rs:311-346
    got = cr.modulate(np.array([t["modulator_bits"]], dtype=np.uint8), dr.PSK8)[0]
    want = np.array([complex(*p) for p in t["modulator_symbols_in_units_of_sqrt_half"]]) * np.sqrt(0.5)
    assert np.allclose(got, want, rtol=0, atol=1e-15)


def _pool(spec=SPEC, pool=5, seed=4):
    """a pool of codewords as the simulator makes one, without a GPU: random messages through the host encoder"""
    alist = lt.code_alist(spec)
    enc = lt.Encoder(alist)
    h = lt.SparseMatrix.from_alist(alist)
    n, k = h.num_cols(), h.num_cols() - h.num_rows()
    msgs = np.random.default_rng(seed).integers(0, 2, (pool, k), dtype=np.uint8)
    return np.stack([enc.encode(m, n) for m in msgs]), k / n


@pytest.mark.parametrize("interleaving", [0, 3, -3])
def test_psk8_chain_equals_the_oracle_generator(oracle, interleaving):
    """float32(demodulate(awgn(modulate(tx)))) is oracle.generate_llrs_psk8, bit for bit, on 40 frames"""
    tx, rate = _pool()
    for ebn0, seed, first in ((4.0, 21, 0), (-2.0, 2 ** 41 + 5, 2 ** 34)):
        want, idx = oracle.generate_llrs_psk8(tx, rate, ebn0, interleaving, seed, first, 40)
        sigma = sim.noise_sigma(rate, ebn0, 3.0)
        rx = cr.awgn(cr.modulate(tx[idx], dr.PSK8, interleaving), sigma, seed, first)
        got = dr.demodulate(rx, sigma, dr.PSK8, interleaving=interleaving).astype(np.float32)
        assert same_bits(got, want), (interleaving, ebn0)


def test_bpsk_f32_chain_equals_the_oracle_generator(oracle):
    """BPSK in float32: llr = scale * (sym + sigma * z) with the noise keyed by position pairs -- oracle.generate_llrs.
    nr5g:2:6 has an even length; a 311-bit pool (odd: the last pair half used) goes through the same comparison."""
    tx, rate = _pool()
    for bits in (tx, tx[:, :311]):
        for ebn0, seed, first in ((2.0, 7, 0), (-1.0, 2 ** 63 + 11, 2 ** 40 - 3)):
            want, idx = oracle.generate_llrs(bits, rate, ebn0, seed, first, 40)
            sigma = sim.noise_sigma(rate, ebn0)
            rx = cr.awgn(cr.modulate(bits[idx], None, 0, np.float32), np.float32(sigma), seed, first)
            assert rx.dtype == np.float32
            assert same_bits(dr.bpsk(rx, sigma), want)       # scale = float32(-2 / sigma^2), sigma the double


def rings(m):
    """2^m points on two rings of unequal energy, unit mean energy, labels in a fixed random order"""
    n = 1 << m
    r = np.where(np.arange(n) % 2 == 0, 0.6, np.sqrt(2.0 - 0.36))
    pts = r * np.exp(2j * np.pi * (np.arange(n) + 0.25) / n)
    return pts[np.random.default_rng(m).permutation(n)]


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5])
def test_modulate_then_noiseless_max_log_demap_returns_the_bits(m):
    pts = {2: dr.QPSK, 3: dr.PSK8}.get(m, rings(m))
    n = 60 * m
    bits = np.random.default_rng(m).integers(0, 2, (3, n), dtype=np.uint8)
    for il in (0, m, -m, 6):
        syms = cr.modulate(bits, pts, il)
        assert same_bits(cr.awgn(syms, 0.0, 5, 1).view(np.float64), syms.view(np.float64))        # sigma 0: the input
        llrs = dr.demodulate(syms, 0.1, pts, energy_term=True, max_log=True, interleaving=il)
        assert np.array_equal((llrs < 0).astype(np.uint8), bits), (m, il)


def test_awgn_moments_and_keying():
    """the noise is standard normal, and frames, symbols and seeds draw different values"""
    z = cr.awgn(np.zeros((8, 4096), dtype=np.complex128), 1.0, 3, 10)
    x = np.concatenate([z.real.ravel(), z.imag.ravel()])
    assert abs(x.mean()) < 0.02 and abs(x.std() - 1.0) < 0.02 and abs((x ** 4).mean() - 3.0) < 0.15
    assert np.array_equal(cr.awgn(np.zeros((2, 16), dtype=np.complex128), 1.0, 3, 11)[0], z[1, :16])
    assert not np.array_equal(cr.awgn(np.zeros((1, 16), dtype=np.complex128), 1.0, 4, 10)[0], z[0, :16])
    # real symbols: position j takes pair j / 2, its first normal for even j, its second for odd j
    r = cr.awgn(np.zeros((8, 9), dtype=np.float64), 1.0, 3, 10)
    assert np.array_equal(r[:, 0::2], z.real[:, :5]) and np.array_equal(r[:, 1::2], z.imag[:, :4])


def test_channel_argument_checks_under_asan_ubsan(tmp_path):
    """csrc/demodulator.h: mod_argument_error, awgn_argument_error, mean_energy and sim_constellation_error, with their
    edges (length 0, INT32_MIN interleaving, a 32-point table, mean energy either side of the band)"""
    exe = str(tmp_path / "channel_args_driver")
    hip_include = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I" + hip_include, "-D__HIP_PLATFORM_AMD__", "-o", exe,
                    os.path.join(ROOT, "tests", "channel_args_driver.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "channel args driver: ok" in r.stdout


def test_new_entries_refuse_bad_arguments_without_a_gpu():
    """the argument checks come before the GPU is touched: they answer the same on a machine without one"""
    from ldpc_toolbox_amd import _capi
    L = _capi.lib()
    h = L.ldpc_toolbox_demod_ctor(b"8PSK", 0)
    buf = np.full(64, 7.0)
    bits = np.ones(24, dtype=np.uint8)
    ARG = -4
    for fn in (L.ldpc_toolbox_mod_run_f32, L.ldpc_toolbox_mod_run_f64):
        assert fn(None, buf.ctypes.data, 8, bits.ctypes.data, 24, 1, 0) == ARG
        assert fn(h, buf.ctypes.data, 7, bits.ctypes.data, 24, 1, 0) == ARG
        assert fn(h, buf.ctypes.data, 8, bits.ctypes.data, 24, 1, 5) == ARG
        assert fn(h, buf.ctypes.data, 8, bits.ctypes.data, 24, 1, -2 ** 31) == ARG
        assert fn(h, buf.ctypes.data, 2 ** 31, bits.ctypes.data, 3 * 2 ** 31, 1, 0) == ARG
        assert fn(h, buf.ctypes.data, 8, bits.ctypes.data, 24, 0, 3) == 0                      # batch 0
    for fn in (L.ldpc_toolbox_awgn_run_f32, L.ldpc_toolbox_awgn_run_f64):
        assert fn(None, buf.ctypes.data, 8, 1, 0.5, 1, 0) == ARG
        for sigma in (-0.5, float("inf"), float("nan")):
            assert fn(h, buf.ctypes.data, 8, 1, sigma, 1, 0) == ARG
        assert fn(h, buf.ctypes.data, 8, 0, 0.5, 1, 0) == 0
    assert (buf == 7.0).all()
    L.ldpc_toolbox_demod_dtor(h)
