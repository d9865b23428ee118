"""CPU: pins tests/demod_restatement.py -- the reference the GPU demodulator tests compare with -- to the oracle and to
the reference's own vectors, and checks the ldpc_toolbox_demod_* C surface as far as it goes without a GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import demod_restatement as dr
from ldpc_toolbox_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")))

ERR_DEVICE, ERR_ARGUMENT = -2, -4

SPECIALS, same_bits = dr.SPECIALS, dr.same_bits


@pytest.mark.parametrize("sigma", [0.05, 0.5, 3.0])
def test_restatement_equals_the_oracle_on_noisy_8psk(oracle, sigma):
    rng = np.random.default_rng(int(sigma * 100))
    n = 100_000
    syms = dr.PSK8[rng.integers(0, 8, n)] + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    assert same_bits(dr.demodulate(syms, sigma, dr.PSK8), oracle.psk8_demodulate(syms, sigma))


@pytest.mark.parametrize("sigma", [0.05, 0.5, 3.0])
def test_restatement_equals_the_oracle_on_specials(oracle, sigma):
    want = oracle.psk8_demodulate(SPECIALS, sigma)
    assert np.isnan(want).any() and not np.isnan(want).all()
    assert same_bits(dr.demodulate(SPECIALS, sigma, dr.PSK8), want)


def test_restatement_reproduces_the_reference_vectors():
    """modulation.rs:311-346, with the comparison tests/test_host_logic.py makes: the signs of the LLRs"""
    t = KATS["psk8"]
    a = np.sqrt(0.5)
    syms = np.array([complex(*(a if v == "a" else v for v in p)) for p in t["demodulator_symbols"]])
    llrs = dr.demodulate(syms, t["demodulator_sigma"], dr.PSK8)
    assert list(np.sign(llrs).astype(int)) == t["demodulator_llr_signs"]
    # the noiseless point of every label demodulates to its own bits (LLR > 0 <=> bit 0), for both named tables
    for pts in (dr.QPSK, dr.PSK8):
        m = len(pts).bit_length() - 1
        bits = np.array([[(v >> (m - 1 - j)) & 1 for j in range(m)] for v in range(len(pts))]).reshape(-1)
        for max_log in (False, True):
            assert np.array_equal(dr.demodulate(pts, 0.5, pts, max_log=max_log) <= 0, bits == 1)
    b = KATS["bpsk"]          # modulation.rs: BpskDemodulator's own vector
    assert np.allclose(dr.bpsk(np.array(b["demod_in"]), np.sqrt(b["sigma_squared"])), b["demod_out"], rtol=0, atol=b["tol"])


@pytest.mark.parametrize("columns", [3, -3, 4, -6])
def test_restatement_deinterleave_equals_the_oracle(oracle, columns):
    x = np.arange(24, dtype=np.float64) + 0.5
    assert np.array_equal(dr.deinterleave(x, columns), oracle.deinterleave(x, abs(columns), columns < 0))
    assert np.array_equal(dr.deinterleave(np.stack([x, -x]), columns)[1], oracle.deinterleave(-x, abs(columns), columns < 0))


# ---- the C surface without a GPU -------------------------------------------------------------------

def _get(L, h, key):
    v = C.c_int64(-99)
    assert L.ldpc_toolbox_demod_get(h, key.encode(), C.byref(v)) == 0
    return v.value


def test_constructors_and_properties():
    L = _capi.lib()
    for name, bits in (("BPSK", 1), ("QPSK", 2), ("8PSK", 3)):
        h = L.ldpc_toolbox_demod_ctor(name.encode(), 0)
        assert h, name
        assert (_get(L, h, "bits_per_symbol"), _get(L, h, "points"), _get(L, h, "energy_term")) == (bits, 1 << bits, 0)
        assert _get(L, h, "device") == -1        # no device state before the first run
        assert L.ldpc_toolbox_demod_get(h, b"no_such_key", C.byref(C.c_int64())) == -1
        L.ldpc_toolbox_demod_dtor(h)
    assert not L.ldpc_toolbox_demod_ctor(b"16QAM", 0) and "unknown modulation" in _capi.last_error()
    assert not L.ldpc_toolbox_demod_ctor(None, 0)
    pts = np.ones(128, dtype=np.float64)
    for bits in (0, 6):
        assert not L.ldpc_toolbox_demod_ctor_table(pts.ctypes.data, bits, 0, 0)
        assert "bits_per_symbol" in _capi.last_error()
    bad = np.ones(32, dtype=np.float64)
    bad[31] = np.nan
    assert not L.ldpc_toolbox_demod_ctor_table(bad.ctypes.data, 4, 1, 0) and "finite" in _capi.last_error()
    bad[31] = np.inf
    assert not L.ldpc_toolbox_demod_ctor_table(bad.ctypes.data, 4, 1, 0)
    h = L.ldpc_toolbox_demod_ctor_table(pts.ctypes.data, 4, 1, 0)
    assert h and (_get(L, h, "bits_per_symbol"), _get(L, h, "points"), _get(L, h, "energy_term")) == (4, 16, 1)
    L.ldpc_toolbox_demod_dtor(h)
    L.ldpc_toolbox_demod_dtor(None)


@pytest.mark.parametrize("entry", ["f32", "f64", "f32_device", "f64_device"])
def test_run_checks_its_arguments_before_the_gpu(entry):
    L = _capi.lib()
    h = L.ldpc_toolbox_demod_ctor(b"8PSK", 0)
    real = np.float32 if entry.startswith("f32") else np.float64
    sym = np.zeros((2, 8, 2), dtype=real)
    out = np.full((2, 24), 7.0, dtype=real)
    fn = getattr(L, "ldpc_toolbox_demod_run_" + entry)
    tail = (None,) if entry.endswith("_device") else ()

    def run(llrs_len=24, symbols_len=8, batch=2, sigma=0.5, interleaving=3, handle=h):
        return fn(handle, out.ctypes.data, llrs_len, sym.ctypes.data, symbols_len, batch, sigma, interleaving, 0, *tail)

    for kw in (dict(llrs_len=23), dict(symbols_len=7), dict(llrs_len=16, symbols_len=8), dict(sigma=0.0), dict(sigma=-1.0),
               dict(sigma=float("nan")), dict(sigma=float("inf")), dict(interleaving=5), dict(interleaving=-7),
               dict(interleaving=-2 ** 31), dict(handle=None)):
        assert run(**kw) == ERR_ARGUMENT, kw
        assert _capi.last_error()
    assert run(batch=0) == 0
    assert (out == 7.0).all()                    # nothing written by any of them
    if L.ldpc_toolbox_device_count() == 0:
        assert run() == ERR_DEVICE and "no HIP device" in _capi.last_error()
        assert run(interleaving=0) == ERR_DEVICE and run(interleaving=-3) == ERR_DEVICE
        assert (out == 7.0).all() and _get(L, h, "device") == -1
    L.ldpc_toolbox_demod_dtor(h)


def test_python_wrapper_without_a_gpu():
    import ldpc_toolbox_amd as lt
    d = lt.Demodulator("8PSK")
    assert (d.bits_per_symbol, d.points, d.energy_term, d.device) == (3, 8, False, -1)
    with pytest.raises(ValueError):
        lt.Demodulator("16QAM")
    with pytest.raises(ValueError):
        lt.Demodulator(np.ones(12, dtype=complex))
    t = lt.Demodulator(np.exp(2j * np.pi * np.arange(16) / 16), energy_term=True)
    assert (t.bits_per_symbol, t.points, t.energy_term) == (4, 16, True)
    with pytest.raises(ValueError):
        d.demodulate(np.zeros((1, 8), dtype=np.complex64), 0.0)
    with pytest.raises(ValueError):
        d.demodulate(np.zeros((1, 8), dtype=np.complex64), 0.5, interleaving=5)
    with pytest.raises(ValueError):
        lt.Demodulator("BPSK").demodulate(np.zeros((1, 8), dtype=np.complex64), 0.5)
    if _capi.lib().ldpc_toolbox_device_count() == 0:
        with pytest.raises(lt.DecoderUnavailable):
            d.demodulate(np.zeros((1, 8), dtype=np.complex64), 0.5, interleaving=3)
    d.close()
    t.close()
