"""CPU: the surface of PART 10 (include/ldpc_toolbox.h) -- the NR demapper with a scale per symbol, the Rayleigh block-fading
channel beside the AWGN channel of PART 4, the simulator's "fading_block" key -- as far as it goes without a GPU: every symbol
exported, declared and bound, every refusal before the GPU is touched with nothing written, ERR_DEVICE where there is none;
and the numpy restatement (tests/nr_csi_restatement.py) pinned against the scalar restatement and the law of the gains."""
import os

import numpy as np
import pytest

import channel_restatement as cr
import ldpc_toolbox_amd as lt
import nr_csi_restatement as nc
import nr_qam_reference as nq
from demod_restatement import same_bits
from ldpc_toolbox_amd import _capi

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ERR_DEVICE, ERR_ARGUMENT = -2, -4       # include/ldpc_toolbox.h
CSI_SYMBOLS = tuple(f"ldpc_toolbox_nr_demap_csi_{t}{d}" for t in ("f32", "f64", "i8") for d in ("", "_device"))
FADING_SYMBOLS = tuple(f"ldpc_toolbox_fading_run_{t}{d}" for t in ("f32", "f64") for d in ("", "_device"))
MARK = 0x5B


def test_every_new_symbol_is_exported_declared_and_bound():
    L = _capi.lib()
    header = open(os.path.join(ROOT, "include", "ldpc_toolbox.h")).read()
    assert "PART 10" in header
    for name in CSI_SYMBOLS + FADING_SYMBOLS:
        assert name in _capi.SYMBOLS and getattr(L, name).argtypes is not None and f"int32_t {name}(" in header, name
        assert "nr_qam" not in name
    assert {"demodulate_csi", "demodulate_csi_device", "demap_csi_i8", "demap_csi_i8_device"} <= set(dir(lt.NrQam))
    assert {"add_fading", "add_fading_device"} <= set(dir(lt.Demodulator))


def marked(shape, dtype):
    """a buffer whose every byte is MARK"""
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8)[...] = MARK
    return a


def all_marked(*arrays):
    return all((a.view(np.uint8) == MARK).all() for a in arrays)


@pytest.mark.parametrize("name,real,out_t", [("f32", np.float32, np.float32), ("f64", np.float64, np.float64), ("i8", np.float32, np.int8)])
def test_csi_demapper_refusals_come_before_the_gpu_and_write_nothing(name, real, out_t):
    L = _capi.lib()
    q = lt.NrQam(6)
    S = 5
    sym, scale, llrs = marked((2, 2 * S), real), marked((2, S), real), marked((2, 6 * S), out_t)
    host, dev = getattr(L, "ldpc_toolbox_nr_demap_csi_" + name), getattr(L, "ldpc_toolbox_nr_demap_csi_" + name + "_device")
    p = llrs.ctypes.data, sym.ctypes.data, scale.ctypes.data
    # PART 8's refusals without the sigma test: the lengths, the frame length, c_init
    for ll, sl, c_init in ((6 * S, S + 1, -1), (6 * S + 1, S, -1), (6 * S - 6, S, -1), (6 * (1 << 29), 1 << 29, -1), (6 * S, S, -2), (6 * S, S, 1 << 31),
                           (6 * S, S, -(1 << 40))):
        for max_log in (0, 1):
            assert host(q._h, p[0], ll, p[1], p[2], sl, 2, max_log, c_init) == ERR_ARGUMENT and _capi.last_error(), (ll, sl, c_init)
            assert dev(q._h, p[0], ll, p[1], p[2], sl, 2, max_log, c_init, None) == ERR_ARGUMENT and _capi.last_error()
    # null handle and buffers: the scale among them
    assert host(None, p[0], 6 * S, p[1], p[2], S, 2, 0, -1) == ERR_ARGUMENT and "null NR modulation handle" in _capi.last_error()
    assert host(q._h, None, 6 * S, p[1], p[2], S, 2, 0, -1) == ERR_ARGUMENT
    assert host(q._h, p[0], 6 * S, None, p[2], S, 2, 0, -1) == ERR_ARGUMENT
    for fn, extra in ((host, ()), (dev, (None,))):
        assert fn(q._h, p[0], 6 * S, p[1], None, S, 2, 0, -1, *extra) == ERR_ARGUMENT and "null scale buffer" in _capi.last_error()
    # device buffers: a symbol buffer off its pair, a scale off its element; an LLR buffer off 16 bytes except for soft bits
    elem = np.dtype(real).itemsize
    assert dev(q._h, p[0], 6 * S, p[1] + elem, p[2], S, 1, 0, -1, None) == ERR_ARGUMENT and "symbol buffer is not aligned" in _capi.last_error()
    assert dev(q._h, p[0], 6 * S, p[1], p[2] + 1, S, 1, 0, -1, None) == ERR_ARGUMENT and "scale buffer is not aligned" in _capi.last_error()
    if name != "i8":
        assert dev(q._h, p[0] + elem, 6 * S, p[1], p[2], S, 1, 0, -1, None) == ERR_ARGUMENT and "LLR buffer is not aligned" in _capi.last_error()
    assert host(q._h, p[0], 6 * S, p[1], p[2], S, 0, 0, 5) == 0, "an empty batch"
    assert all_marked(sym, scale, llrs) and q.device == -1, "none of these wrote anything or made the device state"
    if L.ldpc_toolbox_device_count() == 0:
        # (the scale values are not looked at: marker bytes are as good as any)
        assert host(q._h, p[0], 6 * S, p[1], p[2], S, 2, 0, 3) == ERR_DEVICE and "no HIP device" in _capi.last_error()
        assert all_marked(llrs)
        with pytest.raises(lt.DecoderUnavailable):
            (q.demap_csi_i8 if name == "i8" else q.demodulate_csi)(np.zeros((1, S), dtype=np.complex64 if real == np.float32 else np.complex128),
                                                                   np.ones((1, S)))
    with pytest.raises(ValueError, match="one value per symbol"):
        q.demodulate_csi(np.zeros((1, S), dtype=np.complex64), np.ones((1, S + 1)))
    q.close()


@pytest.mark.parametrize("name,real", [("f32", np.float32), ("f64", np.float64)])
def test_fading_refusals_come_before_the_gpu_and_write_nothing(name, real):
    L = _capi.lib()
    S = 7
    sym, scale = marked((2, 2 * S), real), marked((2, S), real)
    host, dev = getattr(L, "ldpc_toolbox_fading_run_" + name), getattr(L, "ldpc_toolbox_fading_run_" + name + "_device")
    d = lt.Demodulator("QPSK")
    p = sym.ctypes.data, scale.ctypes.data
    for sl, sigma, block in ((S, 0.0, 3), (S, -1.0, 3), (S, float("nan"), 3), (S, float("inf"), 3), (S, 1.0, 0), (1 << 31, 1.0, 3)):
        assert host(d._h, p[0], p[1], sl, 2, sigma, block, 1, 0) == ERR_ARGUMENT and _capi.last_error(), (sl, sigma, block)
        assert dev(d._h, p[0], p[1], sl, 2, sigma, block, 1, 0, None) == ERR_ARGUMENT and _capi.last_error()
    assert host(None, p[0], p[1], S, 2, 1.0, 3, 1, 0) == ERR_ARGUMENT and "null demodulator handle" in _capi.last_error()
    assert host(d._h, None, p[1], S, 2, 1.0, 3, 1, 0) == ERR_ARGUMENT
    assert host(d._h, p[0], None, S, 2, 1.0, 3, 1, 0) == ERR_ARGUMENT and "null symbol or scale buffer" in _capi.last_error()
    elem = np.dtype(real).itemsize
    assert dev(d._h, p[0] + elem, p[1], S, 1, 1.0, 3, 1, 0, None) == ERR_ARGUMENT and "symbol buffer is not aligned" in _capi.last_error()
    assert dev(d._h, p[0], p[1] + 1, S, 1, 1.0, 3, 1, 0, None) == ERR_ARGUMENT and "scale buffer is not aligned" in _capi.last_error()
    bpsk = lt.Demodulator("BPSK")
    assert host(bpsk._h, p[0], p[1], S, 2, 1.0, 3, 1, 0) == ERR_ARGUMENT and "BPSK" in _capi.last_error()
    with pytest.raises(ValueError, match="BPSK"):
        bpsk.add_fading(np.zeros((1, S), dtype=np.complex64), 1.0, 3, 1)
    bpsk.close()
    assert host(d._h, p[0], p[1], S, 0, 1.0, 3, 1, 0) == 0, "an empty batch"
    assert all_marked(sym, scale) and d.device == -1
    if L.ldpc_toolbox_device_count() == 0:
        assert host(d._h, p[0], p[1], S, 2, 1.0, 3, 1, 0) == ERR_DEVICE and "no HIP device" in _capi.last_error()
        assert all_marked(sym, scale)
        with pytest.raises(lt.DecoderUnavailable):
            d.add_fading(np.zeros((1, S), dtype=np.complex64), 1.0, 3, 1)
    d.close()


def test_the_simulator_key_refuses_a_null_simulator():
    """(a simulator handle exists on a machine with a GPU only: tests/test_sim_fading_gpu.py has the key's range and the
    refusal of the runs)"""
    L = _capi.lib()
    assert L.ldpc_toolbox_sim_set(None, b"fading_block", 5) == -1
    if L.ldpc_toolbox_device_count() <= 0:
        assert L.ldpc_toolbox_sim_ctor(lt.code_alist("nr5g:2:2").encode(), b"Minsumf32", b"", 0, 4, 1) is None and _capi.last_error()


# ---- the restatement itself ------------------------------------------------------------------------------------------

def noisy_symbols(qm, shape, seed, real=np.float64):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, size=(shape[0], qm * shape[1]), dtype=np.uint8)
    return cr.awgn(nq.modulate(bits, qm, real=real), 0.3, seed)


@pytest.mark.parametrize("max_log", [False, True])
@pytest.mark.parametrize("qm", [2, 4, 6, 8])
def test_constant_scale_is_the_scalar_restatement_in_f64(qm, max_log):
    """every s the double 1 / (sigma * sigma): (0.5 * s) * (A_u * A_u) is the scalar restatement's K_u"""
    sigma = 0.7
    sym = noisy_symbols(qm, (3, 41), 100 + qm)
    scale = np.full(sym.shape, 1.0 / (sigma * sigma))
    for c_init in (-1, 0x1234567):
        assert same_bits(nc.demodulate_csi(sym, scale, qm, max_log, c_init), nq.demodulate(sym, sigma, qm, max_log, c_init))


@pytest.mark.parametrize("qm", [2, 4, 6, 8])
def test_constant_scale_is_the_scalar_restatement_in_exact_f32(qm):
    """sigma = 0.5: the double 1 / (sigma * sigma) = 4 is also a float"""
    sym = noisy_symbols(qm, (3, 41), 200 + qm, np.float32)
    assert sym.dtype == np.complex64
    scale = np.full(sym.shape, 4.0, dtype=np.float32)
    got = nc.demodulate_csi(sym, scale, qm, False, 77)
    assert got.dtype == np.float32 and same_bits(got, nq.demodulate(sym, 0.5, qm, False, 77))


def test_a_zero_scale_erases_the_symbol():
    sym = noisy_symbols(6, (1, 9), 5)
    for max_log in (False, True):
        assert (nc.demodulate_csi(sym, np.zeros(sym.shape), 6, max_log) == 0).all()


@pytest.mark.parametrize("seed", [1, 0x1234, (1 << 63) + 7])
def test_gains_are_positive_with_unit_mean_square(seed):
    """af^2 is Exp(1), variance 1: the mean over 2^16 draws lies within six standard errors of 1 (1.0022, 1.0025 and 1.0045
    for these seeds)"""
    frames = np.repeat(np.arange(256, dtype=np.uint64)[:, None] + np.uint64((1 << 32) - 100), 256, axis=1)
    blocks = np.repeat(np.arange(256, dtype=np.uint64)[None, :], 256, axis=0)
    af = nc.gains(seed, frames, blocks)
    assert af.dtype == np.float32 and af.size == 1 << 16 and (af > 0).all()
    mean = float((af.astype(np.float64) ** 2).mean())
    print(f"seed {seed:#x}: af in [{af.min():.4g}, {af.max():.4g}], mean af^2 {mean:.4f}")
    assert abs(mean - 1.0) < 6.0 / np.sqrt(1 << 16)


def test_fading_restatement_shares_gains_by_block_and_keys_them_apart_from_the_noise():
    sym = np.zeros((2, 12), dtype=np.complex128)
    out1, sc1 = nc.fading(sym, 0.5, 1, 9, 3)
    out5, sc5 = nc.fading(sym, 0.5, 5, 9, 3)
    outq, scq = nc.fading(sym, 0.5, 1000, 9, 3)
    assert len(np.unique(sc1[0])) == 12 and [len(np.unique(sc5[0][i:i + 5])) for i in (0, 5, 10)] == [1, 1, 1] and len(np.unique(sc5[0])) == 3
    assert len(np.unique(scq[0])) == 1 and scq[0, 0] != scq[1, 0] and scq[0, 0] == sc5[0, 0] == sc1[0, 0]
    # the noise is the AWGN channel's, scaled per symbol: x = sigma_e z with sigma_e = scale^-1/2
    plain = cr.awgn(sym, 1.0, 9, 3)
    assert np.allclose(out5 * np.sqrt(sc5), plain, rtol=1e-12)
    o32, s32 = nc.fading(sym.astype(np.complex64), 0.5, 5, 9, 3)
    assert o32.dtype == np.complex64 and s32.dtype == np.float32 and np.array_equal(s32, sc5.astype(np.float32))
