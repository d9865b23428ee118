"""CPU: the C surface of the NR modulation (include/ldpc_toolbox.h, PART 8) as far as it goes without a GPU -- constructors,
`get`, the points, every argument error (before the GPU is touched, nothing written), and ERR_DEVICE where there is none."""
import ctypes as C

import numpy as np
import pytest

import ldpc_toolbox_amd as lt
import nr_qam_reference as nq
from ldpc_toolbox_amd import _capi

ERR_DEVICE, ERR_ARGUMENT = -2, -4       # include/ldpc_toolbox.h


@pytest.mark.parametrize("qm", [2, 4, 6, 8])
def test_handle_needs_no_gpu_and_reports_the_configuration(qm):
    for spec in (qm, f"nr5g-qam:{qm}"):
        q = lt.NrQam(spec)
        assert (q.bits_per_symbol, q.get("points"), q.get("levels"), q.device, q.get("sequence_launches")) == (qm, 1 << qm, 1 << (qm // 2), -1, 0)
        with pytest.raises(KeyError):
            q.get("energy_term")
        pts = q.points
        assert pts.dtype == np.complex128 and np.array_equal(pts.view(np.uint64), nq.points(qm).view(np.uint64))
        q.close()


def test_points_entry_buffer_convention():
    L = _capi.lib()
    q = lt.NrQam(4)
    buf = np.full(40, 7.5)
    assert L.ldpc_toolbox_nr_qam_points(q._h, None, 0) == 16
    assert L.ldpc_toolbox_nr_qam_points(q._h, buf.ctypes.data, 31) == 16 and (buf == 7.5).all(), "too short: nothing written"
    assert L.ldpc_toolbox_nr_qam_points(q._h, buf.ctypes.data, 32) == 16 and (buf[32:] == 7.5).all()
    assert np.array_equal(buf[:32].view(np.complex128), nq.points(4))
    assert L.ldpc_toolbox_nr_qam_points(None, buf.ctypes.data, 32) == 0
    q.close()


@pytest.mark.parametrize("spec", ["nr5g-qam:1", "nr5g-qam:3", "nr5g-qam:10", "nr5g-qam:0", "nr5g-qam:", "nr5g-qam:4:1", "nr5g-qam:+4", "nr5g-qam: 4",
                                  "nr5g-qam:04", "16QAM", "QPSK", "nr5g:4", ""])
def test_constructor_refusals(spec):
    with pytest.raises(ValueError):
        lt.NrQam(spec)
    assert _capi.last_error()
    assert _capi.lib().ldpc_toolbox_nr_qam_ctor(None, 0) is None


def test_the_table_demapper_still_refuses_16qam():
    assert _capi.lib().ldpc_toolbox_demod_ctor(b"16QAM", 0) is None and "unknown modulation" in _capi.last_error()
    with pytest.raises(ValueError):
        lt.Demodulator(nq.points(6))      # 64 points: kDemodMaxBits stays 5


def test_argument_errors_come_before_the_gpu_and_write_nothing():
    """also on a machine without a GPU these return ERR_ARGUMENT, never ERR_DEVICE"""
    L = _capi.lib()
    q = lt.NrQam(6)
    S = 5
    bits = np.ones((2, 6 * S), dtype=np.uint8)
    for dtype, name in ((np.float32, "f32"), (np.float64, "f64")):
        sym = np.full((2, 2 * S), 7.5, dtype=dtype)
        llrs = np.full((2, 6 * S), 7.5, dtype=dtype)
        mod, demod = getattr(L, "ldpc_toolbox_nr_qam_mod_" + name), getattr(L, "ldpc_toolbox_nr_qam_demod_" + name)
        mod_d, demod_d = getattr(L, "ldpc_toolbox_nr_qam_mod_" + name + "_device"), getattr(L, "ldpc_toolbox_nr_qam_demod_" + name + "_device")
        for bl, sl, c_init in ((6 * S, S + 1, -1), (6 * S + 1, S, -1), (6 * S - 6, S, -1), (6 * (1 << 29), 1 << 29, -1), (6 * S, S, -2), (6 * S, S, 1 << 31),
                               (6 * S, S, -(1 << 40))):
            assert mod(q._h, sym.ctypes.data, sl, bits.ctypes.data, bl, 2, c_init) == ERR_ARGUMENT, (bl, sl, c_init)
            assert _capi.last_error()
            assert mod_d(q._h, sym.ctypes.data, sl, bits.ctypes.data, bl, 2, c_init, None) == ERR_ARGUMENT, (bl, sl, c_init)
        assert mod(None, sym.ctypes.data, S, bits.ctypes.data, 6 * S, 2, -1) == ERR_ARGUMENT
        assert mod(q._h, None, S, bits.ctypes.data, 6 * S, 2, -1) == ERR_ARGUMENT
        assert mod(q._h, sym.ctypes.data, S, None, 6 * S, 2, -1) == ERR_ARGUMENT
        assert (sym == 7.5).all()
        for ll, sl, sigma, c_init in ((6 * S, S + 1, 1.0, -1), (6 * S + 1, S, 1.0, -1), (6 * (1 << 29), 1 << 29, 1.0, -1), (6 * S, S, 0.0, -1),
                                      (6 * S, S, -1.0, -1), (6 * S, S, float("nan"), -1), (6 * S, S, float("inf"), -1), (6 * S, S, 1.0, -2),
                                      (6 * S, S, 1.0, 1 << 31)):
            for max_log in (0, 1):
                assert demod(q._h, llrs.ctypes.data, ll, sym.ctypes.data, sl, 2, sigma, max_log, c_init) == ERR_ARGUMENT, (ll, sl, sigma, c_init)
                assert _capi.last_error()
                assert demod_d(q._h, llrs.ctypes.data, ll, sym.ctypes.data, sl, 2, sigma, max_log, c_init, None) == ERR_ARGUMENT
        assert demod(None, llrs.ctypes.data, 6 * S, sym.ctypes.data, S, 2, 1.0, 0, -1) == ERR_ARGUMENT
        assert demod(q._h, None, 6 * S, sym.ctypes.data, S, 2, 1.0, 0, -1) == ERR_ARGUMENT
        assert demod(q._h, llrs.ctypes.data, 6 * S, None, S, 2, 1.0, 0, -1) == ERR_ARGUMENT
        # a device LLR buffer that is not aligned to 16 bytes, a symbol buffer not aligned to one pair
        assert demod_d(q._h, llrs.ctypes.data + 4, 6 * S, sym.ctypes.data, S, 1, 1.0, 0, -1, None) == ERR_ARGUMENT
        assert demod_d(q._h, llrs.ctypes.data, 6 * S, sym.ctypes.data + 4, S, 1, 1.0, 0, -1, None) == ERR_ARGUMENT
        assert mod_d(q._h, sym.ctypes.data + 4, S, bits.ctypes.data, 6 * S, 1, -1, None) == ERR_ARGUMENT
        assert (llrs == 7.5).all() and (sym == 7.5).all()
        assert mod(q._h, sym.ctypes.data, S, bits.ctypes.data, 6 * S, 0, 5) == 0, "an empty batch"
        assert demod(q._h, llrs.ctypes.data, 6 * S, sym.ctypes.data, S, 0, 1.0, 0, 5) == 0
    c = np.full(16, 0xAB, dtype=np.uint8)
    for length, c_init in ((16, -1), (16, 1 << 31), (1 << 31, 0)):
        assert L.ldpc_toolbox_nr_qam_sequence(q._h, c.ctypes.data, length, c_init) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_qam_sequence(None, c.ctypes.data, 16, 0) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_qam_sequence(q._h, None, 16, 0) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_qam_sequence(q._h, c.ctypes.data, 0, 0) == 0
    assert (c == 0xAB).all()
    assert q.device == -1, "none of these made the device state"
    q.close()


def test_without_a_gpu_the_runs_report_err_device():
    L = _capi.lib()
    q = lt.NrQam(4)
    if L.ldpc_toolbox_device_count() != 0:      # (a machine with a GPU: the same calls run; tests/test_nr_qam_gpu.py checks what they give)
        assert q.modulate(np.zeros((1, 8), dtype=np.uint8)).shape == (1, 2) and q.device >= 0
        q.close()
        return
    bits = np.zeros((1, 8), dtype=np.uint8)
    sym = np.full((1, 2), 7.5 + 7.5j, dtype=np.complex128)
    llrs = np.full((1, 8), 7.5)
    c = np.full(8, 0xAB, dtype=np.uint8)
    assert L.ldpc_toolbox_nr_qam_mod_f64(q._h, sym.ctypes.data, 2, bits.ctypes.data, 8, 1, -1) == ERR_DEVICE and "no HIP device" in _capi.last_error()
    assert L.ldpc_toolbox_nr_qam_demod_f64(q._h, llrs.ctypes.data, 8, sym.ctypes.data, 2, 1, 1.0, 0, 3) == ERR_DEVICE
    assert L.ldpc_toolbox_nr_qam_sequence(q._h, c.ctypes.data, 8, 3) == ERR_DEVICE
    assert (sym == 7.5 + 7.5j).all() and (llrs == 7.5).all() and (c == 0xAB).all()
    with pytest.raises(lt.DecoderUnavailable):
        q.modulate(bits)
    q.close()


def test_sim_set_nr_qam_refuses_a_null_simulator():
    q = lt.NrQam(4)
    assert _capi.lib().ldpc_toolbox_sim_set_nr_qam(None, q._h, 0) == -1 and _capi.last_error()
    q.close()


def test_every_declared_symbol_is_exported():
    L = _capi.lib()
    names = [s for s in _capi.SYMBOLS if "nr_qam" in s]
    assert len(names) == 14
    for s in names:
        getattr(L, s)
