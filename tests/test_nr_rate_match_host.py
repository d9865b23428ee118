"""CPU: the rate matcher's host side (csrc/nr_rate_match.h) -- the closed forms of the selection rank, both mapping
directions and the interleaver against a literal loop of TS 38.212 5.4.2 on a grid of small configurations, the k0 tables,
the largest E and every refusal of the validators -- and the C entries without a GPU.  The driver is a stand-alone program
built under ASan/UBSan; it includes that header only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ldpc_toolbox_amd as lt
from ldpc_toolbox_amd import _capi

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ERR_DEVICE, ERR_ARGUMENT = -2, -4       # include/ldpc_toolbox.h


def test_nr_rate_match_host_functions_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "nr_rate_match_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "nr_rate_match_driver.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "grid: 6400 cases agree with the literal loop" in r.stdout
    assert "k0 tables ok" in r.stdout and "refusals ok" in r.stdout and "large E ok" in r.stdout
    assert "nr rate match driver: ok" in r.stdout


def test_handle_needs_no_gpu_and_reports_the_configuration():
    rm = lt.NrRateMatcher("nr5g:1:384")
    assert (rm.n, rm.k, rm.zc, rm.base_graph, rm.fillers, rm.n_cb, rm.buffer_len) == (26112, 8448, 384, 1, 0, 25344, 25344)
    assert [rm.k0(rv) for rv in range(4)] == [0, 6528, 12672, 21504] and rm.get("device") == -1
    assert (rm.get("pass_elements"), rm.get("stage_bytes")) == (1 << 30, 1 << 28)
    with pytest.raises(KeyError):
        rm.get("k0_4")
    rm.close()
    rm = lt.NrRateMatcher("nr5g:2:2:4:56")
    assert (rm.n, rm.k, rm.fillers, rm.n_cb, rm.buffer_len, rm.k0(1)) == (104, 20, 4, 56, 52, 14)
    rm.close()
    rm = lt.NrRateMatcher("nr5g:1:384:0:16896", device=None)
    assert [rm.k0(rv) for rv in range(4)] == [0, 4224, 8448, 14208]
    rm.close()


@pytest.mark.parametrize("spec", ["nr5g:1", "nr5g:3:384", "nr5g:1:17", "nr5g:1:1", "nr5g:1:384:8000", "nr5g:1:384:0:0", "nr5g:1:384:0:25345",
                                  "nr5g:2:2:16:16", "nr5g:1:384:", "nr5g:1:384:0:1:2", "nr5g:1:+384", "nr5g:1:384:-1", "dvbs2:R1_2",
                                  "nr5g:1: 384", "nr5g:1:0x10", ""])
def test_constructor_refusals(spec):
    with pytest.raises(ValueError):
        lt.NrRateMatcher(spec)
    assert _capi.last_error()


def test_argument_errors_come_before_the_gpu_and_write_nothing():
    """also on a machine without a GPU these return ERR_ARGUMENT, never ERR_DEVICE"""
    L = _capi.lib()
    rm = lt.NrRateMatcher("nr5g:2:2")
    n = rm.n
    cws = np.zeros((2, n), dtype=np.uint8)
    out = np.full((2, 64), 0xAB, dtype=np.uint8)
    for e, nn, rv, qm in ((0, n, 0, 1), (24, n - 1, 0, 1), (24, n, 4, 1), (24, n, 0, 0), (24, n, 0, 9), (25, n, 0, 2), (1 << 31, n, 0, 1)):
        assert L.ldpc_toolbox_nr_rm_match(rm._h, out.ctypes.data, e, cws.ctypes.data, nn, 2, rv, qm) == ERR_ARGUMENT, (e, nn, rv, qm)
        assert _capi.last_error()
    assert L.ldpc_toolbox_nr_rm_match(None, out.ctypes.data, 24, cws.ctypes.data, n, 2, 0, 1) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_rm_match(rm._h, None, 24, cws.ctypes.data, n, 2, 0, 1) == ERR_ARGUMENT
    assert (out == 0xAB).all()
    for dtype, name in ((np.float32, "f32"), (np.float64, "f64")):
        f = getattr(L, "ldpc_toolbox_nr_rm_recover_" + name)
        rx = np.ones((2, 24), dtype=dtype)
        llrs = np.full((2, n), 7.5, dtype=dtype)
        for e, nn, rv, qm, filler in ((24, n, 0, 1, 0.0), (24, n, 0, 1, -3.0), (24, n, 0, 1, float("nan")), (24, n, 0, 1, float("-inf")),
                                      (24, n + 1, 0, 1, 1.0), (24, n, 5, 1, 1.0), (24, n, 0, 5, 1.0), (0, n, 0, 1, 1.0)):
            assert f(rm._h, llrs.ctypes.data, nn, rx.ctypes.data, e, 2, rv, qm, filler, 0) == ERR_ARGUMENT, (e, nn, rv, qm, filler)
        assert f(None, llrs.ctypes.data, n, rx.ctypes.data, 24, 2, 0, 1, 1.0, 0) == ERR_ARGUMENT
        assert f(rm._h, llrs.ctypes.data, n, None, 24, 2, 0, 1, 1.0, 0) == ERR_ARGUMENT
        assert (llrs == 7.5).all()
        assert f(rm._h, llrs.ctypes.data, n, rx.ctypes.data, 24, 0, 0, 1, float("inf"), 1) == 0, "an empty batch"
    assert L.ldpc_toolbox_nr_rm_match(rm._h, out.ctypes.data, 24, cws.ctypes.data, n, 0, 0, 1) == 0
    assert rm.get("device") == -1, "none of these made the device state"
    with pytest.raises(ValueError):
        rm.match(cws, 25, qm=2)
    with pytest.raises(ValueError):
        rm.recover(np.ones((2, 24), dtype=np.float32), into=np.zeros((2, n), dtype=np.float64))
    rm.close()


def test_without_a_gpu_the_entries_say_so():
    if _capi.lib().ldpc_toolbox_device_count() > 0:
        pytest.skip("a GPU is visible")
    rm = lt.NrRateMatcher("nr5g:2:2")
    with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
        rm.match(np.zeros((1, rm.n), dtype=np.uint8), 24)
    with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
        rm.recover(np.zeros((1, 24), dtype=np.float32))
    L = _capi.lib()
    x = np.zeros(256, dtype=np.float32)
    assert L.ldpc_toolbox_nr_rm_recover_f32_device(rm._h, x.ctypes.data, rm.n, x.ctypes.data, 24, 1, 0, 1, 1.0, 0, None) == ERR_DEVICE
    rm.close()
