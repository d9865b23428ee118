"""CPU: the host side of the NR transport block processing (csrc/nr_transport_block.h) -- the segmentation plan against a
literal loop for every A up to 20000, the tables of x^j mod g and the rule that combines runs against bit-serial division,
the E_r of TS 38.212 5.4.2.1 -- and the C entries without a GPU.  The driver is a stand-alone program built under
ASan/UBSan; it includes that header only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ldpc_toolbox_amd as lt
import nr_transport_block_reference as tr
from ldpc_toolbox_amd import _capi
from test_nr_transport_block_reference import REFUSED, TABLE

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ERR_DEVICE, ERR_ARGUMENT = -2, -4       # include/ldpc_toolbox.h


def test_nr_transport_block_host_functions_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "nr_transport_block_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "nr_transport_block_driver.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    m = re.search(r"plans: (\d+) accepted and (\d+) refused agree with the literal loop", r.stdout)
    assert m and int(m.group(1)) + int(m.group(2)) == 40000 and int(m.group(2)) > 1000
    assert re.search(r"crc: \d{4,} split runs agree with bit-serial division", r.stdout)
    assert re.search(r"block lengths: \d{4,} cases agree with the formula and sum to G", r.stdout)
    assert "nr transport block driver: ok" in r.stdout


@pytest.mark.parametrize("bg,a", sorted(TABLE))
def test_handle_needs_no_gpu_and_reports_the_table(bg, a):
    tb = lt.NrTransportBlock(f"nr5g-tb:{bg}:{a}")
    c, k_prime, kb, zc, k, fillers = TABLE[(bg, a)]
    assert (tb.c, tb.k_prime, tb.k_b, tb.zc, tb.k, tb.fillers) == TABLE[(bg, a)]
    assert (tb.a, tb.base_graph, tb.tb_crc, tb.b, tb.cb_crc) == (a, bg, 24 if a > 3824 else 16, a + (24 if a > 3824 else 16), 24 if c > 1 else 0)
    assert tb.n == (68 if bg == 1 else 52) * zc and tb.get("device") == -1
    assert (tb.get("pass_rows"), tb.get("pass_elements"), tb.get("stage_bytes")) == (1 << 22, 1 << 30, 1 << 28)
    assert tb.code_spec == f"nr5g:{bg}:{zc}" and tb.rate_match_spec == f"nr5g:{bg}:{zc}:{fillers}"
    ref = tr.Config(bg, a)
    assert (ref.l_tb, ref.b, ref.l_cb, ref.n) == (tb.tb_crc, tb.b, tb.cb_crc, tb.n)
    with pytest.raises(KeyError):
        tb.get("e")
    # the two handles chain: the rate matcher accepts the F, and its n and k are the blocks'
    rm = lt.NrRateMatcher(tb.rate_match_spec)
    assert (rm.n, rm.k, rm.fillers) == (tb.n, tb.k, fillers)
    rm.close()
    tb.close()


@pytest.mark.parametrize("spec", [f"nr5g-tb:{bg}:{a}" for bg, a in REFUSED] +
                         ["nr5g-tb:1", "nr5g-tb:3:100", "nr5g-tb:0:100", "nr5g-tb:1:0", "nr5g-tb:1:1277993", "nr5g-tb:1:+8", "nr5g:1:384",
                          "nr5g-tb:1:8:", "nr5g-tb:1:8:0", "nr5g-tb:1: 8", "nr5g-tb:1:0x10", "nr5g-tb::8", "nr5g-tb:1:-8", "nr5g-tb:1:99999999999", "NR5G-TB:1:8",
                          "nr5g-tb", ""])
def test_constructor_refusals(spec):
    with pytest.raises(ValueError):
        lt.NrTransportBlock(spec)
    assert _capi.last_error()


def test_base_graph_at_each_boundary():
    cases = ((1, 0.95, 2), (292, 0.95, 2), (293, 0.95, 1), (293, 0.67, 2), (3824, 0.67, 2), (3824, 0.6700001, 1), (3825, 0.67, 1), (3825, 0.25, 2),
             (3825, 0.2500001, 1), (1277992, 0.25, 2), (1277992, 0.9, 1))
    for a, rate, want in cases:
        assert lt.nr_base_graph(a, rate) == want == tr.base_graph(a, rate), (a, rate)


def test_block_lengths():
    tb = lt.NrTransportBlock("nr5g-tb:2:7641")
    ref = tr.Config(2, 7641)
    for g, q in ((300, 2), (302, 2), (66, 6), (3, 1), (4, 1), (5, 1), (8 * 1000, 8), (8 * 1001, 8), (8 * 1002, 8)):
        e_lo, e_hi, c_lo = tb.block_lengths(g, q)
        want = ref.block_lengths(g, q)
        assert [e_lo] * c_lo + [e_hi] * (3 - c_lo) == want and sum(want) == g and 1 <= c_lo <= 3, (g, q)
    for g, q in ((0, 1), (300, 0), (301, 2), (4, 2), (2, 1), (1 << 31, 1)):
        with pytest.raises(ValueError):
            tb.block_lengths(g, q)
        assert _capi.last_error()
    v = C.c_uint64(0)
    L = _capi.lib()
    assert L.ldpc_toolbox_nr_tb_block_lengths(None, 300, 2, C.byref(v), C.byref(v), C.byref(v)) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_tb_block_lengths(tb._h, 300, 2, C.byref(v), None, C.byref(v)) == ERR_ARGUMENT
    tb.close()


def test_argument_errors_come_before_the_gpu_and_write_nothing():
    """also on a machine without a GPU these return ERR_ARGUMENT, never ERR_DEVICE"""
    L = _capi.lib()
    tb = lt.NrTransportBlock("nr5g-tb:2:3826")
    a, k, c = tb.a, tb.k, tb.c
    payload = np.full((2, a), 0xAB, dtype=np.uint8)
    rows = np.full((2 * c, k), 0xAB, dtype=np.uint8)
    tb_ok = np.full(2, 0xAB, dtype=np.uint8)
    cb_ok = np.full((2, c), 0xAB, dtype=np.uint8)
    P, R, T, B = payload.ctypes.data, rows.ctypes.data, tb_ok.ctypes.data, cb_ok.ctypes.data
    for kk, aa in ((k - 1, a), (k + 1, a), (k, a - 1), (k, a + 1), (0, a), (k, 0), (tb.k_prime, a)):
        assert L.ldpc_toolbox_nr_tb_segment(tb._h, R, kk, P, aa, 2) == ERR_ARGUMENT, (kk, aa)
        assert _capi.last_error()
        assert L.ldpc_toolbox_nr_tb_desegment(tb._h, P, aa, T, B, R, kk, 2) == ERR_ARGUMENT, (kk, aa)
        assert L.ldpc_toolbox_nr_tb_segment_device(tb._h, R, kk, P, aa, 2, None) == ERR_ARGUMENT
        assert L.ldpc_toolbox_nr_tb_desegment_device(tb._h, P, aa, T, B, R, kk, 2, None) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_tb_segment(None, R, k, P, a, 2) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_tb_segment(tb._h, None, k, P, a, 2) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_tb_segment(tb._h, R, k, None, a, 2) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_tb_desegment(None, P, a, T, B, R, k, 2) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_tb_desegment(tb._h, None, a, T, B, R, k, 2) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_tb_desegment(tb._h, P, a, None, B, R, k, 2) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_tb_desegment(tb._h, P, a, T, B, None, k, 2) == ERR_ARGUMENT
    g = 600
    packed = np.full(2 * g, 0xAB, dtype=np.uint8)
    out = np.full((2, g), 0xAB, dtype=np.uint8)
    for gg, q in ((0, 1), (g, 0), (g + 1, 4), (2, 2), (1 << 31, 1)):
        assert L.ldpc_toolbox_nr_tb_concatenate(tb._h, out.ctypes.data, gg, packed.ctypes.data, q, 2) == ERR_ARGUMENT, (gg, q)
        assert L.ldpc_toolbox_nr_tb_concatenate_device(tb._h, out.ctypes.data, gg, packed.ctypes.data, q, 2, None) == ERR_ARGUMENT, (gg, q)
    assert L.ldpc_toolbox_nr_tb_concatenate(None, out.ctypes.data, g, packed.ctypes.data, 2, 2) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_tb_concatenate(tb._h, None, g, packed.ctypes.data, 2, 2) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_tb_concatenate(tb._h, out.ctypes.data, g, None, 2, 2) == ERR_ARGUMENT
    for dtype, name in ((np.float32, "f32"), (np.float64, "f64")):
        rx = np.ones((2, g), dtype=dtype)
        sp = np.full(2 * g, 7.5, dtype=dtype)
        for suffix, extra in (("", ()), ("_device", (None,))):
            f = getattr(L, "ldpc_toolbox_nr_tb_split_" + name + suffix)
            for gg, q in ((0, 1), (g, 0), (g + 1, 4), (2, 2), (1 << 31, 1)):
                assert f(tb._h, sp.ctypes.data, rx.ctypes.data, gg, q, 2, *extra) == ERR_ARGUMENT, (gg, q)
            assert f(None, sp.ctypes.data, rx.ctypes.data, g, 2, 2, *extra) == ERR_ARGUMENT
            assert f(tb._h, None, rx.ctypes.data, g, 2, 2, *extra) == ERR_ARGUMENT
            assert f(tb._h, sp.ctypes.data, None, g, 2, 2, *extra) == ERR_ARGUMENT
            assert f(tb._h, sp.ctypes.data, rx.ctypes.data, g, 2, 0, *extra) == 0, "an empty batch"
        assert (sp == 7.5).all()
    assert (payload == 0xAB).all() and (rows == 0xAB).all() and (tb_ok == 0xAB).all() and (cb_ok == 0xAB).all()
    assert (packed == 0xAB).all() and (out == 0xAB).all()
    # an empty batch is no error, and needs no GPU
    assert L.ldpc_toolbox_nr_tb_segment(tb._h, R, k, P, a, 0) == 0
    assert L.ldpc_toolbox_nr_tb_desegment(tb._h, P, a, T, None, R, k, 0) == 0
    assert L.ldpc_toolbox_nr_tb_concatenate(tb._h, out.ctypes.data, g, packed.ctypes.data, 2, 0) == 0
    assert tb.get("device") == -1, "none of these made the device state"
    with pytest.raises(ValueError):
        tb.segment(np.zeros((2, a + 1), dtype=np.uint8))
    with pytest.raises(ValueError):
        tb.desegment(np.zeros((2 * c, k - 1), dtype=np.uint8))
    with pytest.raises(ValueError):
        tb.desegment(np.zeros((2 * c + 1, k), dtype=np.uint8))
    with pytest.raises(ValueError):
        tb.concatenate(np.zeros(2 * g, dtype=np.uint8), g, 7)
    with pytest.raises(ValueError):
        tb.split(np.zeros((2, g), dtype=np.float32), 7)
    tb.close()


def test_the_symbols_are_exported_and_listed():
    names = ["ldpc_toolbox_nr_tb_ctor", "ldpc_toolbox_nr_tb_dtor", "ldpc_toolbox_nr_tb_get", "ldpc_toolbox_nr_base_graph",
             "ldpc_toolbox_nr_tb_block_lengths"]
    for entry in ("segment", "desegment", "concatenate", "split_f32", "split_f64"):
        names += ["ldpc_toolbox_nr_tb_" + entry, "ldpc_toolbox_nr_tb_" + entry + "_device"]
    L = _capi.lib()
    header = open(os.path.join(ROOT, "include", "ldpc_toolbox.h")).read()
    for name in names:
        assert name in _capi.SYMBOLS and hasattr(L, name) and re.search(r"\b" + name + r"\(", header), name
    assert "PART 7" in header and "all-zero block passes every CRC" in header
    assert lt.NrTransportBlock.__name__ in lt.__all__ and "nr_base_graph" in lt.__all__


def test_without_a_gpu_the_entries_say_so():
    if _capi.lib().ldpc_toolbox_device_count() > 0:
        pytest.skip("a GPU is visible")
    tb = lt.NrTransportBlock("nr5g-tb:2:8")
    with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
        tb.segment(np.zeros((1, 8), dtype=np.uint8))
    with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
        tb.desegment(np.zeros((1, tb.k), dtype=np.uint8))
    with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
        tb.concatenate(np.zeros(24, dtype=np.uint8), 24, 2)
    with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
        tb.split(np.zeros((1, 24), dtype=np.float64), 2)
    x = np.zeros(256, dtype=np.uint8)
    assert _capi.lib().ldpc_toolbox_nr_tb_segment_device(tb._h, x.ctypes.data, tb.k, x.ctypes.data, 8, 1, None) == ERR_DEVICE
    tb.close()
