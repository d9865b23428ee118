"""CPU: the host side of the NR link handle (csrc/nr_link.h; include/ldpc_toolbox.h, PART 11) -- the configuration a spec
gives against the restatement of TS 38.212, the specs and calls it refuses before the GPU is touched, and the C entries
without a GPU.  The driver is a stand-alone program built under ASan/UBSan; it includes that header only."""
import os
import re
import subprocess

import numpy as np
import pytest

import ldpc_toolbox_amd as lt
import nr_transport_block_reference as tr
from ldpc_toolbox_amd import _capi

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ERR_DEVICE, ERR_ARGUMENT = -2, -4       # include/ldpc_toolbox.h
LINK_SYMBOLS = ["ldpc_toolbox_nr_link_" + name for name in
                ("ctor", "dtor", "get", "set", "set_filler_llr", "transmit_f32", "transmit_f32_device", "receive_f32", "receive_f32_device",
                 "recover_f32_device", "slot_state")]
# spec -> (C, Zc, K, F, n, E_r): computed by hand from TS 38.212 5.2.2 and 5.4.2.1
TABLE = {
    "nr5g-link:2:8016:18004:4": (3, 288, 2880, 176, 14976, [6000, 6000, 6004]),
    "nr5g-link:2:4000:6004:2": (2, 208, 2080, 44, 10816, [3002, 3002]),
    "nr5g-link:2:176:600:2": (1, None, None, None, 1664, None),
}


def test_nr_link_host_functions_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "nr_link_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "nr_link_driver.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "configurations ok" in r.stdout and re.search(r"starts: \d{3,} configurations agree with the literal sum", r.stdout)
    assert re.search(r"fused recover: \d{6,} soft values agree with split and recover, bit for bit", r.stdout)
    assert "refusals ok" in r.stdout and "nr link driver: ok" in r.stdout


def test_every_symbol_is_exported_declared_and_bound():
    L = _capi.lib()
    header = open(os.path.join(ROOT, "include", "ldpc_toolbox.h")).read()
    for name in LINK_SYMBOLS:
        assert name in _capi.SYMBOLS and re.search(r"\b" + name + r"\(", header), name
        f = getattr(L, name)
        assert f.argtypes is not None and (f.restype is not None or name.endswith("_dtor")), name
    assert sorted(s for s in _capi.SYMBOLS if "nr_link" in s) == sorted(LINK_SYMBOLS)
    assert not [s for s in LINK_SYMBOLS if "nr_qam" in s]
    assert "PART 11" in header and "stays failed until a combine == 0 call" in header and "an all-zero block passes every CRC" in header
    assert lt.NrLink.__name__ in lt.__all__
    for method in ("transmit", "receive", "slot_state", "transmit_device", "receive_device", "recover_device"):
        assert callable(getattr(lt.NrLink, method))


@pytest.mark.parametrize("spec", sorted(TABLE))
def test_handle_needs_no_gpu_and_reports_the_configuration(spec):
    c, zc, k, f, n, e = TABLE[spec]
    _, bg, a, g, qm = spec.split(":")
    bg, a, g, qm = int(bg), int(a), int(g), int(qm)
    ref = tr.Config(bg, a)
    assert (ref.c, ref.n) == (c, n)
    if zc is not None:
        assert (ref.zc, ref.k, ref.fillers) == (zc, k, f) and ref.block_lengths(g, qm) == e
    link = lt.NrLink(spec, "Minsumf32", 8)
    tb = lt.NrTransportBlock(f"nr5g-tb:{bg}:{a}")
    for key in ("a", "base_graph", "tb_crc", "b", "c", "cb_crc", "k_prime", "k_b", "zc", "k", "fillers", "n"):
        assert link.get(key) == tb.get(key), key
    assert (link.c, link.zc, link.k, link.fillers, link.n) == (ref.c, ref.zc, ref.k, ref.fillers, ref.n)
    want = ref.block_lengths(g, qm)
    e_lo, e_hi, c_lo = link.block_lengths
    assert [e_lo] * c_lo + [e_hi] * (ref.c - c_lo) == want and link.block_lengths == tb.block_lengths(g, qm)
    assert (link.g, link.qm, link.layers, link.q, link.symbols, link.slots) == (g, qm, 1, qm, g // qm, 8)
    assert (link.get("max_log"), link.get("pass_elements"), link.get("stage_bytes")) == (0, 1 << 30, 1 << 28)
    assert (link.device, link.decoded_rows, link.skipped_rows) == (-1, 0, 0)
    with pytest.raises(KeyError):
        link.get("pass_rows")
    link.set("max_log", 1)
    link.set("pass_elements", 12345)
    assert (link.get("max_log"), link.get("pass_elements")) == (1, 12345)
    for key, value in (("max_log", 2), ("max_log", -1), ("pass_elements", 0), ("pass_elements", (1 << 30) + 1), ("slots", 4), ("g", 8)):
        with pytest.raises(ValueError):
            link.set(key, value)
        assert _capi.last_error()
    assert (link.get("max_log"), link.get("pass_elements"), link.slots) == (1, 12345, 8), "a refused set changes nothing"
    link.set_filler_llr(20.0)
    link.set_filler_llr(float("inf"))
    for value in (0.0, -1.0, float("nan"), float("-inf")):
        with pytest.raises(ValueError):
            link.set_filler_llr(value)
    assert link.device == -1, "none of these made the device state"
    tb.close()
    link.close()


def test_layers_enter_the_block_lengths_only():
    link = lt.NrLink("nr5g-link:2:8016:18032:4:2", "Minsumf32", 1)
    ref = tr.Config(2, 8016)
    assert (link.q, link.layers, link.qm, link.symbols) == (8, 2, 4, 4508)
    e_lo, e_hi, c_lo = link.block_lengths
    assert [e_lo] * c_lo + [e_hi] * (3 - c_lo) == ref.block_lengths(18032, 8) == [6008, 6008, 6016]
    link.close()


@pytest.mark.parametrize("spec,implementation,slots", [
    ("nr5g-link:2:8016:18004", "Minsumf32", 8), ("nr5g-link:2:8016:18004:4:1:1", "Minsumf32", 8), ("nr5g-link:2:8016:18004:4:", "Minsumf32", 8),
    ("nr5g-link:2:8016:18004:+4", "Minsumf32", 8), ("nr5g-link:2:8016:18004: 4", "Minsumf32", 8), ("NR5G-LINK:2:8016:18004:4", "Minsumf32", 8),
    ("nr5g-tb:2:8016", "Minsumf32", 8), ("", "Minsumf32", 8),
    # what the transport block constructor refuses
    ("nr5g-link:3:8016:18004:4", "Minsumf32", 8), ("nr5g-link:2:0:18004:4", "Minsumf32", 8), ("nr5g-link:2:1277993:18004:4", "Minsumf32", 8),
    # the block lengths entry: q does not divide G, G = 0, fewer symbol groups than blocks, G above 0x7fffffff
    ("nr5g-link:2:8016:18006:4", "Minsumf32", 8), ("nr5g-link:2:8016:18004:4:2", "Minsumf32", 8), ("nr5g-link:2:8016:0:4", "Minsumf32", 8),
    ("nr5g-link:2:8016:8:4", "Minsumf32", 8), ("nr5g-link:2:8016:2147483648:4", "Minsumf32", 8),
    # the modulation constructor, and the layers
    ("nr5g-link:2:8016:18004:1", "Minsumf32", 8), ("nr5g-link:2:8016:18000:3", "Minsumf32", 8), ("nr5g-link:2:8016:18000:10", "Minsumf32", 8),
    ("nr5g-link:2:8016:18004:4:0", "Minsumf32", 8), ("nr5g-link:2:8016:18000:4:5", "Minsumf32", 8),
    # the slots and the implementation
    ("nr5g-link:2:8016:18004:4", "Minsumf32", 0), ("nr5g-link:2:8016:18004:4", "Minsumf33", 8), ("nr5g-link:2:8016:18004:4", "", 8),
    ("nr5g-link:2:8016:18004:4", "Minsumf32", (1 << 31) // 3 + 1),
])
def test_constructor_refusals(spec, implementation, slots):
    with pytest.raises(ValueError):
        lt.NrLink(spec, implementation, slots)
    assert _capi.last_error()
    L = _capi.lib()
    assert L.ldpc_toolbox_nr_link_ctor(None, b"Minsumf32", 8, 0) is None and L.ldpc_toolbox_nr_link_ctor(b"nr5g-link:2:176:600:2", None, 8, 0) is None


def test_argument_errors_come_before_the_gpu_and_write_nothing():
    """also on a machine without a GPU these return ERR_ARGUMENT, never ERR_DEVICE"""
    L = _capi.lib()
    link = lt.NrLink("nr5g-link:2:8016:18004:4", "Minsumf32", 8)
    a, c, s, g = link.a, link.c, link.symbols, link.g
    payload = np.full((2, a), 0xAB, dtype=np.uint8)
    sym = np.full((2, s, 2), 7.5, dtype=np.float32)
    scale = np.full((2, s), 7.5, dtype=np.float32)
    tb_ok = np.full(2, 0xAB, dtype=np.uint8)
    cb_ok = np.full((2, c), 0xAB, dtype=np.uint8)
    its = np.full((2, c), 0x5A5A, dtype=np.int32)
    soft = np.full((2 * c, link.n), 7.5, dtype=np.float32)
    P, S, W, T, B, I = (x.ctypes.data for x in (payload, sym, scale, tb_ok, cb_ok, its))
    for suffix, extra in (("", ()), ("_device", (None,))):
        tx = getattr(L, "ldpc_toolbox_nr_link_transmit_f32" + suffix)
        rx = getattr(L, "ldpc_toolbox_nr_link_receive_f32" + suffix)
        for ss, aa, rv, c_init in ((s - 1, a, 0, -1), (s + 1, a, 0, -1), (g, a, 0, -1), (s, a - 1, 0, -1), (s, 0, 0, -1), (s, a, 4, -1), (s, a, 0, -2),
                                   (s, a, 0, 1 << 31)):
            assert tx(link._h, S, ss, P, aa, 2, rv, c_init, *extra) == ERR_ARGUMENT, (ss, aa, rv, c_init)
            assert _capi.last_error()
            assert rx(link._h, P, aa, T, B, I, S, None, ss, 2, 0.5, rv, c_init, 0, 0, 30, *extra) == ERR_ARGUMENT, (ss, aa, rv, c_init)
            assert rx(link._h, P, aa, T, B, I, S, W, ss, 2, 0.5, rv, c_init, 0, 0, 30, *extra) == ERR_ARGUMENT, (ss, aa, rv, c_init)
        assert tx(None, S, s, P, a, 2, 0, -1, *extra) == ERR_ARGUMENT
        assert tx(link._h, None, s, P, a, 2, 0, -1, *extra) == ERR_ARGUMENT and tx(link._h, S, s, None, a, 2, 0, -1, *extra) == ERR_ARGUMENT
        assert tx(link._h, S, s, P, a, 0, 0, -1, *extra) == 0, "an empty batch"
        for sigma in (0.0, -1.0, float("nan"), float("inf")):
            assert rx(link._h, P, a, T, B, I, S, None, s, 2, sigma, 0, -1, 0, 0, 30, *extra) == ERR_ARGUMENT, sigma
        assert rx(None, P, a, T, B, I, S, None, s, 2, 0.5, 0, -1, 0, 0, 30, *extra) == ERR_ARGUMENT
        assert rx(link._h, None, a, T, B, I, S, None, s, 2, 0.5, 0, -1, 0, 0, 30, *extra) == ERR_ARGUMENT
        assert rx(link._h, P, a, None, B, I, S, None, s, 2, 0.5, 0, -1, 0, 0, 30, *extra) == ERR_ARGUMENT
        assert rx(link._h, P, a, T, B, I, None, None, s, 2, 0.5, 0, -1, 0, 0, 30, *extra) == ERR_ARGUMENT
        # the slots: the range, and combining with a slot that nothing has been received into
        assert rx(link._h, P, a, T, B, I, S, None, s, 2, 0.5, 0, -1, 7, 0, 30, *extra) == ERR_ARGUMENT and "slots" in _capi.last_error()
        assert rx(link._h, P, a, T, B, I, S, None, s, 2, 0.5, 0, -1, 0xFFFFFFFF, 0, 30, *extra) == ERR_ARGUMENT
        assert rx(link._h, P, a, T, B, I, S, None, s, 2, 0.5, 2, -1, 0, 1, 30, *extra) == ERR_ARGUMENT and "never been received" in _capi.last_error()
        assert rx(link._h, P, a, T, B, I, S, None, s, 0, 0.5, 0, -1, 8, 0, 30, *extra) == 0, "an empty batch at the end of the slots"
        assert rx(link._h, P, a, T, B, I, S, None, s, 0, 0.5, 0, -1, 9, 0, 30, *extra) == ERR_ARGUMENT
    # a device symbol buffer off its (re, im) pair, a scale or iteration buffer off its element
    assert L.ldpc_toolbox_nr_link_transmit_f32_device(link._h, S + 4, s, P, a, 1, 0, -1, None) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_link_receive_f32_device(link._h, P, a, T, B, I, S + 4, None, s, 1, 0.5, 0, -1, 0, 0, 30, None) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_link_receive_f32_device(link._h, P, a, T, B, I, S, W + 2, s, 1, 0.5, 0, -1, 0, 0, 30, None) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_link_receive_f32_device(link._h, P, a, T, B, I + 2, S, None, s, 1, 0.5, 0, -1, 0, 0, 30, None) == ERR_ARGUMENT
    rec = L.ldpc_toolbox_nr_link_recover_f32_device
    X = soft.ctypes.data
    for gg, batch, rv, first, combine in ((g - 1, 2, 0, 0, 0), (s, 2, 0, 0, 0), (g, 2, 4, 0, 0), (g, 2, 0, 7, 0), (g, 2, 0, 0, 1)):
        assert rec(link._h, X, gg, batch, rv, first, combine, None) == ERR_ARGUMENT, (gg, batch, rv, first, combine)
    assert rec(None, X, g, 2, 0, 0, 0, None) == ERR_ARGUMENT and rec(link._h, None, g, 2, 0, 0, 0, None) == ERR_ARGUMENT
    assert rec(link._h, X + 2, g, 2, 0, 0, 0, None) == ERR_ARGUMENT and rec(link._h, X, g, 0, 0, 0, 0, None) == 0
    state = L.ldpc_toolbox_nr_link_slot_state
    assert state(link._h, X, B, None, 7, 2) == ERR_ARGUMENT and state(None, X, B, None, 0, 2) == ERR_ARGUMENT
    assert state(link._h, X, B, None, 8, 0) == 0 and state(link._h, None, None, None, 0, 2) == 0, "nothing asked for"
    assert (payload == 0xAB).all() and (sym == 7.5).all() and (scale == 7.5).all() and (tb_ok == 0xAB).all() and (cb_ok == 0xAB).all()
    assert (its == 0x5A5A).all() and (soft == 7.5).all()
    assert link.device == -1, "none of these made the device state"
    with pytest.raises(ValueError):
        link.transmit(np.zeros((2, a + 1), dtype=np.uint8))
    with pytest.raises(ValueError):
        link.receive(np.zeros((2, s), dtype=np.complex64))
    with pytest.raises(ValueError):
        link.receive(np.zeros((2, s), dtype=np.complex64), scale=np.ones((2, s + 1), dtype=np.float32))
    with pytest.raises(ValueError):
        link.receive(np.zeros((2, s), dtype=np.complex64), sigma=0.5, first_slot=7)
    with pytest.raises(ValueError):
        link.slot_state(first_slot=9)
    link.close()


def test_without_a_gpu_the_entries_say_so():
    if _capi.lib().ldpc_toolbox_device_count() > 0:
        pytest.skip("a GPU is visible")
    link = lt.NrLink("nr5g-link:2:176:600:2", "Minsumf32", 2)
    with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
        link.transmit(np.zeros((1, 176), dtype=np.uint8))
    with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
        link.receive(np.zeros((1, 300), dtype=np.complex64), sigma=0.5)
    with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
        link.slot_state()
    x = np.zeros(4096, dtype=np.float32)
    L = _capi.lib()
    assert L.ldpc_toolbox_nr_link_transmit_f32_device(link._h, x.ctypes.data, 300, x.ctypes.data, 176, 1, 0, -1, None) == ERR_DEVICE
    assert L.ldpc_toolbox_nr_link_recover_f32_device(link._h, x.ctypes.data, 600, 1, 0, 0, 0, None) == ERR_DEVICE
    assert link.device == -1
    link.close()
