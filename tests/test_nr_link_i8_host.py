"""CPU: the host side of the 8-bit mode of the NR link handle (include/ldpc_toolbox.h, PART 12; csrc/nr_link.h) -- the key
"soft_bits" and what its setter refuses, the derived "soft_bytes", the two entries that take and give 8-bit soft rows, and
what they refuse before the GPU is touched.  The driver is a stand-alone program built under ASan/UBSan; it includes
csrc/nr_link.h only."""
import os
import re
import subprocess

import numpy as np
import pytest

import ldpc_toolbox_amd as lt
import nr_transport_block_reference as tr
from ldpc_toolbox_amd import _capi

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ERR_DEVICE, ERR_UNSUPPORTED, ERR_ARGUMENT = -2, -3, -4       # include/ldpc_toolbox.h
NEW_SYMBOLS = ["ldpc_toolbox_nr_harq_slots_recover_i8_device", "ldpc_toolbox_nr_harq_slots_state_i8"]
SPEC = "nr5g-link:2:8016:18010:2"


def test_nr_link_i8_host_functions_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "nr_link_i8_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "nr_link_i8_driver.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert re.search(r"dword passes: \d{4,} values agree with the literal search", r.stdout) and "mode ok" in r.stdout
    assert re.search(r"fused recover i8: \d{6,} soft bits agree with split and recover, byte for byte", r.stdout)
    assert "nr link i8 driver: ok" in r.stdout


def test_the_two_entries_are_declared_exported_and_bound():
    L = _capi.lib()
    header = open(os.path.join(ROOT, "include", "ldpc_toolbox.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and re.search(r"\b" + name + r"\(", header), name
        f = getattr(L, name)
        assert f.argtypes is not None and len(f.argtypes) == (8 if "recover" in name else 6) and f.restype is not None, name
        assert "nr_link" not in name
    assert "PART 12" in header and header.index("PART 12") > header.index("PART 11")
    for method in ("recover_i8_device", "slot_state"):
        assert callable(getattr(lt.NrLink, method))
    assert isinstance(lt.NrLink.soft_bits, property) and isinstance(lt.NrLink.soft_bytes, property)


def test_soft_bits_and_soft_bytes_need_no_gpu():
    ref = tr.Config(2, 8016)
    rows = ref.c * 8 * ref.n
    assert (ref.c, ref.n) == (3, 14976)
    link = lt.NrLink(SPEC, "Minsumi8", 8)
    assert (link.soft_bits, link.get("soft_bits"), link.soft_bytes) == (32, 32, 4 * rows), "the default is the float mode"
    link.set("soft_bits", 32)
    link.set("soft_bits", 8)
    assert (link.soft_bits, link.soft_bytes, link.get("soft_bytes")) == (8, rows, rows)
    link.set("soft_bits", 8)
    link.set("soft_bits", 32)
    assert (link.soft_bits, link.soft_bytes) == (32, 4 * rows)
    assert link.device == -1, "none of these made the device state"
    link.close()
    link = lt.NrLink(SPEC, "Minsumi8", 8, soft_bits=8)
    assert (link.soft_bits, link.soft_bytes, link.device) == (8, rows, -1)
    link.close()
    link = lt.NrLink("nr5g-link:2:12:122:2", "Minstarapproxi8", 5, device=None, soft_bits=8)
    assert (link.n, link.soft_bits, link.soft_bytes) == (260, 8, 5 * 260)
    link.close()
    link = lt.NrLink(SPEC, "Minsumf32", 8)
    assert (link.soft_bits, link.soft_bytes) == (32, 4 * rows)
    link.close()


def test_the_setters_refuse_with_a_message_and_change_nothing():
    link = lt.NrLink(SPEC, "Minsumi8", 8)
    for value in (16, 0, 7, -8, 64):
        with pytest.raises(ValueError, match="8 or 32"):
            link.set("soft_bits", value)
        assert _capi.last_error() and link.soft_bits == 32
    link.set_filler_llr(0.05)                                # fine on a float handle; Q(0.05) = round(0.4) = 0
    with pytest.raises(ValueError, match="quantises"):
        link.set("soft_bits", 8)
    assert _capi.last_error() and (link.soft_bits, link.soft_bytes) == (32, 4 * 3 * 8 * 14976)
    link.set_filler_llr(20.0)
    link.set("soft_bits", 8)
    with pytest.raises(ValueError, match="quantises"):
        link.set_filler_llr(0.05)
    assert _capi.last_error()
    for value in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            link.set_filler_llr(value)
    link.set_filler_llr(0.0625)                              # Q = round-half-away(0.5) = 1
    link.set_filler_llr(float("inf"))
    assert link.soft_bits == 8 and link.device == -1
    link.close()
    # an implementation that is not one of the 8-bit names: through the setter and through the constructor
    link = lt.NrLink(SPEC, "Minsumf32", 8)
    with pytest.raises(ValueError, match="8-bit implementations"):
        link.set("soft_bits", 8)
    assert _capi.last_error() and (link.soft_bits, link.soft_bytes) == (32, 4 * 3 * 8 * 14976)
    link.close()
    for name in ("Minsumf32", "Phif64", "Minsumf32Norm"):
        with pytest.raises(ValueError):
            lt.NrLink(SPEC, name, 8, soft_bits=8)
    with pytest.raises(ValueError):
        lt.NrLink(SPEC, "Minsumi8", 8, soft_bits=16)
    for name in ("Minsumi8", "Minstarapproxi8", "Minsumi8Offset", "HLAminstari8PartialHardLimit", "Aminstari8Jones"):
        link = lt.NrLink(SPEC, name, 2, soft_bits=8)
        assert link.soft_bits == 8
        link.close()


def test_argument_errors_of_the_new_entries_come_before_the_gpu_and_write_nothing():
    L = _capi.lib()
    rec, state = L.ldpc_toolbox_nr_harq_slots_recover_i8_device, L.ldpc_toolbox_nr_harq_slots_state_i8
    rec_f32, state_f32 = L.ldpc_toolbox_nr_link_recover_f32_device, L.ldpc_toolbox_nr_link_slot_state
    link = lt.NrLink(SPEC, "Minsumi8", 8, soft_bits=8)
    c, g, n, k = link.c, link.g, link.n, link.k
    rx = np.full((2, g), 0x5A, dtype=np.int8)
    soft = np.full((2 * c, n), 0x5A, dtype=np.int8)
    done = np.full((2, c), 0xAB, dtype=np.uint8)
    rows = np.full((2 * c, k), 0xAB, dtype=np.uint8)
    X, S, D, R = (x.ctypes.data for x in (rx, soft, done, rows))
    for gg, batch, rv, first, combine, what in ((g - 1, 2, 0, 0, 0, "G"), (g // 2, 2, 0, 0, 0, "G"), (g, 2, 4, 0, 0, "rv"), (g, 2, 0, 7, 0, "slots"),
                                                (g, 2, 0, 0xFFFFFFFF, 0, "slots"), (g, 9, 0, 0, 0, "slots"), (g, 2, 0, 0, 1, "never been received")):
        assert rec(link._h, X, gg, batch, rv, first, combine, None) == ERR_ARGUMENT, (gg, batch, rv, first, combine)
        assert what in _capi.last_error(), _capi.last_error()
    assert rec(None, X, g, 2, 0, 0, 0, None) == ERR_ARGUMENT and rec(link._h, None, g, 2, 0, 0, 0, None) == ERR_ARGUMENT
    assert rec(link._h, X, g, 0, 0, 0, 0, None) == 0 and rec(link._h, X, g, 0, 0, 8, 0, None) == 0, "an empty batch"
    assert state(link._h, S, D, R, 7, 2) == ERR_ARGUMENT and "slots" in _capi.last_error()
    assert state(None, S, D, R, 0, 2) == ERR_ARGUMENT
    assert state(link._h, S, D, R, 8, 0) == 0 and state(link._h, None, None, None, 0, 2) == 0, "nothing asked for"
    # the entries of the other mode: float soft rows on an 8-bit handle
    fl = np.full((2 * c, n), 7.5, dtype=np.float32)
    assert rec_f32(link._h, fl.ctypes.data, g, 2, 0, 0, 0, None) == ERR_UNSUPPORTED and "soft_bits 8" in _capi.last_error()
    assert state_f32(link._h, fl.ctypes.data, D, R, 0, 2) == ERR_UNSUPPORTED and _capi.last_error()
    assert state_f32(link._h, fl.ctypes.data, None, None, 7, 2) == ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match="soft_bits 8"):
        link.recover_device(fl.ctypes.data, 2)
    assert state_f32(link._h, None, None, None, 0, 2) == 0 and state_f32(link._h, None, D, R, 7, 2) == ERR_ARGUMENT
    assert link.device == -1, "none of these made the device state"
    link.close()
    # ... and 8-bit soft rows on a float handle, whatever its implementation
    for name in ("Minsumi8", "Minsumf32"):
        link = lt.NrLink(SPEC, name, 8)
        assert rec(link._h, X, g, 2, 0, 0, 0, None) == ERR_UNSUPPORTED and "soft_bits 32" in _capi.last_error()
        assert rec(link._h, X, g - 1, 2, 4, 7, 1, None) == ERR_UNSUPPORTED
        assert state(link._h, S, D, R, 0, 2) == ERR_UNSUPPORTED and _capi.last_error()
        assert state(link._h, None, None, None, 0, 2) == 0 and state(link._h, None, D, R, 7, 2) == ERR_ARGUMENT
        with pytest.raises(RuntimeError, match="soft_bits 32"):
            link.recover_i8_device(X, 2)
        assert link.device == -1
        link.close()
    assert (rx == 0x5A).all() and (soft == 0x5A).all() and (done == 0xAB).all() and (rows == 0xAB).all() and (fl == 7.5).all()


def test_without_a_gpu_the_new_entries_say_so():
    if _capi.lib().ldpc_toolbox_device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _capi.lib()
    link = lt.NrLink("nr5g-link:2:176:600:2", "Minsumi8", 2, soft_bits=8)
    x = np.zeros(4096, dtype=np.int8)
    assert L.ldpc_toolbox_nr_harq_slots_recover_i8_device(link._h, x.ctypes.data, 600, 1, 0, 0, 0, None) == ERR_DEVICE
    assert "no HIP device" in _capi.last_error()
    assert L.ldpc_toolbox_nr_harq_slots_state_i8(link._h, x.ctypes.data, None, None, 0, 1) == ERR_DEVICE
    assert L.ldpc_toolbox_nr_harq_slots_state_i8(link._h, None, x.ctypes.data, None, 0, 1) == ERR_DEVICE
    with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
        link.slot_state()
    with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
        link.recover_i8_device(x.ctypes.data, 1)
    with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
        link.receive(np.zeros((1, 300), dtype=np.complex64), sigma=0.5)
    assert (link.device, link.soft_bits) == (-1, 8) and not x.any()
    link.set("soft_bits", 32)                               # the device state still does not exist
    assert link.soft_bits == 32
    link.close()
