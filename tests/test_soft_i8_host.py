"""CPU: csrc/soft_i8.h -- the clip, the saturating accumulate and the quantiser Q of the 8-bit soft-bit receive path -- in a
stand-alone driver built under ASan/UBSan that includes that header only; and the surface of the six entries of PART 9:
every symbol exported, declared and bound, none counted among the PART 8 names, and the refusals that need no GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import ldpc_toolbox_amd as lt
from ldpc_toolbox_amd import _capi

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ERR_ARGUMENT, ERR_UNSUPPORTED = -4, -3       # include/ldpc_toolbox.h
SOFT_SYMBOLS = ("ldpc_toolbox_decoder_decode_batch_i8", "ldpc_toolbox_decoder_decode_batch_i8_device", "ldpc_toolbox_nr_demap_i8",
                "ldpc_toolbox_nr_demap_i8_device", "ldpc_toolbox_nr_rm_recover_i8", "ldpc_toolbox_nr_rm_recover_i8_device")


def test_soft_i8_header_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "soft_i8_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "soft_i8_driver.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "clip: 256 bytes" in r.stdout and "accumulate: 65536 pairs" in r.stdout
    m = re.search(r"quantise: (\d+) values agree", r.stdout)
    assert m and int(m.group(1)) >= 4081 * 17 and "soft i8 driver: ok" in r.stdout


def test_every_new_symbol_is_exported_declared_and_bound():
    L = _capi.lib()
    header = open(os.path.join(ROOT, "include", "ldpc_toolbox.h")).read()
    assert "PART 9" in header
    for name in SOFT_SYMBOLS:
        assert name in _capi.SYMBOLS and getattr(L, name) is not None and f"int32_t {name}(" in header
        assert "nr_qam" not in name
    assert {"demap_i8", "demap_i8_device"} <= set(dir(lt.NrQam)) and {"recover_i8", "recover_i8_device"} <= set(dir(lt.NrRateMatcher))


def test_refusals_come_before_the_gpu_and_write_nothing():
    L = _capi.lib()
    rx = np.full((2, 60), 0x5A, dtype=np.int8)
    out = np.full((2, 104), 0x5B, dtype=np.int8)
    bits = np.full((2, 104), 0x5C, dtype=np.uint8)
    its = np.full(2, 0x5D, dtype=np.int32)
    post = np.full((2, 104), 0x5E, dtype=np.int16)
    sym = np.full((2, 30), 0.5 + 0.5j, dtype=np.complex64)

    def untouched():
        return (out == 0x5B).all() and (bits == 0x5C).all() and (its == 0x5D).all() and (post == 0x5E).all()

    # null handles
    assert L.ldpc_toolbox_decoder_decode_batch_i8(None, bits.ctypes.data, 104, out.ctypes.data, 104, 2, 10, its.ctypes.data, post.ctypes.data) == ERR_ARGUMENT
    assert "null decoder handle" in _capi.last_error()
    assert L.ldpc_toolbox_decoder_decode_batch_i8_device(None, bits.ctypes.data, 104, out.ctypes.data, 104, 2, 10, its.ctypes.data, None, None) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_demap_i8(None, out.ctypes.data, 60, sym.ctypes.data, 30, 2, 1.0, 0, -1) == ERR_ARGUMENT and "null" in _capi.last_error()
    assert L.ldpc_toolbox_nr_demap_i8_device(None, out.ctypes.data, 60, sym.ctypes.data, 30, 2, 1.0, 0, -1, None) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_rm_recover_i8(None, out.ctypes.data, 104, rx.ctypes.data, 60, 2, 0, 1, 127, 0) == ERR_ARGUMENT and "null" in _capi.last_error()
    assert L.ldpc_toolbox_nr_rm_recover_i8_device(None, out.ctypes.data, 104, rx.ctypes.data, 60, 2, 0, 1, 127, 0, None) == ERR_ARGUMENT
    assert untouched()
    # rate recovery: the filler soft bit, Qm, the row lengths
    rm = lt.NrRateMatcher("nr5g:2:2:4:93")
    for filler in (0, 128, -1, -127):
        assert L.ldpc_toolbox_nr_rm_recover_i8(rm._h, out.ctypes.data, 104, rx.ctypes.data, 60, 2, 0, 1, filler, 0) == ERR_ARGUMENT
        assert "filler soft bit must be 1 .. 127" in _capi.last_error()
        assert L.ldpc_toolbox_nr_rm_recover_i8_device(rm._h, out.ctypes.data, 104, rx.ctypes.data, 60, 2, 0, 1, filler, 1, None) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_rm_recover_i8(rm._h, out.ctypes.data, 104, rx.ctypes.data, 60, 2, 0, 7, 127, 0) == ERR_ARGUMENT
    assert "Qm must divide E" in _capi.last_error()
    assert L.ldpc_toolbox_nr_rm_recover_i8(rm._h, out.ctypes.data, 103, rx.ctypes.data, 60, 2, 0, 1, 127, 0) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_rm_recover_i8(rm._h, out.ctypes.data, 104, rx.ctypes.data, 60, 2, 4, 1, 127, 0) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_rm_recover_i8(rm._h, None, 104, rx.ctypes.data, 60, 2, 0, 1, 127, 0) == ERR_ARGUMENT
    assert L.ldpc_toolbox_nr_rm_recover_i8(rm._h, out.ctypes.data, 104, rx.ctypes.data, 60, 0, 0, 1, 127, 0) == 0, "an empty batch"
    with np.testing.assert_raises(ValueError):
        rm.recover_i8(rx, filler=128)
    with np.testing.assert_raises(ValueError):
        rm.recover_i8(rx.astype(np.float32))
    assert rm.get("device") == -1, "nothing made the device state"
    rm.close()
    # the demapper: the refusals of the float entry; an unaligned output is none of them
    qam = lt.NrQam(2)
    for args in ((61, 30, 1.0, -1), (60, 30, 0.0, -1), (60, 30, float("nan"), -1), (60, 30, 1.0, -2), (60, 30, 1.0, 1 << 31)):
        llrs_len, symbols_len, sigma, c_init = args
        assert L.ldpc_toolbox_nr_demap_i8(qam._h, out.ctypes.data, llrs_len, sym.ctypes.data, symbols_len, 2, sigma, 0, c_init) == ERR_ARGUMENT, args
        assert _capi.last_error()
    assert L.ldpc_toolbox_nr_demap_i8_device(qam._h, out.ctypes.data + 1, 60, sym.ctypes.data + 4, 30, 2, 1.0, 0, -1, None) == ERR_ARGUMENT
    assert "symbol buffer is not aligned" in _capi.last_error()
    assert L.ldpc_toolbox_nr_demap_i8(qam._h, None, 60, sym.ctypes.data, 30, 2, 1.0, 0, -1) == ERR_ARGUMENT
    assert qam.get("device") == -1
    qam.close()
    assert untouched()


def test_a_float_decoder_refuses_soft_bit_input_and_soft_bits_7_is_refused():
    """A decoder or simulator handle exists on a machine with a GPU only: there a float decoder returns ERR_UNSUPPORTED and
    writes nothing, a wrong row length is ERR_ARGUMENT as for the float entry, and "soft_bits" takes 8 and 32 only (8 only
    with an 8-bit implementation).  Without a GPU the constructors themselves refuse, and say why."""
    L = _capi.lib()
    alist = lt.code_alist("nr5g:2:2")
    if L.ldpc_toolbox_device_count() <= 0:
        assert L.ldpc_toolbox_decoder_ctor_alist_string_on_device(alist.encode(), b"Minsumf32", b"", 0) is None and _capi.last_error()
        assert L.ldpc_toolbox_sim_ctor(alist.encode(), b"Minsumi8", b"", 0, 4, 1) is None and _capi.last_error()
        return
    llrs = np.full((2, 104), 0x5A, dtype=np.int8)
    bits = np.full((2, 104), 0x5C, dtype=np.uint8)
    its = np.full(2, 0x5D, dtype=np.int32)
    post = np.full((2, 104), 0x5E, dtype=np.int16)
    dec = lt.LdpcDecoder(alist, "Minsumf32", device=0)
    for stream_entry in (False, True):
        fn = L.ldpc_toolbox_decoder_decode_batch_i8_device if stream_entry else L.ldpc_toolbox_decoder_decode_batch_i8
        extra = (None,) if stream_entry else ()
        assert fn(dec._h, bits.ctypes.data, 104, llrs.ctypes.data, 104, 2, 10, its.ctypes.data, post.ctypes.data, *extra) == ERR_UNSUPPORTED
        assert "8-bit" in _capi.last_error()
    assert (bits == 0x5C).all() and (its == 0x5D).all() and (post == 0x5E).all()
    dec.close()
    dec = lt.LdpcDecoder(alist, "Minsumi8", device=0)
    assert L.ldpc_toolbox_decoder_decode_batch_i8(dec._h, bits.ctypes.data, 104, llrs.ctypes.data, 103, 2, 10, its.ctypes.data, None) == ERR_ARGUMENT
    assert L.ldpc_toolbox_decoder_decode_batch_i8(dec._h, bits.ctypes.data, 105, llrs.ctypes.data, 104, 2, 10, its.ctypes.data, None) == ERR_ARGUMENT
    assert (bits == 0x5C).all() and (its == 0x5D).all()
    dec.close()
    for name, ok8 in (("Minsumi8Offset", True), ("Minsumf32", False)):
        s = lt.Simulator(alist, name, device=0, pool_size=4)
        assert s.get("soft_bits") == 32
        for bad in (7, 0, 16, 64):
            assert L.ldpc_toolbox_sim_set(s._h, b"soft_bits", bad) == -1 and "soft_bits must be 8 or 32" in _capi.last_error()
        assert (L.ldpc_toolbox_sim_set(s._h, b"soft_bits", 8) == 0) == ok8
        assert s.get("soft_bits") == (8 if ok8 else 32)
        if not ok8:
            assert "8-bit implementations" in _capi.last_error()
        s.set("soft_bits", 32)
        assert s.get("soft_bits") == 32
        s.close()
