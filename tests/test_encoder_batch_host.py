"""CPU: the C ABI surface of the batched GPU encoder -- exported symbols, ldpc_toolbox_encoder_get, the argument
errors (found before any GPU is touched) and the absence of a CPU fallback.  The kernels themselves are checked in
tests/test_gpu_encoder.py."""
import ctypes
import json
import os

import numpy as np
import pytest

import ldpc_toolbox_amd as lt
from ldpc_toolbox_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")))

ERR_DEVICE, ERR_ARGUMENT = -2, -4       # include/ldpc_toolbox.h
NEW_SYMBOLS = ("ldpc_toolbox_encoder_ctor_alist_string_on_device", "ldpc_toolbox_encoder_encode_batch",
               "ldpc_toolbox_encoder_encode_batch_device", "ldpc_toolbox_encoder_get")


def _get(handle, key):
    v = ctypes.c_int64(12345)
    rc = _capi.lib().ldpc_toolbox_encoder_get(handle, key.encode(), ctypes.byref(v))
    return rc, int(v.value)


def test_new_symbols_are_exported_and_listed():
    L = ctypes.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "ldpc_toolbox.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in _capi.SYMBOLS, name
        assert name + "(" in header, name


@pytest.mark.parametrize("alist_of, pattern, expect", [
    (lambda: KATS["encoder_dense"]["alist"], "", None),
    (lambda: KATS["encoder_staircase"]["alist"], "", None),
    (lambda: lt.code_alist("dvbs2:R1_2short"), "", dict(k=7200, n=16200, output_len=16200, staircase=1)),
    (lambda: lt.code_alist("ar4ja:1/2:1024"), "1,1,1,1,0", dict(k=1024, n=2560, output_len=2048, staircase=0)),
], ids=["kat_dense", "kat_staircase", "dvbs2_short", "ar4ja_punctured"])
def test_encoder_get(alist_of, pattern, expect):
    alist = alist_of()
    if expect is None:      # the reference's own matrices: sizes from the alist header and the known-answer pairs
        n, m = (int(x) for x in alist.split()[:2])
        kat = KATS["encoder_dense"] if alist == KATS["encoder_dense"]["alist"] else KATS["encoder_staircase"]
        assert len(kat["pairs"][0][0]) == n - m and len(kat["pairs"][0][1]) == n
        expect = dict(k=n - m, n=n, output_len=n, staircase=int(kat is KATS["encoder_staircase"]))
    enc = lt.Encoder(alist, pattern)
    for key, value in expect.items():
        assert _get(enc._h, key) == (0, value), key
    assert (enc.k, enc.n, enc.output_len, enc.staircase) == (expect["k"], expect["n"], expect["output_len"], bool(expect["staircase"]))
    # every one of these messages fits in LDS at 32 frames per word: form 0, and -1 for a code that is not a staircase
    assert _get(enc._h, "staircase_form") == (0, 0 if expect["staircase"] else -1)
    assert enc.staircase_form == (0 if expect["staircase"] else -1)
    # a handle from the plain constructor has no device state
    assert _get(enc._h, "device") == (0, -1) and enc.device == -1
    rc, v = _get(enc._h, "no_such_key")
    assert rc == -1 and v == 12345
    assert _capi.lib().ldpc_toolbox_encoder_get(None, b"k", ctypes.byref(ctypes.c_int64(0))) == -1


@pytest.mark.parametrize("entry", ["host", "device"])
def test_argument_errors_need_no_gpu(entry):
    L = _capi.lib()
    enc = lt.Encoder(lt.code_alist("ar4ja:1/2:1024"), "1,1,1,1,0")
    k, out_len, B = enc.k, enc.output_len, 3
    msgs = np.zeros((B, k), dtype=np.uint8)

    def call(handle, olen, ilen):
        out = np.full((B, 4096), 0xA5, dtype=np.uint8)
        if entry == "host":
            rc = L.ldpc_toolbox_encoder_encode_batch(handle, out.ctypes.data, olen, msgs.ctypes.data, ilen, B)
        else:
            rc = L.ldpc_toolbox_encoder_encode_batch_device(handle, out.ctypes.data, olen, msgs.ctypes.data, ilen, B, None)
        return rc, _capi.last_error(), out

    for handle, olen, ilen in ((None, out_len, k), (enc._h, out_len, k - 1), (enc._h, out_len, k + 1),
                               (enc._h, enc.n, k), (enc._h, out_len - 1, k), (enc._h, 0, k)):
        rc, msg, out = call(handle, olen, ilen)
        assert rc == ERR_ARGUMENT, (handle, olen, ilen, rc)
        assert msg, "an argument error leaves a message"
        assert (out == 0xA5).all(), "an argument error writes nothing"
    # no device state was made on the way
    assert enc.device == -1
    # a pattern that does not divide n fails every batched call the same way (2560 % 3 != 0)
    bad = lt.Encoder(lt.code_alist("ar4ja:1/2:1024"), "1,1,0")
    for olen in (2560, 1706, 1707, 0):
        rc, msg, out = call(bad._h, olen, k)
        assert rc == ERR_ARGUMENT and msg and (out == 0xA5).all(), olen
    # the on-device constructor refuses it outright, on any machine
    assert not L.ldpc_toolbox_encoder_ctor_alist_string_on_device(lt.code_alist("ar4ja:1/2:1024").encode(), b"1,1,0", 0)
    assert _capi.last_error()


def test_batch_zero_returns_zero_without_a_gpu():
    enc = lt.Encoder(KATS["encoder_staircase"]["alist"])
    assert _capi.lib().ldpc_toolbox_encoder_encode_batch(enc._h, None, enc.output_len, None, enc.k, 0) == 0
    assert enc.encode_batch(np.zeros((0, enc.k), dtype=np.uint8)).shape == (0, enc.n)
    assert enc.device == -1


def test_no_cpu_fallback_in_the_batched_entries():
    """without a GPU a well-formed batched call fails loudly, writes nothing, and leaves the scalar encoder usable"""
    L = _capi.lib()
    if L.ldpc_toolbox_device_count() > 0:
        pytest.skip("a GPU is visible")
    kat = KATS["encoder_dense"]
    enc = lt.Encoder(kat["alist"])
    msgs = np.array([p[0] for p in kat["pairs"]], dtype=np.uint8)
    out = np.full((len(msgs), enc.n), 0xA5, dtype=np.uint8)
    rc = L.ldpc_toolbox_encoder_encode_batch(enc._h, out.ctypes.data, enc.n, msgs.ctypes.data, enc.k, len(msgs))
    assert rc == ERR_DEVICE and "no HIP device" in _capi.last_error()
    assert (out == 0xA5).all()
    with pytest.raises(RuntimeError, match="no HIP device"):
        enc.encode_batch(msgs)
    assert enc.device == -1
    with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
        lt.Encoder(kat["alist"], device=0)
    for msg, cw in kat["pairs"]:
        assert enc.encode(np.array(msg, dtype=np.uint8), enc.n).tolist() == cw
