"""CPU: the BCH entries of the C ABI without a GPU -- constructors, `get` and `generator` work, every refusal of a spec
leaves a message, every argument error returns before the device is touched with nothing written, and a well-formed run
call fails with LDPC_TOOLBOX_ERR_DEVICE (there is no CPU path)."""
import ctypes

import numpy as np
import pytest

import bch_reference as br
import ldpc_toolbox_amd as lt
from ldpc_toolbox_amd import _capi

ERR_DEVICE, ERR_ARGUMENT = -2, -4       # include/ldpc_toolbox.h


def test_constructor_get_and_generator():
    code = lt.BchCode("dvbs2:R1_2short")
    ref = br.Code.from_spec("dvbs2:R1_2short")
    assert (code.n, code.k, code.t, code.m, code.parity) == (7200, 7032, 12, 14, 168) == (ref.n, ref.k, ref.t, ref.m, ref.parity)
    assert code.get("primitive") == 0x402B and code.get("device") == -1 and code.get("pass_frames") >= 1 and code.get("stage_frames") == 2 ** 28 // 7200
    g = code.generator()
    assert g.dtype == np.uint8 and len(g) == 169 and sum(int(b) << i for i, b in enumerate(g)) == ref.g
    with pytest.raises(KeyError):
        code.get("no_such_key")
    L = _capi.lib()
    assert L.ldpc_toolbox_bch_get(None, b"n", ctypes.byref(ctypes.c_int64(0))) == -1
    # a buffer that is too short is not written; the length needed is still returned
    short = np.full(10, 0xA5, dtype=np.uint8)
    assert L.ldpc_toolbox_bch_generator(code._h, short.ctypes.data, 10) == 169 and (short == 0xA5).all()
    code.close()
    code.close()


@pytest.mark.parametrize("name", sorted(br.DVBS2))
def test_every_dvbs2_name(name):
    code = lt.BchCode("dvbs2:" + name)
    n, k, t = br.DVBS2[name]
    assert (code.n, code.k, code.t, code.m) == (n, k, t, 14 if name.endswith("short") else 16)
    if name != "R3_4short":  # (the library's LDPC code of that name has k = 1080: see include/ldpc_toolbox.h)
        columns, rows = (int(x) for x in lt.code_alist("dvbs2:" + name).split()[:2])
        assert columns - rows == n, "the BCH word is the LDPC code's message"


@pytest.mark.parametrize("spec,g,k", [("bch:5:25:3:31", 0x8faf, 16), ("bch:6:43:3:63", 0x782cf, 45), ("bch:6:43:2:40", 0x1539, 28),
                                      ("bch:4:13:7:15", None, 1)])
def test_general_specs(spec, g, k):
    code = lt.BchCode(spec)
    ref = br.Code.from_spec(spec)
    assert code.k == k == ref.k and sum(int(b) << i for i, b in enumerate(code.generator())) == ref.g
    if g is not None:
        assert ref.g == g


@pytest.mark.parametrize("spec", ["", "bch", "bch:5:25:3", "bch:5:25:3:31:1", "bch:3:b:1:7", "bch:17:2002d:1:100", "bch:5:45:3:31",
                                  "bch:5:3f:3:31", "bch:5:21:3:31", "bch:4:13:8:15", "bch:5:25:0:31", "bch:5:25:3:32",
                                  "bch:5:25:3:15", "bch:16:1002D:13:65535", "bch:5:2g:3:31", "bch:5:25:3:-1", "dvbs2:R7_8", "c2"])
def test_refused_specs(spec):
    assert not _capi.lib().ldpc_toolbox_bch_ctor(spec.encode(), 0)
    assert _capi.last_error()
    with pytest.raises(ValueError):
        lt.BchCode(spec)


def test_null_spec():
    assert not _capi.lib().ldpc_toolbox_bch_ctor(None, 0) and _capi.last_error()


@pytest.mark.parametrize("entry", ["host", "device"])
def test_argument_errors_need_no_gpu(entry):
    L = _capi.lib()
    code = lt.BchCode("bch:6:43:2:40")
    n, k, B = code.n, code.k, 3
    data = np.zeros((B, 64), dtype=np.uint8)
    errors = np.full(B, 77, dtype=np.int32)

    def call(decode, handle, olen, ilen):
        out = np.full((B, 64), 0xA5, dtype=np.uint8)
        stream = () if entry == "host" else (None,)
        if decode:
            fn = L.ldpc_toolbox_bch_decode_batch if entry == "host" else L.ldpc_toolbox_bch_decode_batch_device
            rc = fn(handle, out.ctypes.data, olen, data.ctypes.data, ilen, B, errors.ctypes.data, *stream)
        else:
            fn = L.ldpc_toolbox_bch_encode_batch if entry == "host" else L.ldpc_toolbox_bch_encode_batch_device
            rc = fn(handle, out.ctypes.data, olen, data.ctypes.data, ilen, B, *stream)
        return rc, _capi.last_error(), out

    cases = [(False, None, n, k), (False, code._h, n, k - 1), (False, code._h, n, n), (False, code._h, k, k), (False, code._h, n - 1, k),
             (False, code._h, 0, k), (True, None, k, n), (True, code._h, k, k), (True, code._h, k, n + 1), (True, code._h, k - 1, n),
             (True, code._h, n - 1, n), (True, code._h, 0, n), (True, code._h, n + 1, n)]
    for decode, handle, olen, ilen in cases:
        rc, msg, out = call(decode, handle, olen, ilen)
        assert rc == ERR_ARGUMENT, (decode, olen, ilen, rc)
        assert msg, "an argument error leaves a message"
        assert (out == 0xA5).all() and (errors == 77).all(), "an argument error writes nothing"
    assert code.get("device") == -1, "no device state was made on the way"
    # null buffers with a batch
    fn = L.ldpc_toolbox_bch_encode_batch
    assert fn(code._h, None, n, data.ctypes.data, k, B) == ERR_ARGUMENT and fn(code._h, data.ctypes.data, n, None, k, B) == ERR_ARGUMENT
    assert code.get("device") == -1


def test_batch_zero_returns_zero_without_a_gpu():
    L = _capi.lib()
    code = lt.BchCode("bch:6:43:2:40")
    assert L.ldpc_toolbox_bch_encode_batch(code._h, None, code.n, None, code.k, 0) == 0
    assert L.ldpc_toolbox_bch_decode_batch(code._h, None, code.k, None, code.n, 0, None) == 0
    assert L.ldpc_toolbox_bch_decode_batch_device(code._h, None, code.n, None, code.n, 0, None, None) == 0
    out, errors = code.decode(np.zeros((0, code.n), dtype=np.uint8))
    assert out.shape == (0, code.k) and errors.shape == (0,)
    assert code.encode(np.zeros((0, code.k), dtype=np.uint8)).shape == (0, code.n)
    assert code.get("device") == -1


def test_no_cpu_path():
    """without a GPU a well-formed call fails loudly and writes nothing"""
    L = _capi.lib()
    if L.ldpc_toolbox_device_count() > 0:
        pytest.skip("a GPU is visible")
    code = lt.BchCode("bch:6:43:2:40")
    msgs = np.ones((2, code.k), dtype=np.uint8)
    out = np.full((2, code.n), 0xA5, dtype=np.uint8)
    errors = np.full(2, 77, dtype=np.int32)
    rc = L.ldpc_toolbox_bch_encode_batch(code._h, out.ctypes.data, code.n, msgs.ctypes.data, code.k, 2)
    assert rc == ERR_DEVICE and "no HIP device" in _capi.last_error() and (out == 0xA5).all()
    rc = L.ldpc_toolbox_bch_decode_batch(code._h, out.ctypes.data, code.n, out.ctypes.data, code.n, 2, errors.ctypes.data)
    assert rc == ERR_DEVICE and "no HIP device" in _capi.last_error() and (out == 0xA5).all() and (errors == 77).all()
    with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
        code.encode(msgs)
    with pytest.raises(lt.DecoderUnavailable, match="no HIP device"):
        code.decode(np.zeros((2, code.n), dtype=np.uint8))
    assert code.get("device") == -1
