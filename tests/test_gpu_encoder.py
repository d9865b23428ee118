"""GPU: the batched encoder (ldpc_toolbox_encoder_encode_batch / _device) against the host encoder -- which
tests/test_host_logic.py pins to the reference's own vectors -- and against H itself.  GF(2): everything is exact
equality."""
import json
import os

import numpy as np
import pytest

import encoder_reference as er
import ldpc_toolbox_amd as lt
from ldpc_toolbox_amd import simulation as sim

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")))

# name -> (alist source, puncturing pattern).  Short codes are compared with the host encoder in full, the long ones
# on a sample of 32 frames of the batch (the syndrome check always covers every frame).
SHORT = {
    "kat_dense": (lambda: KATS["encoder_dense"]["alist"], ""),          # n = 12
    "kat_staircase": (lambda: KATS["encoder_staircase"]["alist"], ""),  # n = 5: smaller than one wavefront
    "dvbs2:R1_2short": (lambda: lt.code_alist("dvbs2:R1_2short"), ""),
    "ar4ja:1/2:1024": (lambda: lt.code_alist("ar4ja:1/2:1024"), ""),
    "ar4ja:1/2:1024/punctured": (lambda: lt.code_alist("ar4ja:1/2:1024"), "1,1,1,1,0"),
    "nr5g:2:24": (lambda: lt.code_alist("nr5g:2:24"), ""),
    "nr5g:1:8": (lambda: lt.code_alist("nr5g:1:8"), ""),
}
LONG = {
    "dvbs2:R1_2": (lambda: lt.code_alist("dvbs2:R1_2"), ""),
    "dvbs2:R9_10": (lambda: lt.code_alist("dvbs2:R9_10"), ""),   # largest k: the LDS sizing edge (16 frames per word)
    "dvbs2:R1_4": (lambda: lt.code_alist("dvbs2:R1_4"), ""),     # most parity rows: the longest scan
    "nr5g:1:384": (lambda: lt.code_alist("nr5g:1:384"), ""),
}
SHORT_BATCHES = (1, 3, 67, 1000)
LONG_BATCH = 1030

_alists, _encoders, _messages, _codewords = {}, {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_device_state():
    """the cached encoders hold device buffers (tables, staging for a thousand long frames): freed when the module is done"""
    yield
    for enc in _encoders.values():
        enc.close()
    for cache in (_encoders, _messages, _codewords):
        cache.clear()


def _alist(name):
    if name not in _alists:
        _alists[name] = {**SHORT, **LONG}[name][0]()
    return _alists[name]


def _encoder(name):
    """one encoder per code and module (the Gauss reduction behind nr5g:1:384 takes seconds)"""
    if name not in _encoders:
        _encoders[name] = lt.Encoder(_alist(name), {**SHORT, **LONG}[name][1])
    return _encoders[name]


def _msgs(name, batch):
    if (name, batch) not in _messages:
        seed = sum(name.encode()) * 1000 + batch
        _messages[name, batch] = np.random.default_rng(seed).integers(0, 2, size=(batch, _encoder(name).k), dtype=np.uint8)
    return _messages[name, batch]


def _encoded(name, batch):
    if (name, batch) not in _codewords:
        _codewords[name, batch] = _encoder(name).encode_batch(_msgs(name, batch))
    return _codewords[name, batch]


def _host(enc, msgs):
    return np.stack([enc.encode(m, enc.output_len) for m in msgs])


def _sample(batch):
    """32 frames spread over the batch: first, last and a stride between"""
    return sorted(set([0, batch - 1] + list(range(1, batch - 1, max((batch - 2) // 30, 1)))[:30]))


CASES = [(n, b) for n in SHORT for b in SHORT_BATCHES] + [(n, LONG_BATCH) for n in LONG]


@pytest.mark.parametrize("name, batch", CASES, ids=[f"{n}-{b}" for n, b in CASES])
def test_equals_the_host_encoder(name, batch):
    enc, msgs, got = _encoder(name), _msgs(name, batch), _encoded(name, batch)
    assert got.shape == (batch, enc.output_len) and got.dtype == np.uint8
    rows = list(range(batch)) if name in SHORT else _sample(batch)
    if name in LONG:
        assert len(rows) == 32 and rows[0] == 0 and rows[-1] == batch - 1
    assert np.array_equal(got[rows], _host(enc, msgs[rows]))


@pytest.mark.parametrize("name", ["dvbs2:R1_2short", "nr5g:2:24", "kat_staircase", "ar4ja:1/2:1024/punctured"])
def test_only_a_byte_equal_to_one_is_a_one(name):
    """the scalar call's convention (c_api/encoder.rs:41-43): 2, 7 and 255 are zeros"""
    enc, msgs = _encoder(name), _msgs(name, 67)
    other = np.random.default_rng(5).choice(np.array([0, 2, 7, 255], dtype=np.uint8), size=msgs.shape)
    noisy = np.where(msgs == 1, np.uint8(1), other).astype(np.uint8)
    assert (noisy != msgs).any()
    got = enc.encode_batch(noisy)
    assert np.array_equal(got, _encoded(name, 67))
    assert np.array_equal(got, _host(enc, noisy))


def _h_rows(alist):
    h = lt.SparseMatrix.from_alist(alist)
    return [list(h.iter_row(r)) for r in range(h.num_rows())]


@pytest.mark.parametrize("name, batch", CASES, ids=[f"{n}-{b}" for n, b in CASES])
def test_codewords_are_systematic_and_satisfy_h(name, batch):
    """independent of the host encoder: the message comes first, and H c = 0 for EVERY frame of the batch -- by the GPU
    syndrome kernel, and by numpy on H's rows (tests/encoder_reference.py), which owes nothing to the library's kernels"""
    enc, msgs, got = _encoder(name), _msgs(name, batch), _encoded(name, batch)
    assert np.array_equal(got[:, :enc.k], msgs)
    assert set(np.unique(got).tolist()) <= {0, 1}
    if enc.output_len != enc.n:       # H applies to the full codeword: the same messages through the unpunctured encoder
        pattern = {**SHORT, **LONG}[name][1]
        name = name.split("/punctured")[0]
        full = _encoder(name).encode_batch(msgs)
        assert np.array_equal(got, sim.puncture(full, sim.parse_puncturing_pattern(pattern)))
        got = full
    dec = lt.LdpcDecoder(_alist(name), "Minsumf32", device=0)
    syn, weight = dec.syndrome(got)
    assert weight.shape == (batch,) and (weight == 0).all(), np.nonzero(weight)[0][:10]
    assert not syn.any()
    dec.close()
    assert not er.syndrome(_h_rows(_alist(name)), got).any()
    if name in SHORT:
        c = got.astype(np.int64)
        for cols in _h_rows(_alist(name)):
            assert not (c[:, cols].sum(axis=1) & 1).any()


@pytest.mark.parametrize("name", ["dvbs2:R1_2short", "nr5g:1:8", "ar4ja:1/2:1024/punctured", "dvbs2:R9_10"])
def test_device_entry(name):
    import torch
    enc = lt.Encoder(_alist(name), {**SHORT, **LONG}[name][1])       # a handle of its own: its work buffers grow and shrink below
    dev = torch.device("cuda:0")
    for batch in (67, 300, 5):                    # larger (the buffers grow), then smaller
        msgs = np.random.default_rng(batch).integers(0, 2, size=(batch, enc.k), dtype=np.uint8)
        want = enc.encode_batch(msgs)
        assert np.array_equal(want[_sample(batch)], _host(enc, msgs[_sample(batch)]))
        d_in = torch.from_numpy(msgs).to(dev)
        keep = d_in.clone()
        # stream = 0: the handle's own stream, ordered after torch's default stream, synchronous
        d_out = torch.full((batch, enc.output_len), 0xA5, dtype=torch.uint8, device=dev)
        enc.encode_batch_device(d_in.data_ptr(), d_out.data_ptr(), batch, stream=0)
        assert np.array_equal(d_out.cpu().numpy(), want)
        # a torch stream of the caller's: enqueue and return
        stream = torch.cuda.Stream(device=dev)
        d_out2 = torch.full((batch, enc.output_len), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            enc.encode_batch_device(d_in.data_ptr(), d_out2.data_ptr(), batch, stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(d_out2.cpu().numpy(), want)
        assert torch.equal(d_in, keep), "the input tensor is unchanged"


def test_unaligned_device_buffers():
    """tensors that start at an odd address take the byte-wise forms of the kernels"""
    import torch
    enc = _encoder("dvbs2:R1_2short")
    batch = 67
    msgs = _msgs("dvbs2:R1_2short", batch)
    dev = torch.device("cuda:0")
    raw_in = torch.zeros(batch * enc.k + 8, dtype=torch.uint8, device=dev)
    raw_out = torch.full((batch * enc.n + 8,), 0xA5, dtype=torch.uint8, device=dev)
    raw_in[1:1 + batch * enc.k] = torch.from_numpy(msgs).to(dev).reshape(-1)
    enc.encode_batch_device(raw_in.data_ptr() + 1, raw_out.data_ptr() + 3, batch)
    out = raw_out.cpu().numpy()
    assert np.array_equal(out[3:3 + batch * enc.n].reshape(batch, enc.n), _encoded("dvbs2:R1_2short", batch))
    assert (out[:3] == 0xA5).all() and (out[3 + batch * enc.n:] == 0xA5).all()


def test_round_trip_through_the_decoder():
    """512 fresh messages encoded on the GPU, BPSK + noise above threshold, min-sum decode: every message comes back"""
    alist = _alist("dvbs2:R1_2short")
    enc = lt.Encoder(alist, device=0)
    assert enc.device == 0, "the on-device constructor builds the device state at once"
    batch = 512
    msgs = np.random.default_rng(2024).integers(0, 2, size=(batch, enc.k), dtype=np.uint8)
    cws = enc.encode_batch(msgs)
    sigma = sim.noise_sigma(enc.k / enc.n, 3.0)       # (7200 / 16200 at Eb/N0 = 3 dB: well above the waterfall)
    symbols = sim.bpsk_modulate(cws) + sigma * np.random.default_rng(7).standard_normal(cws.shape)
    llrs = sim.bpsk_demodulate(symbols, sigma).astype(np.float32)
    dec = lt.LdpcDecoder(alist, "Minsumf32", device=0)
    bits, its, _ = dec.decode_batch(llrs, 50)
    assert (its >= 0).all()
    assert np.array_equal(bits[:, :enc.k], msgs)
    assert np.array_equal(bits, cws)


@pytest.mark.parametrize("name", ["kat_dense", "dvbs2:R1_2short"])
def test_device_state_is_lazy(name):
    enc = lt.Encoder(_alist(name))
    assert enc.device == -1
    msgs = _msgs(name, 3)
    before = _host(enc, msgs)
    assert enc.device == -1, "the scalar call needs no device state"
    got = enc.encode_batch(msgs)
    assert enc.device >= 0
    assert np.array_equal(got, before)
    assert np.array_equal(_host(enc, msgs), before)
