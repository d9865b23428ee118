"""GPU: every path of the batched encoder against tests/encoder_reference.py, a numpy statement of the encoding that does
not come from the library (tests/test_encoder_reference.py pins it), on synthetic codes that reach what the built-in
codes do not: the three forms of the staircase kernels and the sizes where one gives way to the next, the byte-wise
kernels at 16 and 32 frames per word, a second pass of both pass loops, a puncturing grid that strides, and rows of H0
with no, one and 2000 columns.

Every assertion is exact equality of the WHOLE GPU output with the reference, plus a zero syndrome of every frame; the
host encoder (one ctypes call per frame) is compared on at most 32 frames."""
import numpy as np
import pytest

import encoder_reference as er
import ldpc_toolbox_amd as lt

pytestmark = pytest.mark.gpu

PASS_STAIRCASE, PASS_DENSE = 4096, 1 << 20      # frames per pass of launch_staircase / launch_dense
FORM_BATCH = 70                                  # a ragged last group at 32 and at 16 frames per word
FORM_CODES = sorted(er.STAIRCASE_FORM_CODES)
ODD_CODES = [("staircase", k, m) for k, m in er.STAIRCASE_ODD_CODES] + [("triangular", k, m) for k, m in er.TRIANGULAR_CODES]
ODD_BATCHES = (1, 33, 67, 1000)

_encoders, _messages, _references = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_device_state():
    yield
    for enc in _encoders.values():
        enc.close()
    for cache in (_encoders, _messages, _references):
        cache.clear()


def _encoder(kind, k, m, pattern=""):
    if (kind, k, m, pattern) not in _encoders:
        _encoders[kind, k, m, pattern] = lt.Encoder(er.synthetic(kind, k, m)[1], pattern)
    enc = _encoders[kind, k, m, pattern]
    assert (enc.k, enc.n, enc.staircase) == (k, k + m, kind == "staircase")
    return enc


def _msgs(k, batch):
    if (k, batch) not in _messages:
        _messages[k, batch] = np.random.default_rng(1000 * k + batch).integers(0, 2, size=(batch, k), dtype=np.uint8)
        _messages[k, batch].setflags(write=False)
    return _messages[k, batch]


def _reference(kind, k, m, batch):
    """the numpy codewords of _msgs(k, batch): computed once, shared, read-only"""
    if (kind, k, m, batch) not in _references:
        rows = er.synthetic(kind, k, m)[0]
        ref = (er.encode_staircase if kind == "staircase" else er.encode_triangular)(k, rows, _msgs(k, batch))
        assert ref.shape == (batch, k + m) and np.array_equal(ref[:, :k], _msgs(k, batch))
        assert not er.syndrome(rows, ref).any()
        ref.setflags(write=False)
        _references[kind, k, m, batch] = ref
    return _references[kind, k, m, batch]


def _where(got, want, enc, batch):
    """the first differing (frame, column) and the pass, group, slice and chunk of the kernels it belongs to"""
    if got.shape != want.shape:
        return f"shape {got.shape}, expected {want.shape}"
    frame, col = (int(x) for x in np.argwhere(got != want)[0])
    text = f"{int((got != want).sum())} bytes differ in {int((got != want).any(axis=1).sum())} frames; first at frame {frame}, column {col}"
    if got.shape[1] != enc.n:
        return text + " (of the punctured output)"
    form = enc.staircase_form
    per_pass = PASS_STAIRCASE if form >= 0 else PASS_DENSE
    in_pass = frame % per_pass
    text += f": pass {frame // per_pass}, frame {in_pass} of the pass"
    if form < 0:
        return text + (f", message word {col // 64}" if col < enc.k else f", parity row {col - enc.k}")
    word = 16 if form == 1 else 32
    text += f", form {form}, group {in_pass // word} bit {in_pass % word}"
    if col < enc.k:
        return text + f", message column (pack workgroup {col // 256})"
    # (enc_staircase_pass: slices of whole 1024-row chunks, enough of them to fill the chip at a small batch)
    m, row = enc.n - enc.k, col - enc.k
    groups = (min(batch - frame // per_pass * per_pass, per_pass) + word - 1) // word
    slices = min(max((512 + groups - 1) // groups, 1), 8)
    slice_rows = ((m + slices - 1) // slices + 1023) // 1024 * 1024
    return text + f", parity row {row}: slice {row // slice_rows} (of {slice_rows} rows), chunk {row % slice_rows // 1024} of the slice"


def _check(got, kind, k, m, batch, enc, host_sample):
    """got == the numpy reference on every frame, zero syndrome on every frame, == the host encoder on the sample"""
    want = _reference(kind, k, m, batch)
    assert got.dtype == np.uint8
    assert np.array_equal(got, want), _where(got, want, enc, batch)
    syn = er.syndrome(er.synthetic(kind, k, m)[0], got)
    assert not syn.any(), f"check {np.argwhere(syn)[0][0]} fails in the frames of byte {np.argwhere(syn)[0][1]}"
    assert len(host_sample) <= 32
    host = np.stack([enc.encode(x, enc.n) for x in _msgs(k, batch)[host_sample]])
    assert np.array_equal(got[host_sample], host)


def _sample(batch):
    """at most 32 frames: the first 16 and the last 16"""
    return sorted(set(range(min(16, batch))) | set(range(max(batch - 16, 0), batch)))


def _device_encode(enc, msgs, in_offset, out_offset):
    """encode_batch_device on tensors that start `in_offset` / `out_offset` bytes past an aligned address; the 0xA5
    bytes around the output must come back untouched"""
    import torch
    dev = torch.device("cuda:0")
    batch, out_len = len(msgs), enc.output_len
    raw_in = torch.zeros(msgs.size + 8, dtype=torch.uint8, device=dev)
    raw_out = torch.full((batch * out_len + 16,), 0xA5, dtype=torch.uint8, device=dev)
    assert raw_in.data_ptr() % 8 == 0 and raw_out.data_ptr() % 8 == 0
    raw_in[in_offset:in_offset + msgs.size] = torch.tensor(msgs).to(dev).reshape(-1)
    enc.encode_batch_device(raw_in.data_ptr() + in_offset, raw_out.data_ptr() + out_offset, batch)
    out = raw_out.cpu().numpy()
    end = out_offset + batch * out_len
    assert (out[:out_offset] == 0xA5).all() and (out[end:] == 0xA5).all(), "guard bytes around the output"
    assert np.array_equal(raw_in.cpu().numpy()[in_offset:in_offset + msgs.size], msgs.reshape(-1)), "the input is unchanged"
    return out[out_offset:end].reshape(batch, out_len)


# -- a. the three forms of the staircase kernels and the sizes where they change ------------------------------------

@pytest.mark.parametrize("way", ["host", "device_aligned", "device_unaligned"])
@pytest.mark.parametrize("k, m", FORM_CODES, ids=[f"k{k}" for k, _ in FORM_CODES])
def test_staircase_form_boundaries(k, m, way):
    """kp = k rounded up to 8: 40704 is the last that fits in LDS at 32 frames per word (the largest dynamic LDS request
    there is), 40712 the first at 16; 81408 the last at 16, 81416 the first gathered from global memory; 40701 and 81409
    reach the same kp with a k that is no multiple of 8 (byte-wise kernels whatever the pointers are)"""
    enc = _encoder("staircase", k, m)
    expected = er.STAIRCASE_FORM_CODES[k, m]
    assert enc.staircase_form == expected, \
        f"k = {k} takes form {enc.staircase_form}, this case is meant for form {expected}: has kEncLdsBudget moved?"
    msgs = _msgs(k, FORM_BATCH)
    if way == "host":
        got = enc.encode_batch(msgs)
    else:
        got = _device_encode(enc, msgs, *((0, 0) if way == "device_aligned" else (1, 3)))
    _check(got, "staircase", k, m, FORM_BATCH, enc, _sample(FORM_BATCH))


@pytest.mark.parametrize("k, m", [(40701, 2300), (40712, 2300), (81409, 2300)], ids=["form0", "form1", "form2"])
def test_only_a_byte_equal_to_one_is_a_one_in_every_form(k, m):
    enc = _encoder("staircase", k, m)
    msgs = _msgs(k, FORM_BATCH)
    other = np.random.default_rng(5).choice(np.array([0, 2, 7, 255], dtype=np.uint8), size=msgs.shape)
    noisy = np.where(msgs == 1, np.uint8(1), other).astype(np.uint8)
    assert (noisy != msgs).any() and ((noisy == 1) == (msgs == 1)).all()
    assert np.array_equal(er.encode_staircase(k, er.synthetic("staircase", k, m)[0], noisy), _reference("staircase", k, m, FORM_BATCH))
    for got in (enc.encode_batch(noisy), _device_encode(enc, noisy, 0, 0)):
        want = _reference("staircase", k, m, FORM_BATCH)
        assert np.array_equal(got, want), _where(got, want, enc, FORM_BATCH)


# -- b. sizes that are no multiple of a tile, beyond one workgroup ---------------------------------------------------

@pytest.mark.parametrize("batch", ODD_BATCHES)
@pytest.mark.parametrize("kind, k, m", ODD_CODES, ids=[f"{kind}-{k}-{m}" for kind, k, m in ODD_CODES])
def test_odd_sizes(kind, k, m, batch):
    enc = _encoder(kind, k, m)
    _check(enc.encode_batch(_msgs(k, batch)), kind, k, m, batch, enc, _sample(batch))


# -- c. a second turn of the pass loops ------------------------------------------------------------------------------

def test_staircase_pass_boundaries():
    """one handle: exactly one pass, one frame into the second, a ragged second pass, then a small batch in the grown
    buffers"""
    k, m = 301, 1100
    enc = lt.Encoder(er.synthetic("staircase", k, m)[1])
    try:
        for batch in (PASS_STAIRCASE, PASS_STAIRCASE + 1, PASS_STAIRCASE + 37, 5):
            _check(enc.encode_batch(_msgs(k, batch)), "staircase", k, m, batch, enc, _sample(batch))
    finally:
        enc.close()


def test_dense_pass_boundary():
    k, m = 6, 6
    batch = PASS_DENSE + 65
    enc = _encoder("triangular", k, m)
    _check(enc.encode_batch(_msgs(k, batch)), "triangular", k, m, batch, enc, _sample(batch))


# -- d. puncturing ---------------------------------------------------------------------------------------------------

def test_puncture_grid_strides():
    """1100 x 2048 = 2 252 800 outputs, more than the 8192 workgroups of 256 threads the grid is capped at"""
    from ldpc_toolbox_amd import simulation as sim
    alist, pattern, batch = lt.code_alist("ar4ja:1/2:1024"), "1,1,1,1,0", 1100
    h = lt.SparseMatrix.from_alist(alist)
    rows = [sorted(h.iter_row(r)) for r in range(h.num_rows())]
    full_enc, enc = lt.Encoder(alist), lt.Encoder(alist, pattern)
    try:
        assert batch * enc.output_len > 8192 * 256
        msgs = np.random.default_rng(11).integers(0, 2, size=(batch, enc.k), dtype=np.uint8)
        full = full_enc.encode_batch(msgs)
        assert full.shape == (batch, enc.n) and np.array_equal(full[:, :enc.k], msgs)
        assert not er.syndrome(rows, full).any()
        want = er.puncture(full, sim.parse_puncturing_pattern(pattern))
        assert want.shape == (batch, 2048)
        for got in (enc.encode_batch(msgs), _device_encode(enc, msgs, 0, 0)):     # (the second into 0xA5 bytes)
            assert np.array_equal(got, want), _where(got, want, enc, batch)
        sample = _sample(batch)
        assert np.array_equal(want[sample], np.stack([enc.encode(x, enc.output_len) for x in msgs[sample]]))
    finally:
        full_enc.close()
        enc.close()


@pytest.mark.parametrize("pattern", ["0,1,1", "1,1,0", "1,1,1"])
def test_puncture_staircase_odd_blocks(pattern):
    """n = 1401 = 3 x 467: blocks of odd length that start at odd offsets, cut through the message (k = 301)"""
    from ldpc_toolbox_amd import simulation as sim
    k, m, batch = 301, 1100, 67
    enc = _encoder("staircase", k, m, pattern)
    keep = sim.parse_puncturing_pattern(pattern)
    assert enc.output_len == 467 * sum(keep)
    want = er.puncture(_reference("staircase", k, m, batch), keep)
    for got in (enc.encode_batch(_msgs(k, batch)), _device_encode(enc, _msgs(k, batch), 1, 3)):
        assert np.array_equal(got, want), _where(got, want, enc, batch)
    assert np.array_equal(want[:8], np.stack([enc.encode(x, enc.output_len) for x in _msgs(k, batch)[:8]]))


def test_puncture_everything():
    """a pattern of zeros only is accepted: the output length is 0, and a batched call succeeds and returns [batch][0]"""
    k, m, batch = 301, 1100, 67
    enc = _encoder("staircase", k, m, "0,0,0")
    assert enc.output_len == 0
    got = enc.encode_batch(_msgs(k, batch))
    assert got.shape == (batch, 0) and got.dtype == np.uint8
