"""GPU: the batched BCH encoder and bounded-distance decoder against tests/bch_reference.py (tests/test_bch_reference.py
pins it): exhaustively on small codes against the syndrome-table decoder, on the DVB-S2 fields at the lengths where the
kernels take another path, on every DVB-S2 name, and through every form of the entries.  Every comparison is
np.array_equal on every byte and every `errors` value."""
import numpy as np
import pytest
import torch

import bch_reference as br
import ldpc_toolbox_amd as lt

pytestmark = pytest.mark.gpu

PASS_FRAMES = 16384   # csrc/device_bch.h, kBchPassFrames
STAGE_FRAMES = 1 << 20  # csrc/device_bch.h, kBchStageFrames: what a host entry stages on the device at a time


def _small_batch(spec, weights, codewords=3):
    """every pattern of the weights on `codewords` codewords, the table decoder's result for each (by linearity the
    decoder's result on cw + e is cw + its result on e: the table is walked once per pattern)"""
    ref = br.Code.from_spec(spec)
    pats = br.patterns(ref.n, weights)
    out_e, err_e = ref.decode_table(pats)
    msgs = np.random.default_rng(ref.n).integers(0, 2, (codewords, ref.k), dtype=np.uint8)
    cws = ref.encode(msgs)
    rows = np.concatenate([pats ^ cw for cw in cws])
    want = np.concatenate([out_e ^ cw for cw in cws])
    return ref, msgs, cws, pats, rows, want, np.tile(err_e, codewords)


@pytest.mark.parametrize("spec,weights", [("bch:5:25:3:31", (0, 1, 2, 3, 4)), ("bch:5:25:3:25", (0, 1, 2, 3, 4)),
                                          ("bch:6:43:2:40", (0, 1, 2, 3))])
def test_small_codes_exhaustively(spec, weights):
    ref, msgs, cws, pats, rows, want, want_err = _small_batch(spec, weights)
    code = lt.BchCode(spec)
    assert np.array_equal(code.encode(msgs), cws)
    out, err = code.decode(rows, whole=True)
    weight = np.tile(pats.sum(axis=1), len(cws))
    corrected = (want_err >= 0) & (weight <= ref.t)
    detected = want_err < 0
    miscorrected = (want_err >= 0) & (weight > ref.t)
    print(f"{spec}: {len(rows)} frames: {corrected.sum()} corrected, {detected.sum()} detected, {miscorrected.sum()} miscorrected")
    assert corrected.any() and detected.any() and miscorrected.any()
    assert np.array_equal(err, want_err)
    assert np.array_equal(out, want)
    msg_out, err2 = code.decode(rows)
    assert np.array_equal(msg_out, want[:, :ref.k]) and np.array_equal(err2, want_err)
    code.close()


# The lengths N at which the kernels take another path (csrc/bch.h, geometry; csrc/kernels_bch.hip.h).  A frame of `bits`
# bits (N for the decoder, N - parity for the encoder) is cut into runs of 32 * W bits over `lanes` lanes:
#   W (odd) grows where ceil(bits / 32) passes a multiple of 256 words: bits 8192 | 8193 (W 1 -> 3), 24576 | 24577 (3 -> 5),
#   40960 | 40961 (5 -> 7), 57344 | 57345 (7 -> 9);
#   lanes pass a wave at bits 2048 | 2049 (64 -> 65 lanes of one word), which is also a multiple of the 256 positions one
#   step of the staging loop and of the root search covers; 300 is no multiple of 32.
# Each is taken for the decoder (N) and, parity added, for the encoder (N - parity).  parity + 1 leaves one message
# bit; 2^m - 1 is the unshortened code.  The remainder register has 4, 5 and 6 words for t = 8, 10 and 12 over GF(2^16).
def _lengths(m, t, boundaries):
    parity = m * t
    ns = {parity + 1, 300 if m == 14 else 1000, (1 << m) - 1}
    for b in boundaries:
        ns |= {b, b + 1, b + parity, b + parity + 1}
    return sorted(x for x in ns if parity + 1 <= x <= (1 << m) - 1)


PATH_CASES = [(14, "402B", 12, n) for n in _lengths(14, 12, (2048, 8192))] + \
             [(16, "1002D", t, n) for t in (8, 10, 12) for n in _lengths(16, t, (2048, 8192, 24576, 40960, 57344))]


def _planted(ref, rng):
    """rows with planted errors (the kinds of the issue), on one random codeword"""
    n, k, t, parity = ref.n, ref.k, ref.t, ref.parity
    cw = ref.encode(rng.integers(0, 2, (1, k), dtype=np.uint8))[0]
    kinds = [[], [0], [n - 1], [k - 1, k], list(range(n // 2, n // 2 + t)),
             [k + (i * parity) // t for i in range(t)], sorted({(i * (n - 1)) // (t - 1) for i in range(t)}),
             sorted(rng.choice(n, t + 1, replace=False).tolist()), sorted(rng.choice(n, t + 2, replace=False).tolist())]
    rows = np.tile(cw, (len(kinds) + 1, 1))
    for f, where in enumerate(kinds):
        rows[f, where] ^= 1
    # a word within t of a DIFFERENT codeword: cw + g (g's coefficients in the last parity + 1 bytes) with t of g's
    # ones taken back
    g_row = ref.to_row(ref.g, n)
    support = np.flatnonzero(g_row)
    assert len(support) > 2 * t
    rows[-1] ^= g_row
    rows[-1, support[:t]] ^= 1
    return cw, rows


@pytest.mark.parametrize("m,poly,t,n", PATH_CASES)
def test_dvbs2_fields_at_every_path(m, poly, t, n):
    spec = f"bch:{m}:{poly}:{t}:{n}"
    ref = br.Code.from_spec(spec)
    rng = np.random.default_rng(n + t)
    cw, rows = _planted(ref, rng)
    want, want_err = ref.decode(rows)
    assert want_err[0] == 0 and want_err[1] == 1 and want_err[2] == 1 and want_err[3] == 2 and (want_err[4:7] == t).all()
    assert (want[:7] == cw).all()
    assert want_err[-1] == t and not np.array_equal(want[-1], cw), "the last word belongs to another codeword"
    code = lt.BchCode(spec)
    msgs = rng.integers(0, 2, (5, ref.k), dtype=np.uint8)
    assert np.array_equal(code.encode(msgs), ref.encode(msgs))
    out, err = code.decode(rows, whole=True)
    assert np.array_equal(err, want_err), (err, want_err)
    assert np.array_equal(out, want)
    code.close()


@pytest.mark.parametrize("name", sorted(br.DVBS2))
def test_every_dvbs2_name(name):
    ref = br.Code.from_spec("dvbs2:" + name)
    code = lt.BchCode("dvbs2:" + name)
    assert sum(int(b) << i for i, b in enumerate(code.generator())) == ref.g
    rng = np.random.default_rng(ref.n)
    msgs = rng.integers(0, 2, (4, ref.k), dtype=np.uint8)
    cws = ref.encode(msgs)
    assert np.array_equal(code.encode(msgs), cws)
    rows = cws.copy()
    for f, w in enumerate((0, 1, ref.t, ref.t + 1)):
        rows[f, rng.choice(ref.n, w, replace=False)] ^= 1
    want, want_err = ref.decode(rows)
    assert want_err[:3].tolist() == [0, 1, ref.t]
    out, err = code.decode(rows)
    assert np.array_equal(err, want_err) and np.array_equal(out, want[:, :ref.k])
    code.close()


# ---- entry forms -----------------------------------------------------------------------------------------------------

FORM_SPEC = "bch:14:402B:12:300"


@pytest.fixture(scope="module")
def form_case():
    ref = br.Code.from_spec(FORM_SPEC)
    rng = np.random.default_rng(77)
    msgs = rng.integers(0, 2, (67, ref.k), dtype=np.uint8)
    cws = ref.encode(msgs)
    rows = cws.copy()
    for f in range(67):
        rows[f, rng.choice(ref.n, f % (ref.t + 3), replace=False)] ^= 1
    want, want_err = ref.decode(rows)
    assert (want_err < 0).any() and (want_err == ref.t).any() and (want_err == 0).any()
    for a in (msgs, cws, rows, want, want_err):
        a.setflags(write=False)
    code = lt.BchCode(FORM_SPEC)
    yield ref, code, msgs, cws, rows, want, want_err
    code.close()


def _device_bytes(array, offset):
    """a device copy of a uint8 array at an odd byte offset, sentinels around it: (tensor, pointer)"""
    flat = np.ascontiguousarray(array, dtype=np.uint8).reshape(-1)
    t = torch.full((flat.size + offset + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    t[offset:offset + flat.size] = torch.from_numpy(flat.copy()).cuda()
    return t, t.data_ptr() + offset


@pytest.mark.parametrize("batch", [0, 1, 67])
@pytest.mark.parametrize("whole", [False, True])
def test_host_entry(form_case, batch, whole):
    ref, code, msgs, cws, rows, want, want_err = form_case
    assert np.array_equal(code.encode(msgs[:batch]), cws[:batch])
    out, err = code.decode(rows[:batch], whole=whole)
    assert np.array_equal(out, want[:batch, :ref.n if whole else ref.k]) and np.array_equal(err, want_err[:batch])


@pytest.mark.parametrize("own_stream", [True, False])
@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("with_errors", [True, False])
def test_device_entry(form_case, own_stream, whole, with_errors):
    ref, code, msgs, cws, rows, want, want_err = form_case
    B, out_len = len(rows), ref.n if whole else ref.k
    stream = None if own_stream else torch.cuda.Stream()
    handle = 0 if own_stream else stream.cuda_stream
    # encoder: input and output at odd offsets, sentinels before and after the output
    d_msg, p_msg = _device_bytes(msgs, 3)
    d_cw, p_cw = _device_bytes(np.full((B, ref.n), 0xA5, dtype=np.uint8), 1)
    # decoder
    d_in, p_in = _device_bytes(rows, 5)
    d_out, p_out = _device_bytes(np.full((B, out_len), 0xA5, dtype=np.uint8), 7)
    d_err = torch.full((B + 2,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    code.encode_device(p_msg, p_cw, B, stream=handle)
    code.decode_device(p_in, p_out, B, errors_ptr=d_err.data_ptr() + 4 if with_errors else 0, whole=whole, stream=handle)
    if stream is not None:
        stream.synchronize()
    got_cw, got_out, got_err = d_cw.cpu().numpy(), d_out.cpu().numpy(), d_err.cpu().numpy()
    assert np.array_equal(got_cw[1:1 + B * ref.n].reshape(B, ref.n), cws)
    assert (got_cw[:1] == 0xA5).all() and (got_cw[1 + B * ref.n:] == 0xA5).all(), "the encoder wrote outside its output"
    assert np.array_equal(got_out[7:7 + B * out_len].reshape(B, out_len), want[:, :out_len])
    assert (got_out[:7] == 0xA5).all() and (got_out[7 + B * out_len:] == 0xA5).all(), "the decoder wrote outside its output"
    if with_errors:
        assert np.array_equal(got_err[1:1 + B], want_err) and got_err[0] == 77 and got_err[-1] == 77
    else:
        assert (got_err == 77).all()
    assert code.get("device") == 0


def test_input_bytes_other_than_one_are_zeros(form_case):
    ref, code, msgs, cws, rows, want, want_err = form_case
    fill = np.array([0, 2, 255, 128], dtype=np.uint8)
    loud_msgs = np.where(msgs == 1, 1, fill[np.arange(msgs.size).reshape(msgs.shape) % 4]).astype(np.uint8)
    loud_rows = np.where(rows == 1, 1, fill[np.arange(rows.size).reshape(rows.shape) % 4]).astype(np.uint8)
    assert (loud_msgs == 2).any() and (loud_rows == 255).any()
    assert np.array_equal(code.encode(loud_msgs), cws)
    out, err = code.decode(loud_rows, whole=True)
    assert np.array_equal(out, want) and np.array_equal(err, want_err), "a failed word comes back normalised, otherwise unchanged"


def test_one_batch_past_the_pass_limit():
    ref, msgs, cws, pats, rows, want, want_err = _small_batch("bch:5:25:3:31", (0, 1, 2, 3, 4), codewords=1)
    code = lt.BchCode("bch:5:25:3:31")
    assert code.get("pass_frames") == PASS_FRAMES and len(rows) > PASS_FRAMES + 1
    B = PASS_FRAMES + 1
    out, err = code.decode(rows[:B], whole=True)
    assert np.array_equal(err, want_err[:B]) and np.array_equal(out, want[:B])
    assert (want_err[PASS_FRAMES:B] != 0).all(), "the frame of the second pass needs the decoder"
    many = np.random.default_rng(9).integers(0, 2, (B, ref.k), dtype=np.uint8)
    got = code.encode(many)
    assert np.array_equal(got[:, :ref.k], many)
    assert np.array_equal(got[[0, PASS_FRAMES - 1, PASS_FRAMES]], ref.encode(many[[0, PASS_FRAMES - 1, PASS_FRAMES]]))
    # every row is a codeword: the decoder says so
    out, err = code.decode(got)
    assert (err == 0).all() and np.array_equal(out, many)
    code.close()


def test_one_host_batch_past_the_staging_limit():
    """a host call of more frames than the handle stages at a time: the 25-bit code's patterns, over and over"""
    ref, msgs, cws, pats, rows, want, want_err = _small_batch("bch:5:25:3:25", (0, 1, 2, 3, 4), codewords=1)
    code = lt.BchCode("bch:5:25:3:25")
    assert code.get("stage_frames") == STAGE_FRAMES
    B = STAGE_FRAMES + 1
    pick = np.arange(B) % len(rows)
    assert want_err[pick[-1]] != 0, "the frame of the second stage needs the decoder"
    out, err = code.decode(rows[pick], whole=True)
    assert np.array_equal(err, want_err[pick]) and np.array_equal(out, want[pick])
    many = want[pick][:, :ref.k]
    got = code.encode(many)
    assert np.array_equal(got[:, :ref.k], many) and np.array_equal(got[want_err[pick] >= 0], want[pick][want_err[pick] >= 0])
    assert np.array_equal(got[-1], ref.encode(many[-1:])[0])
    code.close()
