"""CPU: pins tests/encoder_reference.py, the numpy reference the batched GPU encoder is tested against
(tests/test_gpu_encoder_forms.py): to the reference project's known answers, to the host encoder on the synthetic
codes and a built-in one, and to itself (a syndrome check that can fail)."""
import json
import os

import numpy as np
import pytest

import encoder_reference as er
import ldpc_toolbox_amd as lt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")))

STAIRCASE = tuple(er.STAIRCASE_FORM_CODES) + er.STAIRCASE_ODD_CODES
BATCH = 70


def _rows_of(alist):
    """rows of an alist as encoder_reference wants them: sorted, so the diagonal of a triangular H comes last"""
    h = lt.SparseMatrix.from_alist(alist)
    return [sorted(h.iter_row(r)) for r in range(h.num_rows())]


def _host(enc, msgs):
    return np.stack([enc.encode(m, enc.n) for m in msgs])


def _messages(k, batch=BATCH):
    """bytes 0/1, and in the last rows 2, 7 and 255 where a zero was: they count as zeros"""
    rng = np.random.default_rng(k)
    msgs = rng.integers(0, 2, size=(batch, k), dtype=np.uint8)
    tail = msgs[-3:]
    tail[tail == 0] = rng.choice(np.array([0, 2, 7, 255], dtype=np.uint8), size=int((tail == 0).sum()))
    return msgs


def test_staircase_reference_reproduces_the_known_answers():
    kat = KATS["encoder_staircase"]
    rows = _rows_of(kat["alist"])
    k = len(kat["pairs"][0][0])
    assert len(kat["pairs"]) >= 2
    for msg, cw in kat["pairs"]:
        assert er.encode_staircase(k, rows, np.array([msg], dtype=np.uint8))[0].tolist() == cw
    msgs = np.array([p[0] for p in kat["pairs"]], dtype=np.uint8)
    assert er.encode_staircase(k, rows, msgs).tolist() == [p[1] for p in kat["pairs"]]
    assert not er.syndrome(rows, np.array([p[1] for p in kat["pairs"]], dtype=np.uint8)).any()


def test_dense_known_answers_are_systematic_with_zero_syndrome():
    kat = KATS["encoder_dense"]
    rows = _rows_of(kat["alist"])
    assert len(kat["pairs"]) >= 2
    for msg, cw in kat["pairs"]:
        assert cw[:len(msg)] == msg
        assert not er.syndrome(rows, np.array([cw], dtype=np.uint8)).any()
        flipped = np.array([cw], dtype=np.uint8)
        flipped[0, -1] ^= 1
        assert er.syndrome(rows, flipped).any()


@pytest.mark.parametrize("k, m", STAIRCASE, ids=[f"{k}-{m}" for k, m in STAIRCASE])
def test_staircase_reference_equals_the_host_encoder(k, m):
    rows, alist = er.synthetic("staircase", k, m)
    enc = lt.Encoder(alist)
    assert enc.staircase and (enc.k, enc.n) == (k, k + m)
    assert enc.staircase_form == er.STAIRCASE_FORM_CODES.get((k, m), 0)
    msgs = _messages(k)
    ref = er.encode_staircase(k, rows, msgs)
    assert np.array_equal(ref, _host(enc, msgs))
    assert not er.syndrome(rows, ref).any()


def test_staircase_rows_have_the_planted_shapes():
    for k, m in STAIRCASE:
        rows, _ = er.synthetic("staircase", k, m)
        degree = [sum(c < k for c in cs) for cs in rows]
        planted = er.planted_degrees(m)
        assert (len(planted) == 12) == (m > 1030)
        for r, d in planted.items():
            assert degree[r] == min(d, k), (k, m, r)
        assert {0, 1, min(er.LONG_ROW, k)} <= set(degree)
        assert all(2 <= d <= 8 for r, d in enumerate(degree) if r not in planted and r != 5)
        used = {c for cs in rows for c in cs}
        assert 0 in used and k - 1 in used
        assert all(len(set(cs)) == len(cs) for cs in rows)


@pytest.mark.parametrize("k, m", er.TRIANGULAR_CODES, ids=[f"{k}-{m}" for k, m in er.TRIANGULAR_CODES])
def test_triangular_reference_equals_the_host_encoder(k, m):
    rows, alist = er.synthetic("triangular", k, m)
    enc = lt.Encoder(alist)
    assert not enc.staircase and enc.staircase_form == -1 and (enc.k, enc.n) == (k, k + m)
    assert any(all(c >= k for c in cs) for cs in rows), "some H0 row is empty"
    msgs = _messages(k)
    ref = er.encode_triangular(k, rows, msgs)
    assert np.array_equal(ref, _host(enc, msgs))
    assert not er.syndrome(rows, ref).any()


def test_staircase_reference_equals_the_host_encoder_on_a_built_in_code():
    alist = lt.code_alist("dvbs2:R1_2short")
    rows, enc = _rows_of(alist), lt.Encoder(alist)
    msgs = _messages(enc.k, 9)
    ref = er.encode_staircase(enc.k, rows, msgs)
    assert np.array_equal(ref, _host(enc, msgs))
    assert not er.syndrome(rows, ref).any()


def test_syndrome_looks_at_every_frame():
    k, m = 301, 1100
    rows, _ = er.synthetic("staircase", k, m)
    cws = er.encode_staircase(k, rows, _messages(k))
    assert cws.shape == (BATCH, k + m) and not er.syndrome(rows, cws).any()
    for frame, col in ((BATCH - 1, k + m - 1), (BATCH - 1, 0), (0, k), (37, 17)):
        bad = cws.copy()
        bad[frame, col] ^= 1
        syn = er.syndrome(rows, bad)
        assert syn.any()
        # the frame is where the docstring says: bit 7 - f % 8 of byte f // 8, and no other frame is touched
        assert set(np.nonzero(syn)[1].tolist()) == {frame // 8}
        assert set(np.unique(syn).tolist()) == {0, 0x80 >> (frame % 8)}


def test_puncture_selects_blocks():
    cw = np.arange(2 * 12, dtype=np.uint8).reshape(2, 12)
    assert er.puncture(cw, [0, 1, 1]).tolist() == [[4, 5, 6, 7, 8, 9, 10, 11], [16, 17, 18, 19, 20, 21, 22, 23]]
    assert er.puncture(cw, [1, 0, 1, 0]).tolist() == [[0, 1, 2, 6, 7, 8], [12, 13, 14, 18, 19, 20]]
    assert np.array_equal(er.puncture(cw, [1, 1, 1]), cw)
    assert er.puncture(cw, [0, 0]).shape == (2, 0)
    # the library's own host-side puncturing step agrees
    from ldpc_toolbox_amd import simulation as sim
    assert np.array_equal(er.puncture(cw, [1, 0, 1, 0]), sim.puncture(cw, sim.parse_puncturing_pattern("1,0,1,0")))
