"""CPU: pins tests/bch_reference.py, the numpy restatement the GPU tests of the BCH code compare against -- the 24
polynomials of EN 302 307-1 Tables 6a / 6b, the generator anchors, the (n, k, t) table, and the two decoders (the
definition as a syndrome table, and Berlekamp-Massey with a root search) against each other on the small codes."""
import json
import os

import numpy as np
import pytest

import bch_reference as br

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dvbs2_bch_polynomials.json")

GENERATORS = [  # (m, P, t, g)
    (16, br.P_NORMAL, 8, 0x11c07255f712797bd19fc6d7504f9662b),
    (16, br.P_NORMAL, 10, 0x160150cedfc2a331f6a785703efd12301b8bb6591),
    (16, br.P_NORMAL, 12, 0x14e260e83845c511c50cf2cd8dc350889034785f7660255e7),
    (14, br.P_SHORT, 8, 0x192d612e23675eda463552df84609),
    (14, br.P_SHORT, 10, 0x1dbfd25eb862e4274cbbd64bda7f7b65cc0f),
    (14, br.P_SHORT, 12, 0x14062dbea9869b262cd23a39069528fe7d7d11905a5),
]
SMALL = [("bch:5:25:3:31", 0x8faf, 16), ("bch:6:43:3:63", 0x782cf, 45), ("bch:6:43:2:40", 0x1539, 28)]


@pytest.mark.parametrize("frame", ["normal", "short"])
def test_minimal_polynomials_are_the_standards(frame):
    gold = json.load(open(GOLDEN))[frame]
    code = br.Code(gold["m"], br.P_NORMAL if frame == "normal" else br.P_SHORT, 12, (1 << gold["m"]) - 1)
    want = [sum(1 << e for e in exps) for exps in gold["polynomials"]]
    assert len(want) == 12 and code.minimal == want
    assert want[0] == code.field.poly, "g1 is the primitive polynomial"


@pytest.mark.parametrize("m,poly,t,g", GENERATORS)
def test_generator_anchors(m, poly, t, g):
    code = br.Code(m, poly, t, (1 << m) - 1)
    assert code.g == g and code.parity == m * t
    # g divides x^(2^m - 1) - 1
    assert br.poly_mod((1 << ((1 << m) - 1)) ^ 1, g) == 0


@pytest.mark.parametrize("spec,g,k", SMALL)
def test_small_code_anchors(spec, g, k):
    code = br.Code.from_spec(spec)
    assert code.g == g and code.k == k
    assert br.poly_mod((1 << code.field.order) ^ 1, g) == 0


def test_equal_minimal_polynomials_are_taken_once():
    # GF(2^4), t = 7: alpha^9 is a conjugate of alpha^3, alpha^11 and alpha^13 of alpha^7
    code = br.Code(4, 0x13, 7, 15)
    assert len(code.minimal) == 4 and code.parity == 14


def test_dvbs2_table():
    assert len(br.DVBS2) == 21
    for name, (n, k, t) in br.DVBS2.items():
        m = 14 if name.endswith("short") else 16
        assert k == n - m * t, name
        if name.endswith("short"):
            assert t == 12 and k == n - 168
    assert br.DVBS2["R1_2"] == (32400, 32208, 12) and br.DVBS2["R2_3"][2] == 10 and br.DVBS2["R9_10"] == (58320, 58192, 8)
    code = br.Code.from_spec("dvbs2:R1_2short")
    assert (code.n, code.k, code.t, code.m) == (7200, 7032, 12, 14)


def test_encoder_is_systematic_and_gives_codewords():
    rng = np.random.default_rng(3)
    for spec in ("bch:5:25:3:25", "bch:14:402B:12:300", "dvbs2:R9_10"):
        code = br.Code.from_spec(spec)
        msgs = rng.integers(0, 2, (3, code.k), dtype=np.uint8)
        msgs[1] *= 255  # a byte other than 1 is a zero
        cw = code.encode(msgs)
        assert np.array_equal(cw[:, :code.k], (msgs == 1).astype(np.uint8))
        assert all(code.is_codeword(r) for r in cw)
        v = code.to_int(cw[0])
        assert br.poly_mod(v, code.g) == 0


@pytest.mark.parametrize("spec,weights,count,detected,miscorrected", [
    ("bch:5:25:3:25", (0, 1, 2, 3), 2626, 0, 0),
    ("bch:5:25:3:25", (4,), 12650, 11705, 945),
    ("bch:6:43:2:40", (3,), 9880, 8540, 1340),
])
def test_table_and_algebraic_decoders_agree(spec, weights, count, detected, miscorrected):
    code = br.Code.from_spec(spec)
    cw = code.encode(np.random.default_rng(5).integers(0, 2, (1, code.k), dtype=np.uint8))[0]
    pats = br.patterns(code.n, weights)
    assert len(pats) == count
    rows = pats ^ cw
    out_t, err_t = code.decode_table(rows)
    out_a, err_a = code.decode(rows)
    assert np.array_equal(out_t, out_a) and np.array_equal(err_t, err_a)
    failed = err_t < 0
    assert np.array_equal(out_t[failed], rows[failed]), "a word that fails comes back unchanged"
    assert int(failed.sum()) == detected
    if max(weights) > code.t:
        assert int((~failed).sum()) == miscorrected
    if max(weights) <= code.t:
        assert (out_t == cw).all() and np.array_equal(err_t, pats.sum(axis=1))
    else:
        good = ~failed  # miscorrections: another codeword, within t of the input
        assert all(code.is_codeword(r) for r in out_t[good][:50])
        assert ((out_t[good] != rows[good]).sum(axis=1) == err_t[good]).all() and (err_t[good] <= code.t).all()
        assert not (out_t[good] == cw).all(axis=1).any()
