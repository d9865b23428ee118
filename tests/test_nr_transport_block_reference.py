"""CPU: pins the numpy restatement of the NR transport block processing (tests/nr_transport_block_reference.py) to values
that do not come from it: the CRC catalogue's check values, and segmentation results worked out by hand from TS 38.212
5.2.2."""
import numpy as np
import pytest

import nr_transport_block_reference as tr

# (BG, A): (C, K', Kb, Zc, K, F)
TABLE = {
    (2, 1): (1, 17, 6, 3, 30, 13),
    (2, 8): (1, 24, 6, 4, 40, 16),
    (2, 176): (1, 192, 6, 32, 320, 128),
    (2, 177): (1, 193, 8, 26, 260, 67),
    (2, 544): (1, 560, 8, 72, 720, 160),
    (2, 545): (1, 561, 9, 64, 640, 79),
    (2, 624): (1, 640, 9, 72, 720, 80),
    (2, 625): (1, 641, 10, 72, 720, 79),
    (2, 3824): (1, 3840, 10, 384, 3840, 0),
    (2, 3826): (2, 1949, 10, 208, 2080, 131),
    (2, 7641): (3, 2579, 10, 288, 2880, 301),
    (1, 292): (1, 308, 22, 14, 308, 0),
    (1, 3824): (1, 3840, 22, 176, 3872, 32),
    (1, 3825): (1, 3849, 22, 176, 3872, 23),
    (1, 8424): (1, 8448, 22, 384, 8448, 0),
    (1, 8426): (2, 4249, 22, 208, 4576, 327),
    (1, 1277992): (152, 8432, 22, 384, 8448, 16),
}
REFUSED = [(2, 3825), (2, 7640), (2, 7642), (1, 8425), (1, 16850)]


def test_crc_check_values_of_the_catalogue():
    """the 72 bits of ASCII "123456789", MSB first, zero init, no reflection, no final XOR"""
    bits = np.unpackbits(np.frombuffer(b"123456789", dtype=np.uint8))
    for poly, check in ((tr.CRC24A, 0xCDE703), (tr.CRC24B, 0x23EF52), (tr.CRC16, 0x31C3)):
        p = tr.parity_bits(bits, poly)
        assert int("".join(map(str, p)), 2) == check
        assert tr.remainder(np.concatenate([bits, p]), poly) == 0, "a sequence that ends in its CRC divides"
        assert tr.remainder(np.concatenate([bits ^ np.eye(72, dtype=np.uint8)[5], p]), poly) != 0


def test_lifting_sizes():
    assert len(tr.LIFTING_SIZES) == 51 and len(set(tr.LIFTING_SIZES)) == 51
    assert tr.LIFTING_SIZES[:8] == [2, 3, 4, 5, 6, 7, 8, 9] and tr.LIFTING_SIZES[-3:] == [320, 352, 384]


@pytest.mark.parametrize("bg,a", sorted(TABLE))
def test_segmentation_table(bg, a):
    c = tr.Config(bg, a)
    assert c.row() == TABLE[(bg, a)]
    assert c.l_tb == (24 if a > 3824 else 16) and c.b == a + c.l_tb and c.l_cb == (24 if c.c > 1 else 0)
    assert c.n == (68 if bg == 1 else 52) * c.zc


def test_crc_choice_at_3824():
    assert tr.Config(1, 3824).tb_poly == tr.CRC16 and tr.Config(1, 3825).tb_poly == tr.CRC24A


@pytest.mark.parametrize("bg,a", REFUSED)
def test_refused_pairs(bg, a):
    with pytest.raises(ValueError):
        tr.Config(bg, a)


@pytest.mark.parametrize("bg,a", [(2, 8), (2, 3826), (2, 7641)])
def test_segment_and_desegment_round_trip(bg, a):
    c = tr.Config(bg, a)
    rng = np.random.default_rng(a)
    payload = rng.integers(0, 2, (3, a), dtype=np.uint8)
    rows = c.segment(payload)
    assert rows.shape == (3 * c.c, c.k) and not rows[:, c.k_prime:].any()
    got, tb_ok, cb_ok = c.desegment(rows)
    assert np.array_equal(got, payload) and tb_ok.all() and cb_ok.all()
    # block r of transport block t carries bits r (K' - L_cb) .. of (payload, CRC): block-major rows
    take = min(c.k_prime - c.l_cb, a)
    assert np.array_equal(rows[1, :take], payload[1, :take])
    if c.c > 1:
        assert np.array_equal(rows[1 * 3 + 1, :5], payload[1, take:take + 5])
    rows[0 * 3 + 2, 0] ^= 1
    _, tb_ok, cb_ok = c.desegment(rows)
    assert list(tb_ok) == [1, 1, 0] and cb_ok.sum() == 3 * c.c - 1 and cb_ok[2, 0] == 0


def test_block_lengths_and_concatenation():
    c = tr.Config(2, 7641)
    assert c.block_lengths(3 * 100, 2) == [100, 100, 100]
    assert c.block_lengths(2 * 151, 2) == [100, 100, 102]
    assert c.block_lengths(6 * 11, 6) == [18, 24, 24]
    g, q, batch = 2 * 151, 2, 2
    blocks = [np.full((batch, e), r, dtype=np.uint8) + 10 * np.arange(batch, dtype=np.uint8)[:, None] for r, e in enumerate([100, 100, 102])]
    packed = c.pack(blocks)
    rx = c.split(np.arange(batch * g, dtype=np.float32).reshape(batch, g), q)
    assert rx[0] == 0 and rx[100] == g and rx[200] == 100 and rx[400] == 200 and rx[502] == g + 200
    out = c.concatenate(np.where(packed == 1, 1, 0), batch, g, q)
    assert out.shape == (batch, g) and out[0, 100:200].all() and not out[0, :100].any() and not out[1].any()
    assert np.array_equal(c.split(np.asarray(c.concatenate(packed % 2, batch, g, q), dtype=np.float64), q), (packed % 2).astype(np.float64))


def test_base_graph_boundaries():
    assert [tr.base_graph(a, r) for a, r in ((292, 0.9), (293, 0.9), (3824, 0.67), (3824, 0.68), (3825, 0.67), (3825, 0.25), (3825, 0.26))] == \
        [2, 1, 2, 1, 1, 2, 1]
