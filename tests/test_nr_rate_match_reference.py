"""CPU: pins the numpy restatement of NR rate matching (tests/nr_rate_match_reference.py) that the GPU tests compare with:
the k0 values of TS 38.212 Table 5.4.2.1-2, and the properties any bit selection has."""
import numpy as np
import pytest

import nr_rate_match_reference as rr


@pytest.mark.parametrize("bg, ncb, want", [
    (1, 25344, [0, 6528, 12672, 21504]),       # Ncb = N: 17, 33, 56 times Zc
    (2, 19200, [0, 4992, 9600, 16512]),        # 13, 25, 43 times Zc
    (1, 16896, [0, 4224, 8448, 14208]),        # limited buffer, two thirds of N: floor(a Ncb / N) = 11, 22, 37
])
def test_k0_equals_the_published_table(bg, ncb, want):
    c = rr.Config(bg, 384, 0, ncb)
    assert [c.k0(rv) for rv in range(4)] == want


@pytest.mark.parametrize("bg, zc, fillers, ncb", [(1, 2, 0, None), (2, 2, 4, None), (2, 3, 7, None), (1, 3, 5, 150), (2, 2, 4, 56)])
def test_one_turn_of_the_buffer_sends_every_column_once_in_order(bg, zc, fillers, ncb):
    c = rr.Config(bg, zc, fillers, ncb)
    sel = c.selection(c.L, 0)
    want = [col for col in range(2 * zc, 2 * zc + c.ncb) if not c.k - fillers <= col < c.k]
    assert sel.tolist() == want and len(want) == c.L
    assert np.array_equal(c.transmitted(c.L, 0, 1), sel), "Qm = 1 is no interleaver"


@pytest.mark.parametrize("rv", range(4))
@pytest.mark.parametrize("e", [6, 48, 96, 102, 250])
def test_repeat_counts_sum_to_e(rv, e):
    c = rr.Config(2, 2, 4, 93)
    rep = c.repeats(e, rv)
    assert rep.sum() == e
    assert rep[:2 * c.zc].sum() == 0 and rep[c.k - c.fillers:c.k].sum() == 0 and rep[2 * c.zc + c.ncb:].sum() == 0
    sent = np.delete(rep[2 * c.zc:2 * c.zc + c.ncb], np.arange(c.k - 2 * c.zc - c.fillers, c.k - 2 * c.zc))
    assert sent.max() - sent.min() <= 1, "a circular read repeats every bit as often as any other, or once more"


@pytest.mark.parametrize("qm", [1, 2, 4, 6, 8])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_match_then_recover_returns_the_signs(qm, dtype):
    c = rr.Config(1, 2, 3)
    cws = np.random.default_rng(5).integers(0, 2, (3, c.n), dtype=np.uint8)
    e = 24 * 7                                 # more than L = 129: some columns twice
    for rv in range(4):
        tx = c.match(cws, e, rv, qm)
        assert tx.shape == (3, e) and set(np.unique(tx)) <= {0, 1}
        rx = (1.0 - 2.0 * tx).astype(dtype)    # a positive LLR means bit 0
        llrs = c.recover(rx, rv, qm, 20.0)
        rep = c.repeats(e, rv)
        assert llrs.dtype == dtype and np.array_equal(llrs[:, rep > 0], ((1.0 - 2.0 * cws) * rep)[:, rep > 0])
        idle = (rep == 0) & ~((np.arange(c.n) >= c.k - 3) & (np.arange(c.n) < c.k))
        assert (llrs[:, idle] == 0).all() and (llrs[:, c.k - 3:c.k] == 20.0).all()


def test_interleaver_is_the_row_column_one():
    c = rr.Config(2, 2)
    sel, f = c.selection(12, 0), c.transmitted(12, 0, 4)
    assert f.tolist() == sel.reshape(4, 3).T.reshape(-1).tolist()


def test_combining_adds_and_fillers_are_overwritten():
    c = rr.Config(2, 2, 4)
    rx = np.arange(1, 41, dtype=np.float32)[None, :]
    first = c.recover(rx, 0, 2, np.inf)
    both = c.recover(rx, 2, 2, 20.0, old=first)
    rep0, rep2 = c.repeats(40, 0), c.repeats(40, 2)
    assert (both[0, c.k - 4:c.k] == 20.0).all() and np.isinf(first[0, c.k - 4:c.k]).all()
    keep = (rep2 == 0)
    keep[c.k - 4:c.k] = False
    assert np.array_equal(both[0, keep], first[0, keep]) and (both[0, (rep0 > 0) & (rep2 > 0)] > first[0, (rep0 > 0) & (rep2 > 0)]).all()
