"""CPU: the numpy restatement of the 8-bit soft-bit receive path (tests/nr_soft_i8_restatement.py) pinned on its own, so
that the GPU tests compare the library with something that has been checked:
(a) where no partial sum leaves +-127 it is `nr_rate_match_reference.Config.recover` on the same integers in float32;
(b) hand-worked saturating columns, where the order of the sums shows;
(c) -128 reads as -127, in the received row and in the old buffer;
and the quantiser against hand-worked values."""
import numpy as np

import nr_rate_match_reference as rr
import nr_soft_i8_restatement as sr

CASES = [(60, 0, 1), (104, 2, 2), (208, 0, 4), (372, 1, 6), (6656, 1, 8)]          # (E, rv, Qm) on nr5g:2:2:4:93


def test_quantise_by_hand():
    x = np.array([0.0, -0.0, 0.0624, 0.0625, -0.0625, 0.1875, -0.1875, 0.3125, 1.0, -1.0, 15.8, 15.8124, 15.8125, 15.875, 16.0, 1e9, -15.8125, -1e9,
                  np.inf, -np.inf, np.nan], dtype=np.float32)
    want = [0, 0, 0, 1, -1, 2, -2, 3, 8, -8, 126, 126, 127, 127, 127, 127, -127, -127, 127, -127, 0]
    assert sr.quantise(x).tolist() == want and sr.quantise(x).dtype == np.int8
    assert sr.quantise(x.astype(np.float64)).tolist() == want
    # Q(clip(v) / 8) = clip(v) for all 256 bytes
    v = np.arange(-128, 128).astype(np.int8)
    assert np.array_equal(sr.quantise(sr.dequantise(v)), sr.clip(v).astype(np.int8))
    assert sr.clip(v).min() == -127 and sr.clip(v).max() == 127 and sr.clip(np.int8(-128)) == -127


def test_equals_the_float_recovery_where_nothing_saturates():
    """(a) inputs |v| <= 127 // (max repeats + 1): a column's sum over one transmission, and on top of an old value of the
    same bound, stays within +-127"""
    cfg = rr.Config(2, 2, 4, 93)
    rng = np.random.default_rng(11)
    for e, rv, qm in CASES:
        bound = 127 // (int(cfg.repeats(e, rv).max()) + 1)
        assert bound >= 1
        rx = rng.integers(-bound, bound + 1, size=(3, e)).astype(np.int8)
        old = rng.integers(-bound, bound + 1, size=(3, cfg.n)).astype(np.int8)
        sat = np.zeros((3, cfg.n), dtype=bool)
        got = sr.recover_i8(cfg, rx, rv, qm, 127, saturated=sat)
        want = cfg.recover(rx.astype(np.float32), rv, qm, 127.0)
        assert not sat.any() and np.array_equal(got.astype(np.float32), want), (e, rv, qm)
        got = sr.recover_i8(cfg, rx, rv, qm, 55, old=old, saturated=sat)
        want = cfg.recover(rx.astype(np.float32), rv, qm, 55.0, old=old.astype(np.float32))
        assert not sat.any() and np.array_equal(got.astype(np.float32), want), (e, rv, qm)
        assert (got[:, cfg.k - 4:cfg.k] == 55).all(), "a filler column is the filler whatever the old value"


def test_saturating_columns_by_hand():
    """(b) nr5g:2:2 without fillers, Ncb = N = 100, rv 0, Qm 1, E = 300: column 4 + d is carried by selection indices d,
    d + 100, d + 200, which are also its transmitted positions"""
    cfg = rr.Config(2, 2)
    assert (cfg.n, cfg.N, cfg.L) == (104, 100, 100)
    rx = np.zeros((1, 300), dtype=np.int8)
    rx[0, [0, 100, 200]] = [100, 100, -100]             # clip(clip(100 + 100) - 100) = 27, not 100
    rx[0, [1, 101, 201]] = [-100, 100, 100]             # 100
    rx[0, [2, 102, 202]] = [-100, -100, 100]            # -27
    rx[0, [3, 103, 203]] = [127, 127, 127]              # 127
    rx[0, [4, 104, 204]] = [50, 50, 26]                 # 126: nothing saturates
    sat = np.zeros((1, 104), dtype=bool)
    got = sr.recover_i8(cfg, rx, 0, 1, saturated=sat)
    assert got[0, 4:9].tolist() == [27, 100, -27, 127, 126] and sat[0, 4:9].tolist() == [True, False, True, True, False]
    assert (got[0, :4] == 0).all() and (got[0, 9:] == 0).all()
    # combining: clip(clip(old) + S)
    old = np.zeros((1, 104), dtype=np.int8)
    old[0, 4:9] = [100, 100, -100, -128, 1]
    old[0, 0] = -128                                    # R = 0: clip(old)
    got2 = sr.recover_i8(cfg, rx, 0, 1, old=old)
    assert got2[0, 4:9].tolist() == [127, 127, -127, 0, 127] and got2[0, 0] == -127


def test_minus_128_reads_as_minus_127():
    """(c) in the received row: -128 + 1 = -126 after the clip, where a sign-extended -128 would give -127; alone: -127"""
    cfg = rr.Config(2, 2)
    rx = np.zeros((1, 200), dtype=np.int8)
    rx[0, [0, 100]] = [-128, 1]
    rx[0, 1] = -128
    rx[0, [2, 102]] = [-128, -128]
    got = sr.recover_i8(cfg, rx, 0, 1)
    assert got[0, 4:7].tolist() == [-126, -127, -127]
    assert sr.dequantise(np.int8(-128)) == np.float32(-15.875)
