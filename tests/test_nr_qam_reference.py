"""CPU: pins the numpy restatement of the NR mapper, demapper and scrambling (tests/nr_qam_reference.py) to TS 38.211 --
the tables of 5.1.3-5.1.6 spelled out, the demapper of the whole 2^QM-point constellation, and properties of the Gold
sequence that the serial LFSR does not assume."""
import numpy as np
import pytest

import demod_restatement as dr
import nr_qam_reference as nq


def test_16qam_points_are_table_5_1_4():
    """d(i) = [(1 - 2 b0)(2 - (1 - 2 b2)) + j (1 - 2 b1)(2 - (1 - 2 b3))] / sqrt(10), written out for b0 b1 b2 b3 = V"""
    table = [(1, 1), (1, 3), (3, 1), (3, 3), (1, -1), (1, -3), (3, -1), (3, -3),
             (-1, 1), (-1, 3), (-3, 1), (-3, 3), (-1, -1), (-1, -3), (-3, -1), (-3, -3)]
    a = np.sqrt(1.0 / 10.0)
    want = np.array([complex(i * a, q * a) for i, q in table])
    assert np.array_equal(nq.points(4), want)


def test_levels_of_every_axis():
    assert nq.levels(1) == [1, -1]
    assert nq.levels(2) == [1, 3, -1, -3]
    assert nq.levels(3) == [3, 1, 5, 7, -3, -1, -5, -7]
    assert nq.levels(4) == [5, 7, 3, 1, 11, 9, 13, 15, -5, -7, -3, -1, -11, -9, -13, -15]
    # 38.211 5.1.5, 64QAM: Re d = (1 - 2 b0)[4 - (1 - 2 b2)[2 - (1 - 2 b4)]]; 5.1.6 adds [8 - ...] and b6
    for b0 in (0, 1):
        for b2 in (0, 1):
            for b4 in (0, 1):
                assert nq.levels(3)[4 * b0 + 2 * b2 + b4] == (1 - 2 * b0) * (4 - (1 - 2 * b2) * (2 - (1 - 2 * b4)))
                for b6 in (0, 1):
                    assert nq.levels(4)[8 * b0 + 4 * b2 + 2 * b4 + b6] == \
                        (1 - 2 * b0) * (8 - (1 - 2 * b2) * (4 - (1 - 2 * b4) * (2 - (1 - 2 * b6))))


@pytest.mark.parametrize("qm", [2, 4, 6, 8])
def test_unit_mean_energy_and_qpsk(qm):
    p = nq.points(qm)
    assert len(p) == 1 << qm and len(set(p.tolist())) == 1 << qm
    assert abs(float((p.real * p.real + p.imag * p.imag).mean()) - 1.0) <= 1e-12
    if qm == 2:
        assert np.array_equal(p.view(np.uint64), dr.QPSK.view(np.uint64)), "QM = 2 is the library's QPSK bit for bit"


def _fold_2d(symbols, sigma, pts, step):
    """the demapper of the whole constellation, literally: d_V = sr re_V + si im_V - half |p_V|^2 over all 2^QM points, bit j
    of V = sum_j b_j << (QM-1-j), left folds over ascending V.  -> (llrs [S][QM], max |d|)"""
    qm = len(pts).bit_length() - 1
    scale = 1.0 / (sigma * sigma)
    half = 0.5 * scale
    sr, si = symbols.real * scale, symbols.imag * scale
    d = [sr * p.real + si * p.imag - half * (p.real * p.real + p.imag * p.imag) for p in pts]
    out = []
    for j in range(qm):
        acc = [None, None]
        for v in range(len(pts)):
            b = (v >> (qm - 1 - j)) & 1
            acc[b] = d[v] if acc[b] is None else step(acc[b], d[v])
        out.append(acc[0] - acc[1])
    return np.stack(out, axis=-1), float(np.max(np.abs(np.stack(d))))


@pytest.mark.parametrize("qm", [4, 2, 6, 8])
@pytest.mark.parametrize("max_log", [False, True])
def test_separable_llrs_equal_the_two_dimensional_fold(qm, max_log):
    """The bit-j sum over the 2-D set factorises and the other axis cancels: the per-axis LLRs are the whole
    constellation's, up to rounding.  Bound: 2^-44 * max(1, max |d|) -- at most 2^QM + 2 roundings of 2^-53 relative to the
    largest d, at most 2^9 of them."""
    rng = np.random.default_rng(100 + qm)
    pts = nq.points(qm)
    n = 4000
    worst = 0.0
    for sigma in (1.0, 0.3, 0.05):
        tx = pts[rng.integers(0, len(pts), n)]
        sym = tx + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        got = nq.demodulate(sym[None, :], sigma, qm, max_log=max_log).reshape(n, qm)
        want, dmax = _fold_2d(sym, sigma, pts, nq.maxnum if max_log else nq.maxstar)
        err = float(np.max(np.abs(got - want)))
        bound = 2.0 ** -44 * max(1.0, dmax)
        worst = max(worst, err / max(1.0, dmax))
        assert err <= bound, (qm, max_log, sigma, err, bound)
    print(f"QM {qm} max_log {max_log}: worst difference {worst:.2e} relative to max(1, max |d|)")


def test_round_trip_and_scrambling_of_the_restatement():
    rng = np.random.default_rng(5)
    for qm in (2, 4, 6, 8):
        bits = rng.integers(0, 2, (2, 12 * qm)).astype(np.uint8)
        for c_init in (-1, 0x1234567):
            sym = nq.modulate(bits, qm, c_init)
            llrs = nq.demodulate(sym, 0.05, qm, c_init=c_init)
            assert np.array_equal((llrs < 0).astype(np.uint8), bits)
        c = nq.gold(0x1234567, 12 * qm)
        assert np.array_equal(nq.modulate(bits, qm, 0x1234567), nq.modulate(bits ^ c, qm))


def test_c_init_zero_is_the_x1_sequence():
    """x2 = 0 throughout: c(n) = x1(n + 1600), and x1 is c_init-free"""
    x1 = [1] + [0] * 30
    for n in range(1600 + 500):
        x1.append(x1[n + 3] ^ x1[n])
    assert nq.gold(0, 500).tolist() == x1[1600:2100]
    assert not np.array_equal(nq.gold(1, 500), nq.gold(0, 500))


def _mulmod(a, b, poly):
    """a b mod x^31 + poly over GF(2), Python integers as polynomials"""
    p = 0
    for i in range(31):
        if (b >> i) & 1:
            p ^= a << i
    for d in range(p.bit_length() - 1, 30, -1):
        if (p >> d) & 1:
            p ^= (1 << d) ^ (poly << (d - 31))
    return p


def _xpow(e, poly):
    r, base = 1, 2
    while e:
        if e & 1:
            r = _mulmod(r, base, poly)
        base = _mulmod(base, base, poly)
        e >>= 1
    return r


def test_period_by_jump_ahead():
    """c has period 2^31 - 1: x^(2^31 - 1) = 1 modulo both feedback polynomials (and no smaller power of the prime 2^31 - 1's
    divisors -- it is prime, so x != 1 suffices).  The jump-ahead is checked against the serial LFSR on the way: the state
    at offset n is x^n applied to the first 61 bits."""
    for poly, taps in ((0b1001, (3, 0)), (0b1111, (3, 2, 1, 0))):
        assert _xpow((1 << 31) - 1, poly) == 1 and _xpow(1, poly) != 1
        rng = np.random.default_rng(poly)
        seq = [int(b) for b in rng.integers(0, 2, 31)]
        for n in range(3000):
            seq.append(sum(seq[n + t] for t in taps) & 1)
        for n in (31, 1600, 2900):
            r = _xpow(n, poly)
            for k in range(31):
                assert sum(((r >> i) & 1) * seq[k + i] for i in range(31)) & 1 == seq[n + k]
        # ... and therefore at offset n + (2^31 - 1) the state is the one at n
        assert _xpow(1600 + (1 << 31) - 1, poly) == _xpow(1600, poly)
