"""GPU: the simulator with an NR modulation (ldpc_toolbox_sim_set_nr_qam) on nr5g:2:16 (n = 832, k = 160), plain min-sum,
rate-matched to E = 480.  The generator is compared with the restated chain (tests/nr_qam_reference.py: mapper, AWGN,
f64 demapper) bit for bit; the counters with a CPU pipeline -- the simulator's own frames, the numpy restatement's recovery
(tests/nr_rate_match_reference.py), the decoder, the XOR with the pooled message."""
import numpy as np
import pytest

import ldpc_toolbox_amd as lt
import nr_qam_reference as nq
import nr_rate_match_reference as rr
from demod_restatement import same_bits
from ldpc_toolbox_amd import _capi, ber
from ldpc_toolbox_amd import simulation as sim

pytestmark = pytest.mark.gpu

CODE = "nr5g:2:16"
N, K, E = 832, 160, 480
MAX_ITER = 30
POOL, POOL_SEED = 16, 5


@pytest.fixture(scope="module")
def setup():
    alist = lt.code_alist(CODE)
    s = lt.Simulator(alist, "Minsumf32", device=0, pool_size=POOL, pool_seed=POOL_SEED)
    dec = lt.LdpcDecoder(alist, "Minsumf32", device=0)
    rm = lt.NrRateMatcher(CODE)
    ref = rr.Config(2, 16)
    qams = {qm: lt.NrQam(qm) for qm in (2, 4, 6, 8)}
    yield s, dec, rm, ref, alist, qams
    for x in (s, dec, rm) + tuple(qams.values()):
        x.close()


@pytest.mark.parametrize("max_log", [False, True])
@pytest.mark.parametrize("qm", [4, 6, 8])
def test_generate_equals_the_restated_chain(setup, qm, max_log):
    """(a) 70 frames; the pool rows are what the rate matcher left"""
    s, dec, rm, ref, alist, qams = setup
    ebn0_db, seed, first, frames = 2.0 + qm, 31, (1 << 32) - 30, 70
    s.set_rate_match(rm, E, 0, qm)
    try:
        before = s.pool_data()[1]
        s.set_nr_qam(qams[qm], max_log)
        assert (s.get("nr_qam"), s.get("modulation"), s.get("max_log"), s.get("constellation"), s.bits_per_symbol) == (1, qm, int(max_log), 0, qm)
        msgs, tx = s.pool_data()
        assert tx.shape == (POOL, E) and np.array_equal(tx, before), "set_nr_qam leaves the pool rows alone"
        got, idx = s.generate(ebn0_db, seed, first, frames)
        sigma = sim.noise_sigma(s.rate, ebn0_db, qm)
        want = nq.simulator_llrs(tx[idx], qm, sigma, seed, first, max_log)
        assert got.shape == (frames, E) and (got > 0).any() and (got < 0).any()
        assert same_bits(got, want), (qm, max_log)
    finally:
        s.set_nr_qam(None)
        s.set_rate_match(None)
    assert (s.get("nr_qam"), s.get("modulation"), s.n_tx) == (0, 1, N)


EBN0_64QAM = 4.5


def test_counters_equal_the_cpu_pipeline(setup):
    """(b) QM = 6, E = 480 (rate 1/3, 80 symbols of 64QAM) at 4.5 dB, chosen on a 0.5 dB grid from one GPU run of these 256
    frames: 256, 253, 251, 243, 219, 166, 99, 48, 14, 0 frame errors at 1.5, 2, ... 6 dB.  At 4.5 dB 156 converge and 100
    do not (counters [256, 2322, 99, 0, 4862, 1892])."""
    s, dec, rm, ref, alist, qams = setup
    qm, ebn0_db, seed, first, frames = 6, EBN0_64QAM, 31, 100, 256
    s.set_rate_match(rm, E, 0, qm)
    s.set_nr_qam(qams[qm])
    try:
        msgs, tx = s.pool_data()
        rx, idx = s.generate(ebn0_db, seed, first, frames)
        assert rx.shape == (frames, E)
        llrs = ref.recover(rx, 0, qm, np.inf)
        bits, its, _ = dec.decode_batch(llrs, MAX_ITER)
        errs = (bits[:, :K] != msgs[idx]).sum(axis=1)
        used = np.where(its >= 0, its, MAX_ITER)
        want = [frames, int(errs.sum()), int((errs > 0).sum()), int(((errs > 0) & (its >= 0)).sum()), int(used.sum()),
                int(used[errs == 0].sum())]
        print(f"64QAM, E = {E} at {ebn0_db} dB: {int((its >= 0).sum())} of {frames} converge; counters {want}")
        assert (its >= 0).sum() >= 30 and (its < 0).sum() >= 30, "the point must have converging and failing frames"
        assert s.run(ebn0_db, seed, first, frames, MAX_ITER).tolist() == want
    finally:
        s.set_nr_qam(None)
        s.set_rate_match(None)


def test_counters_do_not_depend_on_pooling(setup):
    """(c) several chunks a little above the waterfall: the stragglers go through the pool"""
    s, dec, rm, ref, alist, qams = setup
    frames = 2 * s.get("preferred_batch") + 5
    s.set_rate_match(rm, E, 0, 6)
    s.set_nr_qam(qams[6], True)
    try:
        got = {}
        for pooling in (0, 1):
            s.set("pooling", pooling)
            got[pooling] = (s.run(EBN0_64QAM + 1.0, 7, 0, frames, MAX_ITER), s.get("pooled_frames"))
        print(f"{frames} frames: {got[0][0].tolist()}; {got[1][1]} frames through the pool")
        assert got[0][1] == 0 and np.array_equal(got[0][0], got[1][0]) and got[0][0][0] == frames and got[0][0][2] > 0
    finally:
        s.set("pooling", 1)
        s.set_nr_qam(None)
        s.set_rate_match(None)


def test_stragglers_are_pooled(setup):
    """(c) with 200 iterations, far more than the converging frames need, later calls run a reduced budget and pool the
    stragglers"""
    s, dec, rm, ref, alist, qams = setup
    chunk = s.get("preferred_batch")
    s.set_rate_match(rm, E, 0, 6)
    s.set_nr_qam(qams[6])
    try:
        got = {}
        for pooling in (0, 1):
            s.set("pooling", pooling)
            total, pooled = np.zeros(6, dtype=np.int64), 0
            for call in range(3):
                total += s.run(EBN0_64QAM + 1.0, 7, chunk * call, chunk, 200)
                pooled += s.get("pooled_frames")
            got[pooling] = (total, pooled)
        print(f"pooling 0: {got[0][0].tolist()}; pooling 1: {got[1][0].tolist()}, {got[1][1]} frames through the pool")
        assert got[0][1] == 0 and got[1][1] > 0, "the second configuration must actually pool"
        assert np.array_equal(got[0][0], got[1][0]) and got[0][0][2] > 0
    finally:
        s.set("pooling", 1)
        s.set_nr_qam(None)
        s.set_rate_match(None)


def test_setting_clearing_and_refusals(setup):
    """(d)"""
    s, dec, rm, ref, alist, qams = setup
    L = _capi.lib()
    before = s.run(2.0, 31, 100, 64, MAX_ITER)
    # n_tx = 832 = 2^6 * 13: QM 2, 4, 8 divide it, 6 does not
    with pytest.raises(ValueError, match="multiple of QM"):
        s.set_nr_qam(qams[6])
    assert (s.get("nr_qam"), s.get("modulation")) == (0, 1)
    assert np.array_equal(s.run(2.0, 31, 100, 64, MAX_ITER), before), "a refusal changes nothing"
    il = lt.Simulator(alist, "Minsumf32", device=0, pool_size=2, modulation="QPSK", interleaving=4)
    with pytest.raises(ValueError, match="interleaving"):
        il.set_nr_qam(qams[2])
    assert (il.get("nr_qam"), il.get("constellation")) == (0, 1)
    il.close()
    # set_nr_qam clears a constellation and the other way round; None restores "modulation"
    qpsk = lt.Demodulator("QPSK", device=0)
    s.set_constellation(qpsk, True)
    as_qpsk = s.run(2.0, 31, 100, 64, MAX_ITER)
    s.set_nr_qam(qams[4])
    assert (s.get("nr_qam"), s.get("constellation"), s.get("modulation"), s.get("max_log")) == (1, 0, 4, 0)
    as_16qam = s.run(2.0, 31, 100, 64, MAX_ITER)
    assert L.ldpc_toolbox_sim_set(s._h, b"interleaving", 4) == -1 and "interleaving" in _capi.last_error()
    assert s.get("interleaving") == 0
    s.set_constellation(qpsk, True)
    assert (s.get("nr_qam"), s.get("constellation"), s.get("modulation"), s.get("max_log")) == (0, 1, 2, 1)
    assert np.array_equal(s.run(2.0, 31, 100, 64, MAX_ITER), as_qpsk)
    s.set_nr_qam(qams[2], True)
    assert (s.get("nr_qam"), s.get("constellation"), s.get("modulation"), s.get("max_log")) == (1, 0, 2, 1)
    s.set_nr_qam(None)
    assert (s.get("nr_qam"), s.get("constellation"), s.get("modulation")) == (0, 0, 1)
    assert np.array_equal(s.run(2.0, 31, 100, 64, MAX_ITER), before), "None restores the earlier counters"
    assert not np.array_equal(as_16qam, before) and not np.array_equal(as_16qam, as_qpsk)
    qpsk.close()
    # with a rate matcher: E must stay a multiple of QM, and the matcher cannot go while n is none
    s.set_rate_match(rm, E, 0, 6)
    s.set_nr_qam(qams[6])
    with pytest.raises(ValueError, match="bits per symbol"):
        s.set_rate_match(rm, 482, 0, 1)
    with pytest.raises(ValueError, match="clear that first"):
        s.set_rate_match(None)
    assert (s.n_tx, s.get("nr_qam"), s.get("rate_match")) == (E, 1, 1)
    s.set_nr_qam(None)
    s.set_rate_match(None)
    assert np.array_equal(s.run(2.0, 31, 100, 64, MAX_ITER), before)


def test_ber_driver_with_an_nr_modulation(setup, tmp_path, capsys):
    """(e)"""
    s, dec, rm, ref, alist, qams = setup
    path = tmp_path / "qam.txt"
    lo, hi = EBN0_64QAM, EBN0_64QAM + 1.0
    args = ["--code", CODE, "--decoder", "Minsumf32", "--min-ebn0", str(lo), "--max-ebn0", str(hi), "--step-ebn0", "1", "--max-iter", str(MAX_ITER),
            "--max-frames", "256", "--frames-per-batch", "256", "--frame-errors", "100000", "--seed", "4", "--pool-size", str(POOL),
            "--nr-rate-match", "480:0:6", "--nr-qam", "6", "--output-file", str(path)]
    res = ber.main(args)
    capsys.readouterr()
    text = path.read_text()
    assert len(res) == 2 and "Frame size (N): 480" in text and "NR rate matching (E[:RV[:QM]]): 480:0:6" in text
    assert " - Modulation: NR 64QAM\n - Bits per symbol: 6\n" in text and "max-log" not in text
    rows = [[c.strip() for c in line.split("|")] for line in text.strip().splitlines()[-2:]]
    own = lt.Simulator(alist, "Minsumf32", device=0, pool_size=POOL, pool_seed=5)
    own.set_rate_match(rm, E, 0, 6)
    own.set_nr_qam(qams[6])
    for row, ebn0_db in zip(rows, (lo, hi)):
        counters = own.run(ebn0_db, ber.point_seed(4, ebn0_db), 0, 256, MAX_ITER)
        assert [int(row[1]), int(row[2]), int(row[3]), int(row[4])] == counters[:4].tolist()
    own.close()
    assert int(rows[0][3]) > int(rows[1][3]) > 0, "frame errors fall with Eb/N0"
    ber.main(args[:-2] + ["--max-log", "--output-file", str(path)])
    assert " - Demodulator: max-log" in path.read_text()
    for extra in (["--modulation", "QPSK"], ["--interleaving", "4"], ["--constellation", str(path)]):
        with pytest.raises(SystemExit):
            ber.main(args + extra)
    with pytest.raises(SystemExit):
        ber.main(args[:-6] + ["--nr-qam", "6"])        # n_tx = 832 is no multiple of 6
    with pytest.raises(SystemExit):
        ber.main(args[:-4] + ["--nr-qam", "5"])
    capsys.readouterr()
