"""GPU: the simulator over the Rayleigh block-fading channel ("fading_block" of ldpc_toolbox_sim_set; include/ldpc_toolbox.h,
PART 10) on nr5g:2:16 (n = 832, k = 160) with a rate matcher, the set-up of tests/test_sim_nr_qam_gpu.py: pool 16 with seed
5, 30 iterations, E = 480.

The generators are compared bit for bit with the DEFINED RESULT restated (tests/nr_csi_restatement.py: the f64 mapper, the
f64 fading channel, the f64 demapper with the channel's scales, each LLR rounded once to float); a HARQ process is one
concatenated row through that channel.  The counters are compared with themselves under "pooling", chunking and, for
run_harq, at either "soft_bits"."""
import numpy as np
import pytest

import ldpc_toolbox_amd as lt
import nr_csi_restatement as nc
import nr_rate_match_reference as rr
from demod_restatement import same_bits
from ldpc_toolbox_amd import _capi
from ldpc_toolbox_amd import simulation as sim

pytestmark = pytest.mark.gpu

CODE = "nr5g:2:16"
N, K, E = 832, 160, 480
MAX_ITER = 30
POOL, POOL_SEED = 16, 5
# E = 480, 96, 96: 80, 16, 16 symbols of 64QAM and 240, 48, 48 of QPSK; with 7 symbols per gain the blocks 77 .. 83 and
# 91 .. 97 (64QAM), 238 .. 244 and 287 .. 293 (QPSK) of the concatenated row straddle the two seams
SEQ = [(480, 0), (96, 2), (96, 3)]
HARQ_BLOCK = 7
# Eb/N0 per QM, chosen on a 1 dB grid from one GPU run of frames 100 .. 611 (seed 7, max-log, 5 symbols per gain), frame
# errors of AWGN / fading:  QPSK 2 dB 63 / 382, 3 dB 0 / 191, 4 dB 0 / 58, 5 dB 0 / 12, 6 dB 0 / 0;
# 64QAM 6 dB 7 / 288, 7 dB 0 / 147, 8 dB 0 / 56, 9 dB 0 / 17, 10 dB 0 / 1, 11 dB 0 / 0.  At the chosen points AWGN delivers
# every frame and fading fails 12 and 17 of 512 (counters [512, 531, 12, 0, 3631, 3271] and [512, 483, 17, 0, 3617, 3107]).
# The HARQ runs are 3 dB lower: at 6 dB, 64QAM with 7 symbols per gain, 301 of 512 frames stop after the first
# transmission, 142 of 211 after the second (145 with 8-bit soft buffers) and 6 fail after all three.
EBN0 = {2: 5.0, 6: 9.0}


@pytest.fixture(scope="module")
def setup():
    alist = lt.code_alist(CODE)
    s = lt.Simulator(alist, "Minsumf32", device=0, pool_size=POOL, pool_seed=POOL_SEED)
    rm = lt.NrRateMatcher(CODE)
    ref = rr.Config(2, 16)
    qams = {qm: lt.NrQam(qm) for qm in (2, 6)}
    codewords = s.pool_data()[1].copy()
    assert (s.n, s.k, s.n_tx, codewords.shape, s.get("fading_block")) == (N, K, N, (POOL, N), 0)
    yield s, rm, ref, alist, qams, codewords
    for x in (s, rm) + tuple(qams.values()):
        x.close()


def clear(s):
    s.set("fading_block", 0)
    s.set("pooling", 1)
    s.set_nr_qam(None)
    s.set_rate_match(None)


@pytest.mark.parametrize("max_log", [False, True], ids=["exact", "max-log"])
@pytest.mark.parametrize("qm", [2, 6])
def test_generate_equals_the_defined_result(setup, qm, max_log):
    """8 frames from frame 3 on, 5 symbols per gain and one gain for the whole row; one call or two; and the key set back to 0
    gives the AWGN frames recorded before it was set"""
    s, rm, ref, alist, qams, codewords = setup
    ebn0_db, seed, first, frames = EBN0[qm], 31, 3, 8
    s.set_rate_match(rm, E, 0, qm)
    s.set_nr_qam(qams[qm], max_log)
    try:
        tx = s.pool_data()[1]
        sigma = sim.noise_sigma(s.rate, ebn0_db, qm)
        awgn, awgn_idx = s.generate(ebn0_db, seed, first, frames)
        for block in (5, E // qm + 1000):
            s.set("fading_block", block)
            assert s.get("fading_block") == block
            got, idx = s.generate(ebn0_db, seed, first, frames)
            assert np.array_equal(idx, awgn_idx), "the channel does not change which pooled row a frame sends"
            want = nc.simulator_llrs(tx[idx], qm, sigma, seed, first, block, max_log)
            assert got.shape == (frames, E) and (got > 0).any() and (got < 0).any()
            assert same_bits(got, want), (qm, max_log, block)
            assert not same_bits(got, awgn)
            a, b = s.generate(ebn0_db, seed, first, 3), s.generate(ebn0_db, seed, first + 3, frames - 3)
            assert same_bits(np.concatenate([a[0], b[0]]), got) and np.array_equal(np.concatenate([a[1], b[1]]), idx)
        s.set("fading_block", 0)
        assert s.get("fading_block") == 0
        again, again_idx = s.generate(ebn0_db, seed, first, frames)
        assert same_bits(again, awgn) and np.array_equal(again_idx, awgn_idx), "0 restores the AWGN frames"
    finally:
        clear(s)


@pytest.mark.parametrize("max_log", [False, True], ids=["exact", "max-log"])
@pytest.mark.parametrize("qm", [2, 6])
def test_generate_harq_is_the_concatenated_row_through_the_channel(setup, qm, max_log):
    s, rm, ref, alist, qams, codewords = setup
    ebn0_db, seed, first, frames = EBN0[qm], 31, 3, 8
    assert (E // qm) % HARQ_BLOCK != 0 and ((E + 96) // qm) % HARQ_BLOCK != 0, "a gain block straddles each seam"
    s.set_rate_match(rm, E, 0, qm)
    s.set_nr_qam(qams[qm], max_log)
    try:
        s.set_harq(rm, SEQ, qm)
        s.set("fading_block", HARQ_BLOCK)
        sigma = sim.noise_sigma(s.rate, ebn0_db, qm)
        plain, plain_idx = s.generate(ebn0_db, seed, first, frames)
        rows = np.concatenate([ref.match(codewords, e, rv, qm) for e, rv in SEQ], axis=1)
        want = nc.simulator_llrs(rows[plain_idx], qm, sigma, seed, first, HARQ_BLOCK, max_log)
        offset = 0
        for t, (e, rv) in enumerate(SEQ):
            got, idx = s.generate_harq(ebn0_db, seed, first, frames, t)
            assert np.array_equal(idx, plain_idx) and got.shape == (frames, e)
            assert same_bits(got, want[:, offset:offset + e]), (qm, max_log, t)
            if t == 0:
                assert same_bits(got, plain), "transmission 0 is what generate returns"
            offset += e
    finally:
        s.set("fading_block", 0)
        s.set_nr_qam(None)
        s.set_harq(None)


def four_calls(fn, first, frames):
    parts = [fn(first + i * (frames // 4), frames // 4) for i in range(4)]
    return [sum(p[j] for p in parts) for j in range(len(parts[0]))]


@pytest.mark.parametrize("qm", [2, 6])
def test_run_counters_do_not_depend_on_pooling_or_chunking(setup, qm):
    s, rm, ref, alist, qams, codewords = setup
    ebn0_db, seed, first, frames = EBN0[qm], 7, 100, 512
    s.set_rate_match(rm, E, 0, qm)
    s.set_nr_qam(qams[qm], True)
    try:
        awgn = s.run(ebn0_db, seed, first, frames, MAX_ITER)
        s.set("fading_block", 5)
        got = {}
        for pooling in (0, 1):
            s.set("pooling", pooling)
            got[pooling] = s.run(ebn0_db, seed, first, frames, MAX_ITER)
            got[pooling, "four"] = four_calls(lambda f0, nf: (s.run(ebn0_db, seed, f0, nf, MAX_ITER),), first, frames)[0]
        print(f"QM {qm}, {ebn0_db} dB, 5 symbols per gain: {got[0].tolist()}; AWGN: {awgn.tolist()}")
        for other in (got[1], got[0, "four"], got[1, "four"]):
            assert other.tolist() == got[0].tolist()
        assert got[0][0] == frames and 0 < got[0][2] < frames, "the point must have converging and failing frames"
        assert got[0][2] > awgn[2], "at one average Eb/N0 fading costs frames"
    finally:
        clear(s)


@pytest.mark.parametrize("soft_bits", [32, 8])
def test_run_harq_counters_do_not_depend_on_pooling_or_chunking(soft_bits):
    """64QAM, E = 480, 96, 96, 7 symbols per gain, Minsumi8Offset (the implementation both "soft_bits" take)"""
    alist = lt.code_alist(CODE)
    s = lt.Simulator(alist, "Minsumi8Offset", device=0, pool_size=POOL, pool_seed=POOL_SEED)
    rm, qam = lt.NrRateMatcher(CODE), lt.NrQam(6)
    ebn0_db, seed, first, frames = EBN0[6] - 3.0, 7, 100, 512
    try:
        s.set_rate_match(rm, E, 0, 6)
        s.set_nr_qam(qam)
        s.set_harq(rm, SEQ, 6)
        s.set("fading_block", HARQ_BLOCK)
        s.set("soft_bits", soft_bits)
        got = {}
        for pooling in (0, 1):
            s.set("pooling", pooling)
            got[pooling] = s.run_harq(ebn0_db, seed, first, frames, MAX_ITER)
            got[pooling, "four"] = four_calls(lambda f0, nf: s.run_harq(ebn0_db, seed, f0, nf, MAX_ITER), first, frames)
        print(f"soft_bits {soft_bits}: {got[0][0].tolist()}; per_tx {got[0][1].tolist()}")
        for other in (got[1], got[0, "four"], got[1, "four"]):
            assert other[0].tolist() == got[0][0].tolist() and other[1].tolist() == got[0][1].tolist()
        counters, per_tx = got[0]
        assert counters[0] == frames and per_tx[0][0] == frames and 0 < per_tx[1][0] < frames, "some frames need a second transmission"
        assert (per_tx[1:, 0] == (per_tx[:-1, 0] - per_tx[:-1, 1])).all(), "who does not stop goes on"
    finally:
        for x in (s, rm, qam):
            x.close()


def test_ber_driver_with_a_fading_block(setup, tmp_path, capsys):
    from ldpc_toolbox_amd import ber
    s, rm, ref, alist, qams, codewords = setup
    path = tmp_path / "fading.txt"
    ebn0_db = EBN0[6]
    args = ["--code", CODE, "--decoder", "Minsumf32", "--min-ebn0", str(ebn0_db), "--max-ebn0", str(ebn0_db), "--step-ebn0", "1", "--max-iter",
            str(MAX_ITER), "--max-frames", "256", "--frames-per-batch", "256", "--frame-errors", "100000", "--seed", "4", "--pool-size", str(POOL),
            "--nr-rate-match", "480:0:6", "--nr-qam", "6", "--output-file", str(path)]
    ber.main(args)
    plain = path.read_text()
    assert "fading" not in plain.lower()
    ber.main(args + ["--nr-fading-block", "5"])
    capsys.readouterr()
    text = path.read_text()
    line = " - Fading: Rayleigh block fading with perfect CSI, 5 symbols per block\n"
    assert " - Bits per symbol: 6\n" + line in text and text.replace(line, "").split("\n\n")[0] == plain.split("\n\n")[0], "one more header line"
    row = [c.strip() for c in text.strip().splitlines()[-1].split("|")]
    own = lt.Simulator(alist, "Minsumf32", device=0, pool_size=POOL, pool_seed=5)
    own.set_rate_match(rm, E, 0, 6)
    own.set_nr_qam(qams[6])
    own.set("fading_block", 5)
    counters = own.run(ebn0_db, ber.point_seed(4, ebn0_db), 0, 256, MAX_ITER)
    own.close()
    assert [int(row[1]), int(row[2]), int(row[3]), int(row[4])] == counters[:4].tolist()
    for bad in (args[:-4] + ["--nr-fading-block", "5"], args + ["--nr-fading-block", "-1"], args + ["--nr-fading-block", str(1 << 31)]):
        with pytest.raises(SystemExit):
            ber.main(bad)                       # without --nr-qam; out of range
    capsys.readouterr()


def test_the_key_and_the_refusal_of_the_runs(setup):
    """the setter takes 0 .. 2^31 - 1 whatever the modulation; the runs are refused while there is no NR modulation: -1 with a
    message, the counters as they were"""
    s, rm, ref, alist, qams, codewords = setup
    L = _capi.lib()
    for bad in (-1, 1 << 31, -(1 << 40)):
        assert L.ldpc_toolbox_sim_set(s._h, b"fading_block", bad) == -1 and "fading_block" in _capi.last_error()
        with pytest.raises(ValueError, match="fading_block"):
            s.set("fading_block", bad)
    assert s.get("fading_block") == 0
    before = s.run(2.0, 31, 100, 64, MAX_ITER)
    try:
        for ok in (1, 0x7fffffff, 5):
            assert L.ldpc_toolbox_sim_set(s._h, b"fading_block", ok) == 0 and s.get("fading_block") == ok
        assert s.get("nr_qam") == 0
        counters = np.full(9, 0xAB, dtype=np.uint64)
        per_tx = np.full((3, 4), 0xAB, dtype=np.uint64)
        llrs = np.full((4, N), 7.5, dtype=np.float32)
        idx = np.full(4, 0xAB, dtype=np.uint32)
        calls = {
            "run": lambda: L.ldpc_toolbox_sim_run(s._h, 2.0, 31, 100, 64, MAX_ITER, counters.ctypes.data),
            "run_bch": lambda: L.ldpc_toolbox_sim_run_bch(s._h, 2.0, 31, 100, 64, MAX_ITER, 2, counters.ctypes.data),
            "generate": lambda: L.ldpc_toolbox_sim_generate(s._h, 2.0, 31, 100, 4, llrs.ctypes.data, idx.ctypes.data),
            "run_harq": lambda: L.ldpc_toolbox_sim_run_harq(s._h, 2.0, 31, 100, 64, MAX_ITER, counters.ctypes.data, per_tx.ctypes.data),
            "generate_harq": lambda: L.ldpc_toolbox_sim_generate_harq(s._h, 2.0, 31, 100, 4, 0, llrs.ctypes.data, idx.ctypes.data),
        }
        for with_sequence in (False, True):
            if with_sequence:
                s.set_harq(rm, [(480, 0), (96, 2)], 1)      # (BPSK: a sequence the runs would otherwise take)
            for name, call in calls.items():
                assert call() == -1 and "fading_block needs an NR modulation" in _capi.last_error(), (name, with_sequence)
                assert (counters == 0xAB).all() and (per_tx == 0xAB).all() and (llrs == 7.5).all() and (idx == 0xAB).all(), name
        s.set_harq(None)
        with pytest.raises(RuntimeError, match="fading_block needs an NR modulation"):
            s.run(2.0, 31, 100, 64, MAX_ITER)
        # a constellation is no NR modulation either
        qpsk = lt.Demodulator("QPSK", device=0)
        s.set_constellation(qpsk)
        assert calls["run"]() == -1 and (counters == 0xAB).all()
        s.set_constellation(None)
        qpsk.close()
        s.set("fading_block", 0)
        assert np.array_equal(s.run(2.0, 31, 100, 64, MAX_ITER), before), "0 restores the earlier counters"
    finally:
        s.set("fading_block", 0)
        s.set_harq(None)
