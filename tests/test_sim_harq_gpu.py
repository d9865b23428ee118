"""GPU: the HARQ simulator (ldpc_toolbox_sim_set_harq, _run_harq, _generate_harq) on nr5g:2:16 (n = 832, k = 160), plain
min-sum, 30 iterations, pool 16 with seed 5 -- the set-up of tests/test_sim_rate_match_gpu.py.

The definition restated (include/ldpc_toolbox.h).  A frame's HARQ process is one long transmitted row, the T rate-matched
rows of its pooled codeword concatenated, and the channel's noise for (seed, frame) on that row; transmission t is the slice
[P_t, P_t + E_t) of its LLRs.  The soft buffer is recover(combine = 0) of transmission 0, then recover(combine = 1) of each
later one into the same row; after every transmission the frame is decoded with the full 30 iterations and stops at the
first attempt that converges, or after the last.  The generators are compared bit for bit with the restatements
(tests/channel_restatement.py, tests/nr_qam_reference.py, tests/nr_rate_match_reference.py), the counters with a CPU
pipeline: the simulator's own frames, the numpy recovery, `LdpcDecoder.decode_batch` and the stopping rule."""
import numpy as np
import pytest

import channel_restatement as cr
import ldpc_toolbox_amd as lt
import nr_qam_reference as nq
import nr_rate_match_reference as rr
from demod_restatement import same_bits
from ldpc_toolbox_amd import _capi, ber
from ldpc_toolbox_amd import simulation as sim

pytestmark = pytest.mark.gpu

CODE = "nr5g:2:16"
N, K = 832, 160
MAX_ITER = 30
POOL, POOL_SEED = 16, 5
SEQ = [(480, 0), (96, 2), (96, 3), (96, 1)]


@pytest.fixture(scope="module")
def setup():
    alist = lt.code_alist(CODE)
    s = lt.Simulator(alist, "Minsumf32", device=0, pool_size=POOL, pool_seed=POOL_SEED)
    dec = lt.LdpcDecoder(alist, "Minsumf32", device=0)
    rm = lt.NrRateMatcher(CODE)
    ref = rr.Config(2, 16)
    qams = {qm: lt.NrQam(qm) for qm in (2, 4, 6, 8)}
    codewords = s.pool_data()[1].copy()
    assert (s.n, s.k, s.n_tx, codewords.shape) == (N, K, N, (POOL, N))
    yield s, dec, rm, ref, alist, qams, codewords
    for x in (s, dec, rm) + tuple(qams.values()):
        x.close()


def concatenated_row(ref, codewords, seq, qm):
    """[rows][sum E]: every transmission's rate-matched row, one after the other"""
    return np.concatenate([ref.match(codewords, e, rv, qm) for e, rv in seq], axis=1)


def defined_llrs(rows, qm_mod, sigma, seed, first, max_log):
    """the LLRs of the concatenated rows [frames][sum E], float32: BPSK (qm_mod 1) is llr_from of frame_gen.hip.h on the
    channel's float32 noise -- y = (+-1) + float32(sigma) * z, llr = float32(-2 / sigma^2) * y -- and an NR modulation the
    simulator's defined chain"""
    if qm_mod == 1:
        y = cr.awgn(cr.modulate(rows, None, real=np.float32), sigma, seed, first)
        return (np.float32(-2.0 / (sigma * sigma)) * y).astype(np.float32)
    return nq.simulator_llrs(rows, qm_mod, sigma, seed, first, max_log)


@pytest.mark.parametrize("qm_mod,max_log,seq", [(1, False, [(481, 0), (95, 2), (96, 3)]), (4, False, SEQ), (4, True, SEQ), (8, False, SEQ),
                                                (8, True, SEQ)])
def test_generate_harq_equals_the_concatenation_definition(setup, qm_mod, max_log, seq):
    """(a) 70 frames from 2^32 - 30 on.  BPSK with E = 481, 95, 96: both seams are odd, so a normal pair is shared between
    two transmissions and each must use its own normal of it."""
    s, dec, rm, ref, alist, qams, codewords = setup
    ebn0_db, seed, first, frames = 2.0 + qm_mod, 31, (1 << 32) - 30, 70
    try:
        if qm_mod > 1:
            s.set_rate_match(rm, seq[0][0], seq[0][1], qm_mod)      # (n = 832 is no multiple of every QM: E_0 first)
            s.set_nr_qam(qams[qm_mod], max_log)
        s.set_harq(rm, seq, qm_mod)
        assert s.harq() == seq and s.n_tx == seq[0][0] and s.get("modulation") == qm_mod
        sigma = sim.noise_sigma(s.rate, ebn0_db, qm_mod)
        plain, plain_idx = s.generate(ebn0_db, seed, first, frames)
        want = None
        offset = 0
        for t, (e, rv) in enumerate(seq):
            got, idx = s.generate_harq(ebn0_db, seed, first, frames, t)
            assert np.array_equal(idx, plain_idx)
            if want is None:
                want = defined_llrs(concatenated_row(ref, codewords, seq, qm_mod)[idx], qm_mod, sigma, seed, first, max_log)
            assert got.shape == (frames, e) and (got > 0).any() and (got < 0).any()
            assert same_bits(got, want[:, offset:offset + e]), (qm_mod, max_log, t)
            if t == 0:
                assert same_bits(got, plain), "transmission 0 is what generate returns"
            offset += e
        with pytest.raises(ValueError, match="no transmission"):
            s.generate_harq(ebn0_db, seed, first, frames, len(seq))
    finally:
        s.set_nr_qam(None)
        s.set_harq(None)
    assert (s.get("harq"), s.get("rate_match"), s.n_tx) == (0, 0, N)


def cpu_pipeline(s, dec, ref, seq, qm, ebn0_db, seed, first, frames):
    """-> counters[6], per_tx[T][4] and, per transmission, (stopping, continuing) frames: every attempt decoded on the CPU
    side's soft buffer, frames leaving at their first converged attempt"""
    msgs = s.pool_data()[0]
    T = len(seq)
    active = np.arange(frames)
    soft, spent = None, np.zeros(frames, dtype=np.int64)
    counters, per_tx, populations = np.zeros(6, dtype=np.int64), np.zeros((T, 4), dtype=np.int64), []
    for t, (e, rv) in enumerate(seq):
        rx, idx = s.generate_harq(ebn0_db, seed, first, frames, t)
        soft = ref.recover(rx[active], rv, qm, np.inf, old=soft)
        bits, its, _ = dec.decode_batch(soft, MAX_ITER)
        errs = (bits[:, :K] != msgs[idx[active]]).sum(axis=1)
        ok = its >= 0
        used = np.where(ok, its, MAX_ITER)
        per_tx[t] = [active.size, ok.sum(), (ok & (errs > 0)).sum(), used.sum()]
        final = ok | (t == T - 1)
        total = spent + used
        counters += [final.sum(), errs[final].sum(), (errs[final] > 0).sum(), (ok & (errs > 0)).sum(), total[final].sum(),
                     total[final & (errs == 0)].sum()]
        populations.append((int(ok.sum()), int((~ok).sum())))
        active, soft, spent = active[~final], soft[~final], total[~final]
        if active.size == 0:
            break
    return counters, per_tx, populations


def test_counters_equal_the_cpu_pipeline(setup):
    """(b) BPSK, rv 0, 2, 3, 1 with E = 480, 96, 96, 96 at 0.5 dB, seed 31, frames 100 .. 355.  The pipeline's
    (attempts, stops) per transmission are (256, 32), (224, 65), (159, 110), (49, 22); 27 frames fail after all four
    attempts (counters [256, 1525, 27, 0, 16870, 13630]), and none is a false decode.  So the false-decode branch of the
    counters (counters[3], per_tx[t][2]) is not reached by this sample: it is covered only by the arithmetic that test (c)
    shares with `run`."""
    s, dec, rm, ref, alist, qams, codewords = setup
    ebn0_db, seed, first, frames = 0.5, 31, 100, 256
    s.set_harq(rm, SEQ, 1)
    try:
        want, want_tx, populations = cpu_pipeline(s, dec, ref, SEQ, 1, ebn0_db, seed, first, frames)
        print(f"BPSK HARQ at {ebn0_db} dB: (stopping, continuing) {populations}; counters {want.tolist()}; per_tx {want_tx.tolist()}")
        assert len(populations) == 4 and all(a >= 20 and b >= 20 for a, b in populations), populations
        got, got_tx = s.run_harq(ebn0_db, seed, first, frames, MAX_ITER)
        assert got.tolist() == want.tolist() and got_tx.tolist() == want_tx.tolist()
    finally:
        s.set_harq(None)


def test_agreement_with_run(setup):
    """(c) T = 1 is `run`; a sequence leaves `run`, `generate` and the pool those of its first transmission"""
    s, dec, rm, ref, alist, qams, codewords = setup
    plain = s.run(1.5, 31, 100, 300, MAX_ITER)
    frames = s.get("preferred_batch") + 300                  # two chunks
    try:
        s.set_rate_match(rm, 480, 0, 1)
        want, want_big = s.run(1.5, 31, 100, 300, MAX_ITER), s.run(1.5, 31, 100, frames, MAX_ITER)
        want_llrs, want_idx = s.generate(1.5, 31, 100, 70)
        want_msgs, want_tx = s.pool_data()
        s.set_harq(rm, SEQ[:1], 1)
        assert (s.get("harq"), s.get("harq_e0"), s.get("harq_rv0"), s.get("harq_e1"), s.get("rate_match"), s.n_tx) == (1, 480, 0, 0, 1, 480)
        for pooling in (0, 1):
            s.set("pooling", pooling)
            got, got_tx = s.run_harq(1.5, 31, 100, 300, MAX_ITER)
            assert got.tolist() == want.tolist() and got_tx.shape == (1, 4)
            assert got_tx[0].tolist()[::3] == [300, want[4]] and got_tx[0][1] - got_tx[0][2] <= 300 - want[2]
            big, big_tx = s.run_harq(1.5, 31, 100, frames, MAX_ITER)
            assert big.tolist() == want_big.tolist() and s.get("pooled_frames") == 0
        assert want[2] > 30 and want[0] - want[2] > 30, "the point must have converging and failing frames"
        s.set_harq(rm, SEQ, 1)
        assert (s.get("harq"), s.harq(), s.n_tx, s.rate) == (4, SEQ, 480, K / 480)
        assert s.run(1.5, 31, 100, 300, MAX_ITER).tolist() == want.tolist()
        llrs, idx = s.generate(1.5, 31, 100, 70)
        assert same_bits(llrs, want_llrs) and np.array_equal(idx, want_idx)
        msgs, tx = s.pool_data()
        assert np.array_equal(msgs, want_msgs) and np.array_equal(tx, want_tx)
        s.set_rate_match(rm, 480, 0, 1)
        assert (s.get("harq"), s.get("rate_match")) == (0, 1), "every set_rate_match call clears the further transmissions"
        s.set_harq(rm, SEQ, 1)
    finally:
        s.set("pooling", 1)
        s.set_rate_match(None)
    assert (s.get("harq"), s.get("rate_match"), s.n_tx) == (0, 0, N)
    assert s.run(1.5, 31, 100, 300, MAX_ITER).tolist() == plain.tolist(), "None restores the earlier counters"


def test_counters_do_not_depend_on_chunking_or_pooling(setup):
    """(d) several chunks at 1.0 dB, where most frames need a second transmission: with "pooling" 1 the stage pools fill,
    are flushed between chunks and pass their failures on"""
    s, dec, rm, ref, alist, qams, codewords = setup
    chunk = s.get("preferred_batch")
    frames = 2 * chunk + 5
    s.set_harq(rm, SEQ, 1)
    try:
        got = {}
        for pooling in (0, 1):
            s.set("pooling", pooling)
            got[pooling] = s.run_harq(1.0, 7, 0, frames, MAX_ITER) + (s.get("pooled_frames"),)
        parts = [s.run_harq(1.0, 7, f0, nf, MAX_ITER) for f0, nf in ((0, chunk), (chunk, chunk), (2 * chunk, 5))]
        summed = (sum(p[0] for p in parts), sum(p[1] for p in parts))
        print(f"{frames} frames: {got[0][0].tolist()}; per_tx {got[0][1].tolist()}; {got[1][2]} retransmission attempts pooled")
        for other in (got[1], summed):
            assert other[0].tolist() == got[0][0].tolist() and other[1].tolist() == got[0][1].tolist()
        assert got[0][2] == 0 and got[1][2] > 0 and got[1][2] == got[0][1][1:, 0].sum()
        assert got[0][0][0] == frames and got[0][1][0][0] == frames and got[0][1][1][0] > 0
        assert (got[0][1][1:, 0] == (got[0][1][:-1, 0] - got[0][1][:-1, 1])).all(), "who does not stop goes on"
    finally:
        s.set("pooling", 1)
        s.set_harq(None)


EBN0_64QAM = 3.5


def test_64qam_end_to_end(setup):
    """(e) set_nr_qam(NrQam(6)), E = 480, 96, 96, 96 with Qm 6, 256 frames (seed 31, from 100) against the CPU pipeline.
    The Eb/N0 is chosen on a 0.5 dB grid from one GPU run of these frames, (stopping, continuing) per transmission:
      2.0 dB (3, 253) (21, 232) (103, 129) (78, 51)      2.5 dB (5, 251) (59, 192) (133, 59) (39, 20)
      3.0 dB (13, 243) (107, 136) (117, 19) (15, 4)      3.5 dB (36, 220) (144, 76) (72, 4) (4, 0)
      4.0 dB (88, 168) (143, 25) (25, 0)                 4.5 dB (156, 100) (97, 3) (3, 0)
      5.0 dB (209, 47) (47, 0)                           5.5 dB (241, 15) (15, 0)                 6.0 dB (256, 0)
    At 3.5 dB every frame is delivered (counters [256, 0, 0, 0, 12146, 12146]); 5.0 dB has the grid's one false decode."""
    s, dec, rm, ref, alist, qams, codewords = setup
    seed, first, frames = 31, 100, 256
    s.set_rate_match(rm, 480, 0, 6)
    s.set_nr_qam(qams[6])
    try:
        s.set_harq(rm, SEQ, 6)
        want, want_tx, populations = cpu_pipeline(s, dec, ref, SEQ, 6, EBN0_64QAM, seed, first, frames)
        print(f"64QAM HARQ at {EBN0_64QAM} dB: (stopping, continuing) {populations}; counters {want.tolist()}; per_tx {want_tx.tolist()}")
        assert len(populations) >= 2 and all(a >= 20 and b >= 20 for a, b in populations[:2]), populations
        got, got_tx = s.run_harq(EBN0_64QAM, seed, first, frames, MAX_ITER)
        assert got.tolist() == want.tolist() and got_tx.tolist() == want_tx.tolist()
    finally:
        s.set_nr_qam(None)
        s.set_harq(None)


def test_refusals_and_clearing(setup):
    """(f)"""
    s, dec, rm, ref, alist, qams, codewords = setup
    L = _capi.lib()
    before = s.run(2.0, 31, 100, 64, MAX_ITER)
    with pytest.raises(ValueError, match="no HARQ sequence"):
        s.run_harq(2.0, 31, 100, 64, MAX_ITER)

    def unchanged():
        return (s.get("harq"), s.get("rate_match"), s.n_tx, s.get("n_tx")) == (0, 0, N, N)

    # a table constellation, 8PSK, an interleaver
    qpsk = lt.Demodulator("QPSK", device=0)
    s.set_constellation(qpsk)
    with pytest.raises(ValueError, match="BPSK or an NR modulation.*table constellation"):
        s.set_harq(rm, SEQ, 1)
    s.set_constellation(None)
    qpsk.close()
    assert unchanged()
    s.set_rate_match(rm, 480)
    s.set("modulation", 3)
    with pytest.raises(ValueError, match="BPSK or an NR modulation.*8PSK"):
        s.set_harq(rm, SEQ, 1)
    assert (s.get("harq"), s.get("rate_match"), s.n_tx) == (0, 1, 480)
    s.set("modulation", 1)
    s.set_rate_match(None)
    s.set("interleaving", 4)
    with pytest.raises(ValueError, match="no interleaving"):
        s.set_harq(rm, SEQ, 1)
    s.set("interleaving", 0)
    assert unchanged()
    # the sequence itself, and what set_rate_match refuses for the first transmission
    for seq, qm, why in (([], 1, "1 .. 8 transmissions"), (SEQ * 2 + SEQ[:1], 1, "1 .. 8 transmissions"), ([(480, 0), (96, 4)], 1, "rv must be"),
                         ([(480, 0), (95, 2)], 2, "Qm must divide E"), ([(0x7fffffff, 0), (96, 2)], 1, "sum above")):
        with pytest.raises(ValueError, match=why):
            s.set_harq(rm, seq, qm)
    wrong = lt.NrRateMatcher("nr5g:2:16:4")
    with pytest.raises(ValueError, match="filler"):
        s.set_harq(wrong, SEQ, 1)
    wrong.close()
    assert unchanged()
    # E_1 is no multiple of QM = 4
    s.set_rate_match(rm, 480, 0, 2)
    s.set_nr_qam(qams[4])
    with pytest.raises(ValueError, match="bits per symbol"):
        s.set_harq(rm, [(480, 0), (94, 2)], 2)
    assert (s.get("harq"), s.get("rate_match"), s.n_tx) == (0, 1, 480)
    s.set_nr_qam(None)
    s.set_rate_match(None)
    assert np.array_equal(s.run(2.0, 31, 100, 64, MAX_ITER), before), "a refusal changes nothing"
    # a modulation set after the sequence that does not fit it: the run is refused, not the setter
    s.set_harq(rm, [(480, 0), (95, 2)], 1)
    s.set_nr_qam(qams[2])
    counters = np.full(6, 0xAB, dtype=np.uint64)
    per_tx = np.full((2, 4), 0xAB, dtype=np.uint64)
    assert L.ldpc_toolbox_sim_run_harq(s._h, 2.0, 31, 100, 64, MAX_ITER, counters.ctypes.data, per_tx.ctypes.data) == -4
    assert "bits per symbol" in _capi.last_error() and (counters == 0).all()
    with pytest.raises(ValueError, match="bits per symbol"):
        s.generate_harq(2.0, 31, 100, 8, 1)
    s.set_nr_qam(None)
    # a BCH code
    code = lt.BchCode("bch:8:11D:2:160")
    s.set_bch(code)
    counters[:] = 0xAB
    assert L.ldpc_toolbox_sim_run_harq(s._h, 2.0, 31, 100, 64, MAX_ITER, counters.ctypes.data, per_tx.ctypes.data) == -4
    assert "BCH" in _capi.last_error() and (counters == 0).all()
    with pytest.raises(ValueError, match="BCH"):
        s.run_harq(2.0, 31, 100, 64, MAX_ITER)
    s.set_bch(None)
    code.close()
    assert s.run_harq(2.0, 31, 100, 64, MAX_ITER)[0][0] == 64
    # clearing
    assert L.ldpc_toolbox_sim_set_harq(None, rm._h, None, None, 0, 1) == -1
    s.set_harq(None)
    assert unchanged()
    with pytest.raises(ValueError, match="no HARQ sequence"):
        s.run_harq(2.0, 31, 100, 64, MAX_ITER)
    assert np.array_equal(s.run(2.0, 31, 100, 64, MAX_ITER), before), "None restores the earlier counters"


def test_ber_driver_with_a_harq_sequence(setup, tmp_path, capsys, monkeypatch):
    """(g)"""
    s, dec, rm, ref, alist, qams, codewords = setup
    path, path_harq = tmp_path / "harq.txt", tmp_path / "harq_tx.txt"
    points = (0.5, 1.5)
    args = ["--code", CODE, "--decoder", "Minsumf32", "--min-ebn0", "0.5", "--max-ebn0", "1.5", "--step-ebn0", "1", "--max-iter", str(MAX_ITER),
            "--max-frames", "256", "--frames-per-batch", "256", "--frame-errors", "100000", "--seed", "4", "--pool-size", str(POOL),
            "--nr-rate-match", "480", "--nr-harq", "2:96,3:96,1:96", "--output-file", str(path), "--output-file-harq", str(path_harq)]
    res = ber.main(args)
    capsys.readouterr()
    text, text_harq = path.read_text(), path_harq.read_text()
    for t in (text, text_harq):
        assert "Frame size (N): 480" in t and "NR rate matching (E[:RV[:QM]]): 480" in t
        assert " - NR HARQ transmissions (RV:E): 0:480, 2:96, 3:96, 1:96\n" in t
    rows = [[c.strip() for c in line.split("|")] for line in text.strip().splitlines()[-2:]]
    lines = text_harq.strip().splitlines()[-8:]
    own = lt.Simulator(alist, "Minsumf32", device=0, pool_size=POOL, pool_seed=5)
    own.set_harq(rm, SEQ, 1)
    for i, (row, ebn0_db) in enumerate(zip(rows, points)):
        counters, per_tx = own.run_harq(ebn0_db, ber.point_seed(4, ebn0_db), 0, 256, MAX_ITER)
        assert [int(row[1]), int(row[2]), int(row[3]), int(row[4])] == counters[:4].tolist()
        assert np.array_equal(res[i].harq_per_tx, per_tx)
        assert lines[4 * i:4 * i + 4] == ber.harq_lines(ebn0_db, SEQ, per_tx, 256)
        for t, line in enumerate(lines[4 * i:4 * i + 4]):
            cells = [c.strip() for c in line.split("|")]
            assert [int(c) for c in cells[1:8]] == [t, SEQ[t][1], SEQ[t][0]] + per_tx[t].tolist()
            delivered = int((per_tx[:t + 1, 1] - per_tx[:t + 1, 2]).sum())
            assert float(cells[8]) == pytest.approx(1 - delivered / 256, abs=5e-3 * max(1 - delivered / 256, 1e-9) + 1e-12)
    own.close()
    assert int(rows[0][3]) > int(rows[1][3]) >= 0, "frame errors fall with Eb/N0"
    # E defaults to the first transmission's
    ber.main(args[:-8] + ["--nr-rate-match", "192:0:1", "--nr-harq", "2,3:96", "--output-file", str(path)])
    assert " - NR HARQ transmissions (RV:E): 0:192, 2:192, 3:96\n" in path.read_text()
    for extra in (["--bch-max-errors", "2"], ["--bch-code", "bch:8:11D:2:160"], ["--codes", "nr5g:2:16"], ["--interleaving", "4"],
                  ["--nr-harq", "2:96:1"], ["--nr-harq", "x"], ["--nr-harq", "4:96"]):
        with pytest.raises(SystemExit):
            ber.main(args + extra)
    with pytest.raises(SystemExit):
        ber.main([a for a in args if a not in ("--nr-rate-match", "480")])     # --nr-harq without --nr-rate-match
    with pytest.raises(SystemExit):
        ber.main(args[:-8] + ["--nr-rate-match", "480", "--output-file-harq", str(path_harq)])   # the file without a sequence
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        ber.main(args)
    capsys.readouterr()
