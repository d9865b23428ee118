"""GPU: the HARQ simulator with "soft_bits" 8 (include/ldpc_toolbox.h, PART 9) -- the set-up of tests/test_sim_harq_gpu.py
(nr5g:2:16, n = 832, k = 160, pool 16 with seed 5, 30 iterations, E = 480, 96, 96, 96 with rv 0, 2, 3, 1) with Minsumi8Offset.

The definition restated as a CPU pipeline: a frame's attempt after transmission t is the float row `generate_harq(t)`
returns taken through the numpy quantiser, the numpy saturating recovery (tests/nr_soft_i8_restatement.py) into the frame's
int8 soft row with combine = (t > 0), and `LdpcDecoder.decode_batch` on the soft row / 8 as float32; frames leave at their
first converged attempt.  That pipeline is the reference for the counters."""
import numpy as np
import pytest

import ldpc_toolbox_amd as lt
import nr_rate_match_reference as rr
import nr_soft_i8_restatement as sr
from ldpc_toolbox_amd import _capi, ber

pytestmark = pytest.mark.gpu

CODE = "nr5g:2:16"
N, K = 832, 160
MAX_ITER = 30
POOL, POOL_SEED = 16, 5
SEQ = [(480, 0), (96, 2), (96, 3), (96, 1)]
NAME = "Minsumi8Offset"
EBN0_BPSK = -0.25
EBN0_64QAM = 3.0


@pytest.fixture(scope="module")
def setup():
    alist = lt.code_alist(CODE)
    s = lt.Simulator(alist, NAME, device=0, pool_size=POOL, pool_seed=POOL_SEED)
    dec = lt.LdpcDecoder(alist, NAME, device=0)
    rm = lt.NrRateMatcher(CODE)
    ref = rr.Config(2, 16)
    assert (s.n, s.k, s.get("soft_bits")) == (N, K, 32)
    yield s, dec, rm, ref, alist
    for x in (s, dec, rm):
        x.close()


def cpu_pipeline(s, dec, ref, seq, qm, ebn0_db, seed, first, frames):
    """-> counters[6], per_tx[T][4], per transmission (stopping, continuing) frames, and how many (frame, column) cells of a
    combined soft row saturated"""
    msgs = s.pool_data()[0]
    T = len(seq)
    active = np.arange(frames)
    soft, spent = None, np.zeros(frames, dtype=np.int64)
    counters, per_tx, populations, saturated = np.zeros(6, dtype=np.int64), np.zeros((T, 4), dtype=np.int64), [], 0
    for t, (e, rv) in enumerate(seq):
        rx, idx = s.generate_harq(ebn0_db, seed, first, frames, t)
        sat = np.zeros((active.size, ref.n), dtype=bool)
        soft = sr.recover_i8(ref, sr.quantise(rx[active]), rv, qm, 127, old=soft, saturated=sat)
        saturated += int(sat.sum()) if t > 0 else 0
        bits, its, _ = dec.decode_batch(sr.dequantise(soft), MAX_ITER)
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
    return counters, per_tx, populations, saturated


def run_both_ways(s, ebn0_db, seed, first, frames):
    """run_harq with pooling 1, with pooling 0, and cut into three chunks and summed"""
    out = {}
    for pooling in (1, 0):
        s.set("pooling", pooling)
        out[pooling] = s.run_harq(ebn0_db, seed, first, frames, MAX_ITER)
    s.set("pooling", 1)
    cuts = [(first, frames // 3), (first + frames // 3, frames // 3), (first + 2 * (frames // 3), frames - 2 * (frames // 3))]
    parts = [s.run_harq(ebn0_db, seed, f0, nf, MAX_ITER) for f0, nf in cuts]
    out["chunks"] = (sum(p[0] for p in parts), sum(p[1] for p in parts))
    return out


def test_bpsk_counters_equal_the_cpu_pipeline(setup):
    """BPSK, 256 frames (seed 31, from 100).  The point: every transmission but the last must have at least 20 stopping and 20
    continuing frames.  The composed pipeline's (stopping, continuing) per transmission on a 0.25 dB grid, one GPU run:
      -0.75 dB (7, 249) (28, 221) (124, 97) (49, 48)     -0.5 dB (13, 243) (49, 194) (129, 65) (39, 26)
      -0.25 dB (23, 233) (82, 151) (117, 34) (21, 13)     0.0 dB (40, 216) (107, 109) (92, 17) (8, 9)
       0.25 dB (78, 178) (102, 76) (69, 7) (5, 2)         0.5 dB (117, 139) (88, 51) (48, 3) (2, 1)
    0.5 dB, the float test's point, misses it at the third transmission; -0.25 dB is the one point that meets it
    (counters [256, 484, 13, 0, 17123, 15563]).
    No combined cell saturates at any of these points, and none can: a BPSK LLR here is 2 y / sigma^2 with sigma^2 about
    1.6, some 1.3 +- 1.6 LLR units or 10 +- 13 steps, and the 768 transmitted bits carry a column a few times at most, so a
    combined soft bit stays far from 127.  The saturation condition is asserted where the LLRs reach the clip: 64QAM, below."""
    s, dec, rm, ref, alist = setup
    seed, first, frames = 31, 100, 256
    s.set_harq(rm, SEQ, 1)
    try:
        float_run = s.run_harq(EBN0_BPSK, seed, first, frames, MAX_ITER)
        want, want_tx, populations, saturated = cpu_pipeline(s, dec, ref, SEQ, 1, EBN0_BPSK, seed, first, frames)
        print(f"BPSK HARQ, 8-bit soft bits, {EBN0_BPSK} dB: (stopping, continuing) {populations}; {saturated} combined cells saturate; "
              f"counters {want.tolist()}; per_tx {want_tx.tolist()}; float soft buffers: {float_run[0].tolist()}")
        s.set("soft_bits", 8)
        assert s.get("soft_bits") == 8
        for how, (got, got_tx) in run_both_ways(s, EBN0_BPSK, seed, first, frames).items():
            assert got.tolist() == want.tolist() and got_tx.tolist() == want_tx.tolist(), how
        assert len(populations) == 4 and all(a >= 20 and b >= 20 for a, b in populations[:-1]), populations
        # run, generate and generate_harq are not touched by the key
        llrs8, idx8 = s.generate_harq(EBN0_BPSK, seed, first, 8, 1)
        plain8 = s.run(EBN0_BPSK, seed, first, frames, MAX_ITER)
        s.set("soft_bits", 32)
        assert s.get("soft_bits") == 32
        again = s.run_harq(EBN0_BPSK, seed, first, frames, MAX_ITER)
        assert again[0].tolist() == float_run[0].tolist() and again[1].tolist() == float_run[1].tolist(), "32 restores the float run"
        llrs32, idx32 = s.generate_harq(EBN0_BPSK, seed, first, 8, 1)
        assert np.array_equal(llrs8.view(np.uint32), llrs32.view(np.uint32)) and np.array_equal(idx8, idx32)
        assert s.run(EBN0_BPSK, seed, first, frames, MAX_ITER).tolist() == plain8.tolist()
    finally:
        s.set("soft_bits", 32)
        s.set("pooling", 1)
        s.set_harq(None)


def test_64qam_counters_equal_the_cpu_pipeline(setup):
    """set_nr_qam(NrQam(6)), Qm 6, 256 frames (seed 31, from 100).  The composed pipeline's (stopping, continuing) per
    transmission and the combined cells that saturate, on a 0.25 dB grid, one GPU run:
      2.5 dB  (5, 251) (102, 149) (110, 39) (32, 7)  2     2.75 dB (10, 246) (120, 126) (105, 21) (17, 4)  2
      3.0 dB  (20, 236) (146, 90) (75, 15) (12, 3)   3     3.25 dB (40, 216) (165, 51) (44, 7) (6, 1)      7
      3.5 dB  (72, 184) (152, 32) (29, 3) (3, 0)    10     3.75 dB (94, 162) (139, 23) (22, 1) (1, 0)     13
    No point of the grid has 20 stopping and 20 continuing frames in all of the first three transmissions: below 3.0 dB fewer
    than 20 frames stop at the first, from 3.0 dB on fewer than 20 continue after the third.  3.0 dB comes closest -- it
    misses by the third transmission's 15 continuing frames -- so the condition is asserted for the first two transmissions,
    as tests/test_sim_harq_gpu.py does for this modulation, and that the third and fourth are reached.  Counters at 3.0 dB:
    [256, 38, 3, 1, 13742, 13476]; 3 combined cells saturate."""
    s, dec, rm, ref, alist = setup
    seed, first, frames = 31, 100, 256
    qam = lt.NrQam(6)
    s.set_rate_match(rm, 480, 0, 6)
    s.set_nr_qam(qam)
    try:
        s.set_harq(rm, SEQ, 6)
        want, want_tx, populations, saturated = cpu_pipeline(s, dec, ref, SEQ, 6, EBN0_64QAM, seed, first, frames)
        print(f"64QAM HARQ, 8-bit soft bits, {EBN0_64QAM} dB: (stopping, continuing) {populations}; {saturated} combined cells saturate; "
              f"counters {want.tolist()}; per_tx {want_tx.tolist()}")
        s.set("soft_bits", 8)
        for how, (got, got_tx) in run_both_ways(s, EBN0_64QAM, seed, first, frames).items():
            assert got.tolist() == want.tolist() and got_tx.tolist() == want_tx.tolist(), how
        assert len(populations) == 4 and all(a >= 20 and b >= 20 for a, b in populations[:2]), populations
        assert saturated >= 1
    finally:
        s.set("soft_bits", 32)
        s.set("pooling", 1)
        s.set_nr_qam(None)
        s.set_harq(None)
        qam.close()


def test_several_chunks_fill_and_flush_the_stage_pools(setup):
    """two chunks and five frames at 1.0 dB: with "pooling" 1 the int8 stage pools fill, are flushed between chunks and pass
    their failures on; the counters are those of "pooling" 0 and of the three calls summed"""
    s, dec, rm, ref, alist = setup
    chunk = s.get("preferred_batch")
    frames = 2 * chunk + 5
    s.set_harq(rm, SEQ, 1)
    s.set("soft_bits", 8)
    try:
        got = {}
        for pooling in (0, 1):
            s.set("pooling", pooling)
            got[pooling] = s.run_harq(1.0, 7, 0, frames, MAX_ITER) + (s.get("pooled_frames"),)
        parts = [s.run_harq(1.0, 7, f0, nf, MAX_ITER) for f0, nf in ((0, chunk), (chunk, chunk), (2 * chunk, 5))]
        summed = (sum(p[0] for p in parts), sum(p[1] for p in parts))
        for other in (got[1], summed):
            assert other[0].tolist() == got[0][0].tolist() and other[1].tolist() == got[0][1].tolist()
        assert got[0][2] == 0 and got[1][2] > 0 and got[1][2] == got[0][1][1:, 0].sum()
        assert got[0][0][0] == frames and got[0][1][1][0] > 0
        assert (got[0][1][1:, 0] == (got[0][1][:-1, 0] - got[0][1][:-1, 1])).all(), "who does not stop goes on"
    finally:
        s.set("soft_bits", 32)
        s.set("pooling", 1)
        s.set_harq(None)


def test_soft_bits_8_needs_an_8_bit_implementation(setup):
    s, dec, rm, ref, alist = setup
    L = _capi.lib()
    f = lt.Simulator(alist, "Minsumf32", device=0, pool_size=POOL, pool_seed=POOL_SEED)
    with pytest.raises(ValueError, match="8-bit implementations"):
        f.set("soft_bits", 8)
    assert f.get("soft_bits") == 32
    assert L.ldpc_toolbox_sim_set(f._h, b"soft_bits", 7) == -1 and "soft_bits must be 8 or 32" in _capi.last_error()
    f.set("soft_bits", 32)
    f.close()
    with pytest.raises(ValueError, match="8 or 32"):
        s.set("soft_bits", 7)
    assert s.get("soft_bits") == 32


def test_ber_driver_with_8_bit_soft_bits(setup, tmp_path, capsys):
    s, dec, rm, ref, alist = setup
    path, path_harq = tmp_path / "harq.txt", tmp_path / "harq_tx.txt"
    points = (0.5, 1.5)
    args = ["--code", CODE, "--decoder", NAME, "--min-ebn0", "0.5", "--max-ebn0", "1.5", "--step-ebn0", "1", "--max-iter", str(MAX_ITER),
            "--max-frames", "256", "--frames-per-batch", "256", "--frame-errors", "100000", "--seed", "4", "--pool-size", str(POOL),
            "--nr-rate-match", "480", "--nr-harq", "2:96,3:96,1:96", "--output-file", str(path), "--output-file-harq", str(path_harq)]
    res = ber.main(args + ["--nr-soft-bits", "8"])
    capsys.readouterr()
    text, text_harq = path.read_text(), path_harq.read_text()
    assert " - NR HARQ soft buffer: 8-bit soft bits\n" in text and " - NR HARQ transmissions (RV:E): 0:480, 2:96, 3:96, 1:96\n" in text
    lines = text_harq.strip().splitlines()[-8:]
    s.set_harq(rm, SEQ, 1)
    s.set("soft_bits", 8)
    try:
        for i, ebn0_db in enumerate(points):
            counters, per_tx = s.run_harq(ebn0_db, ber.point_seed(4, ebn0_db), 0, 256, MAX_ITER)
            assert np.array_equal(res[i].harq_per_tx, per_tx)
            assert lines[4 * i:4 * i + 4] == ber.harq_lines(ebn0_db, SEQ, per_tx, 256)
    finally:
        s.set("soft_bits", 32)
        s.set_harq(None)
    # the option needs a HARQ sequence and an 8-bit decoder
    for bad in (args[:args.index("--nr-harq")] + args[args.index("--nr-harq") + 2:-2] + ["--nr-soft-bits", "8"],
                [a if a != NAME else "Minsumf32" for a in args] + ["--nr-soft-bits", "8"], args + ["--nr-soft-bits", "16"]):
        with pytest.raises(SystemExit):
            ber.main(bad)
    capsys.readouterr()
    ber.main(args + ["--nr-soft-bits", "32"])
    capsys.readouterr()
    assert "NR HARQ soft buffer" not in path.read_text()
