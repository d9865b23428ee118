"""GPU: the simulator with a real outer BCH code (ldpc_toolbox_sim_set_bch) and the receive chain with the BCH decoder at
its end.  Counters 6..8 are compared with a CPU pipeline -- the simulator's own frames, the LDPC decoder, the XOR with
the pooled message, then the numpy BCH decoder of tests/bch_reference.py -- and the chain's last stage with the same
reference run on the LDPC decoder's own output."""
import numpy as np
import pytest
import torch

import bch_reference as br
import ldpc_toolbox_amd as lt
from ldpc_toolbox_amd import _capi, ber
from ldpc_toolbox_amd import simulation as sim

pytestmark = pytest.mark.gpu

CODE = "dvbs2:R1_2short"     # k_ldpc = 7200 = n_bch, t = 12
# dvbs2:R1_2short, BPSK, plain min-sum stopped after 30 iterations at 1.3 dB: of 64 frames the oracle (bit-identical to
# the GPU) leaves 29 without a bit error in the first 7200 bits, 19 with 1..12 and 16 with more -- chosen on the CPU
EBN0_DB, MAX_ITER, T = 1.3, 30, 12
FRAMES = 512                 # one chunk of the simulator


@pytest.fixture(scope="module")
def setup():
    alist = lt.code_alist(CODE)
    s = lt.Simulator(alist, "Minsumf32", device=0, pool_size=16, pool_seed=5)
    dec = lt.LdpcDecoder(alist, "Minsumf32", device=0)
    code = lt.BchCode(CODE)
    ref = br.Code.from_spec(CODE)
    assert s.k == ref.n == code.n
    yield s, dec, code, ref
    for x in (s, dec, code):
        x.close()


@pytest.fixture(scope="module")
def cpu_pipeline(setup):
    """per frame of the run below: LDPC bit errors, iterations, and the residual errors the reference BCH decoder leaves"""
    s, dec, code, ref = setup
    llrs, idx = s.generate(EBN0_DB, 31, 100, FRAMES)
    msgs, _ = s.pool_data()
    bits, its, _ = dec.decode_batch(llrs, MAX_ITER)
    e = (bits[:, :s.k] != msgs[idx]).astype(np.uint8)
    errs = e.sum(axis=1)
    residual = np.zeros(FRAMES, dtype=np.int64)
    outcome = np.zeros(FRAMES, dtype=np.int32)
    for f in np.flatnonzero(errs):
        out, outcome[f] = ref.decode_one(e[f])
        residual[f] = int(out[:ref.k].sum())
    used = np.where(its >= 0, its, MAX_ITER)
    return errs, used, residual, outcome


def test_counters_equal_the_cpu_pipeline(setup, cpu_pipeline):
    s, dec, code, ref = setup
    errs, used, residual, outcome = cpu_pipeline
    corrected = (errs > 0) & (residual == 0)
    failed = residual > 0
    print(f"{FRAMES} frames: {int((errs == 0).sum())} clean, {int(corrected.sum())} corrected by the BCH code, {int(failed.sum())} "
          f"not; {int((outcome < 0).sum())} detected, {int(((outcome >= 0) & failed).sum())} miscorrected, "
          f"{int(((errs > T) & ~failed).sum())} with more than t errors but none in the message")
    assert corrected.sum() >= 10 and failed.sum() >= 10, "the point must have BCH-corrected and BCH-failed frames"
    plain = s.run(EBN0_DB, 31, 100, FRAMES, MAX_ITER)
    genie = s.run(EBN0_DB, 31, 100, FRAMES, MAX_ITER, T)
    s.set_bch(code)
    assert s.get("bch") == 1
    try:
        real = s.run(EBN0_DB, 31, 100, FRAMES, MAX_ITER, T)
        assert np.array_equal(s.run(EBN0_DB, 31, 100, FRAMES, MAX_ITER), plain), "run() does not see the code"
    finally:
        s.set_bch(None)
    assert s.get("bch") == 0
    want = [int(residual.sum()), int(failed.sum()), int(used[~failed].sum())]
    assert real[6:].tolist() == want
    assert np.array_equal(real[:6], plain) and np.array_equal(genie[:6], plain), "counters 0..5 are what they are without a code"
    assert plain.tolist() == [FRAMES, int(errs.sum()), int((errs > 0).sum()), plain[3], int(used.sum()), int(used[errs == 0].sum())]
    # on the frames with at most t errors the two accountings agree: both count them as corrected
    few = errs <= T
    assert (residual[few] == 0).all()
    assert genie[6:].tolist() == [int(errs[~few].sum()), int((~few).sum()), int(used[few].sum())]
    # ... and NULL restores the genie's numbers exactly
    assert np.array_equal(s.run(EBN0_DB, 31, 100, FRAMES, MAX_ITER, T), genie)


def test_counters_do_not_depend_on_pooling(setup):
    """three calls of one chunk each at 1.25 dB with 200 iterations, far more than the frames need (37 on average): from the
    second call on the stragglers are pooled and decoded again (136 frames), so the BCH counters come from the chunks'
    count and from the pool's flush.  78 frames keep bit errors; the BCH code corrects one of them."""
    s, dec, code, ref = setup
    s.set_bch(code)
    try:
        got = {}
        for pooling in (0, 1):
            s.set("pooling", pooling)
            total = np.zeros(9, dtype=np.int64)
            pooled = 0
            for call in range(3):
                total += s.run(1.25, 7, 4096 * call, 4096, 200, T)
                pooled += s.get("pooled_frames")
            got[pooling] = (total, pooled)
        print(f"pooling 0: {got[0][0].tolist()}; pooling 1: {got[1][0].tolist()}, {got[1][1]} frames through the pool")
        assert got[0][1] == 0 and got[1][1] > 0, "the second configuration must actually pool"
        assert np.array_equal(got[0][0], got[1][0])
        assert got[0][0][7] > 0 and got[0][0][2] > got[0][0][7], "BCH-failed and BCH-corrected frames"
    finally:
        s.set("pooling", 1)
        s.set_bch(None)


def test_pool_left_by_larger_chunks(setup):
    """a run without a code in chunks of 8192 frames leaves the straggler pool with room for 16384; the code is set and
    the group lowered to 4096 afterwards, and a pooled run of several chunks must still count as the unpooled one does:
    the patterns of a flush are as many as the pool holds, not as two of this call's chunks"""
    s, dec, code, ref = setup
    try:
        s.set("group_size", 8192)
        s.set("pooling", 1)
        before = s.run(1.25, 7, 0, 16384, 200)
        assert before[0] == 16384
        s.set("group_size", 4096)
        s.set_bch(code)
        got = {}
        for pooling in (1, 0):
            s.set("pooling", pooling)
            s.run(1.25, 7, 0, 4096, 200, T)          # (the call that learns the budget)
            got[pooling] = (s.run(1.25, 7, 4096, 12288, 200, T), s.get("pooled_frames"))
        print(f"pooling 1: {got[1][0].tolist()}, {got[1][1]} frames through the pool; pooling 0: {got[0][0].tolist()}")
        assert got[1][1] > 0 and got[0][1] == 0
        assert np.array_equal(got[0][0], got[1][0]) and got[0][0][7] > 0
    finally:
        s.set("pooling", 1)
        s.set("group_size", 0)
        s.set_bch(None)


def test_refusals(setup):
    s, dec, code, ref = setup
    before = s.run(EBN0_DB, 31, 100, 64, MAX_ITER, T)
    for spec in ("dvbs2:R1_3short", "bch:14:402B:12:7201", "dvbs2:R1_2"):
        wrong = lt.BchCode(spec)
        with pytest.raises(ValueError, match="not the LDPC code's k"):
            s.set_bch(wrong)
        wrong.close()
    assert s.get("bch") == 0 and np.array_equal(s.run(EBN0_DB, 31, 100, 64, MAX_ITER, T), before), "a refusal changes nothing"
    s.set_bch(code)
    try:
        for wrong_t in (1, 11, 13):
            with pytest.raises(ValueError, match="not the t of the BCH code"):
                s.run(EBN0_DB, 31, 100, 64, MAX_ITER, wrong_t)
        L = _capi.lib()
        out = np.full(9, 77, dtype=np.uint64)
        assert L.ldpc_toolbox_sim_run_bch(s._h, EBN0_DB, 31, 100, 64, MAX_ITER, 11, out.ctypes.data) == -4
        assert L.ldpc_toolbox_sim_run_bch(s._h, EBN0_DB, 31, 100, 64, MAX_ITER, 0, out.ctypes.data) == -4, "0 is not t either"
        assert "not the t of the BCH code" in _capi.last_error()
    finally:
        s.set_bch(None)
    # the pair that cannot be chained: the library's LDPC code dvbs2:R3_4short has k = 1080, the BCH code n = 11880
    # (that LDPC code has a check node of degree 1, which only the Phi and Tanh rules take)
    short = lt.Simulator(lt.code_alist("dvbs2:R3_4short"), "Phif32", device=0, pool_size=2)
    pair = lt.BchCode("dvbs2:R3_4short")
    assert (short.k, pair.n) == (1080, 11880)
    with pytest.raises(ValueError, match="not the LDPC code's k"):
        short.set_bch(pair)
    short.close()
    pair.close()


def test_ber_driver_prints_the_table_of_those_counters(setup, tmp_path, capsys):
    s, dec, code, ref = setup
    path = tmp_path / "bch.txt"
    args = ["--code", CODE, "--decoder", "Minsumf32", "--min-ebn0", str(EBN0_DB), "--max-ebn0", str(EBN0_DB), "--step-ebn0", "1",
            "--max-iter", str(MAX_ITER), "--max-frames", str(FRAMES), "--frames-per-batch", str(FRAMES), "--frame-errors", "100000",
            "--seed", "4", "--pool-size", "16", "--bch-code", CODE, "--output-file", str(path)]
    ber.main(args)
    capsys.readouterr()
    text = path.read_text()
    assert "Maximum bit errors correctable: 12" in text and "LDPC+BCH results" in text
    row = [c.strip() for c in text.strip().splitlines()[-1].split("|")]
    own = lt.Simulator(lt.code_alist(CODE), "Minsumf32", device=0, pool_size=16, pool_seed=5)
    own.set_bch(code)
    counters = own.run(EBN0_DB, ber.point_seed(4, EBN0_DB), 0, FRAMES, MAX_ITER, T)
    own.close()
    assert counters[7] > 0 and counters[2] > counters[7]
    want = [c.strip() for c in sim.format_progress(ber.statistics_from_counters(EBN0_DB, s.k, counters, 1.0)).split("|")]
    assert row[:9] == want[:9], "every column but throughput and elapsed time"
    with pytest.raises(SystemExit):
        ber.main(args + ["--bch-max-errors", "10"])
    capsys.readouterr()


def test_chain_on_one_stream(setup):
    """BCH encode -> LDPC encode -> modulate -> AWGN -> demap -> LDPC decode (output_len = 7200) -> BCH decode"""
    s, dec, code, ref = setup
    alist = lt.code_alist(CODE)
    enc = lt.Encoder(alist)
    d = lt.Demodulator("BPSK", device=0)
    frames, n, k, kb = 64, dec.n, dec.k, code.k
    msgs = np.random.default_rng(2024).integers(0, 2, (frames, kb), dtype=np.uint8)
    sigma = sim.noise_sigma(k / n, EBN0_DB)
    dev = torch.device("cuda", 0)
    d_msgs = torch.from_numpy(msgs).to(dev)
    d_word = torch.zeros((frames, k), dtype=torch.uint8, device=dev)
    d_cws = torch.zeros((frames, n), dtype=torch.uint8, device=dev)
    d_sym = torch.zeros((frames, n), dtype=torch.float32, device=dev)
    d_llrs = torch.zeros((frames, n), dtype=torch.float32, device=dev)
    d_bits = torch.zeros((frames, k), dtype=torch.uint8, device=dev)
    d_its = torch.zeros(frames, dtype=torch.int32, device=dev)
    d_out = torch.zeros((frames, kb), dtype=torch.uint8, device=dev)
    d_err = torch.zeros(frames, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    st = stream.cuda_stream
    code.encode_device(d_msgs.data_ptr(), d_word.data_ptr(), frames, stream=st)
    enc.encode_batch_device(d_word.data_ptr(), d_cws.data_ptr(), frames, st)
    d.modulate_device(d_cws.data_ptr(), d_sym.data_ptr(), False, frames, n, 0, st)
    d.add_noise_device(d_sym.data_ptr(), False, frames, n, sigma, 99, 1000, st)
    d.demodulate_device(d_sym.data_ptr(), d_llrs.data_ptr(), False, frames, n, sigma, 0, False, st)
    dec.decode_batch_device(d_llrs.data_ptr(), False, frames, MAX_ITER, d_bits.data_ptr(), k, d_its.data_ptr(), 0, st)
    code.decode_device(d_bits.data_ptr(), d_out.data_ptr(), frames, errors_ptr=d_err.data_ptr(), stream=st)
    stream.synchronize()
    word = d_word.cpu().numpy()
    assert np.array_equal(word, ref.encode(msgs)) and np.array_equal(d_cws.cpu().numpy()[:, :k], word)
    bits, out, err = d_bits.cpu().numpy(), d_out.cpu().numpy(), d_err.cpu().numpy()
    want, want_err = ref.decode(bits)
    assert np.array_equal(err, want_err) and np.array_equal(out, want[:, :kb])
    clean, fixed, detected = int((err == 0).sum()), int(((err > 0) & (err <= T)).sum()), int((err < 0).sum())
    print(f"{frames} frames: {clean} without residual errors, {fixed} corrected, {detected} detected")
    assert clean >= 3 and fixed >= 3 and detected >= 3
    assert np.array_equal(out[err >= 0], msgs[err >= 0]), "at this point no frame is miscorrected"
    enc.close()
    d.close()
