"""GPU: the simulator with a constellation (ldpc_toolbox_sim_set_constellation): its fused generator against
"modulation" = 3 for the 8PSK handle and against the restatement chain modulate -> AWGN -> demap
(tests/constellation_cases.chain_llrs) for every other table and both fold steps, its counters against the CPU pipeline,
its refusals, and the sweep driver's --modulation QPSK / --constellation / --max-log."""
import numpy as np
import pytest
import torch

import constellation_cases as cc
import ldpc_toolbox_amd as lt
from demod_restatement import same_bits
from ldpc_toolbox_amd import simulation as sim

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPEC = "nr5g:2:15"       # n = 780: a multiple of 2, 3, 4 and 5
FRAMES, FIRST = 600, 100


def alist():
    return lt.code_alist(SPEC)


def simulator(name, max_log=False, interleaving=0, impl="Minsumf32", **kw):
    d = cc.make_demodulator(lt, name)
    s = lt.Simulator(alist(), impl, device=0, pool_size=16, pool_seed=9, modulation=d, interleaving=interleaving,
                     max_log=max_log, **kw)
    d.close()       # the simulator holds a copy of the constellation
    return s


# ---- 1: the 8PSK handle is "modulation" = 3 ----------------------------------------------------------------

@pytest.mark.parametrize("interleaving", [0, 3, -3])
def test_psk8_handle_equals_modulation_3(interleaving):
    old = lt.Simulator(alist(), "HLMinsumf32", device=0, pool_size=16, pool_seed=9, modulation="8PSK", interleaving=interleaving)
    new = simulator("8PSK", False, interleaving, impl="HLMinsumf32")
    assert new.n_tx == 780 and new.get("constellation") == 1 and old.get("constellation") == 0
    assert new.get("modulation") == 3 and new.get("max_log") == 0
    for ebn0, seed in ((1.0, 5), (4.0, 2 ** 41 + 5)):
        want, widx = old.generate(ebn0, seed, FIRST, FRAMES)
        got, gidx = new.generate(ebn0, seed, FIRST, FRAMES)
        assert np.array_equal(gidx, widx) and same_bits(got, want), (interleaving, ebn0)
        assert np.array_equal(new.run(ebn0, seed, FIRST, FRAMES, 25), old.run(ebn0, seed, FIRST, FRAMES, 25))
    got = new.run(1.0, 5, FIRST, FRAMES, 25)
    assert got[0] == FRAMES and 0 < got[2] < FRAMES                # failures and successes at 1 dB
    old.close()
    new.close()


# ---- 2: other tables, both fold steps, against the restatement chain -----------------------------------------

@pytest.mark.parametrize("max_log", [False, True])
@pytest.mark.parametrize("name", ["two", "QPSK", "rings16", "rings32"])
def test_generate_equals_the_restatement_chain(name, max_log):
    m = cc.bits_of(name)
    for interleaving in (0, -m, 6):
        s = simulator(name, max_log, interleaving)
        assert s.get("modulation") == m and s.get("max_log") == int(max_log) and s.bits_per_symbol == m
        _, tx = s.pool_data()
        for ebn0, seed, first, frames in ((6.0, 21, FIRST, 40), (-1.0, 2 ** 63 + 5, 2 ** 34, 7)):
            got, idx = s.generate(ebn0, seed, first, frames)
            sigma = sim.noise_sigma(s.rate, ebn0, m)
            want = cc.chain_llrs(tx[idx], name, max_log, interleaving, sigma, seed, first)
            assert same_bits(got, want), (name, max_log, interleaving, ebn0)
            # generate_into: the same frames written straight into device memory
            d_llrs = torch.zeros((frames, s.n_tx), dtype=torch.float32, device=DEV)
            idx2 = s.generate_into(d_llrs.data_ptr(), ebn0, seed, first, frames)
            assert np.array_equal(idx2, idx) and same_bits(d_llrs.cpu().numpy(), got)
        s.close()


def test_fold_steps_and_energy_term_matter():
    """the restatement itself tells the variants apart on these frames (so the equalities above can fail)"""
    s = simulator("rings16", False)
    _, tx = s.pool_data()
    got, idx = s.generate(6.0, 21, FIRST, 40)
    sigma = sim.noise_sigma(s.rate, 6.0, 4)
    assert not np.array_equal(got, cc.chain_llrs(tx[idx], "rings16", True, 0, sigma, 21, FIRST))
    import channel_restatement as cr
    import demod_restatement as dr
    pts = cc.TABLES["rings16"][0]
    rx = cr.awgn(cr.modulate(tx[idx], pts, 0), sigma, 21, FIRST)
    assert not np.array_equal(got, dr.demodulate(rx, sigma, pts, False, False, 0).astype(np.float32))
    s.close()


# ---- 3: counters against the CPU pipeline -------------------------------------------------------------------

# Chosen on the CPU with the oracle (HLMinsumf32, 25 iterations, 600 frames, the restatement chain on a stand-in pool of 16
# encoded random messages): QPSK exact at 1.0 dB gave 242 frame errors of 600 (2.0 dB: 14), the 16-point table with the
# max-log demapper at 6.0 dB gave 332 of 600 (5.0 dB: 527, 7.0 dB: 87) -- failures and successes at both points.  With the
# simulator's own pool (pool_size 16, pool_seed 9) the same points give 243 and 317 frame errors of 600.
COUNTER_POINTS = [("QPSK", False, 1.0), ("rings16", True, 6.0)]


@pytest.mark.parametrize("name,max_log,ebn0", COUNTER_POINTS)
def test_run_counters_match_the_cpu_pipeline(oracle, name, max_log, ebn0):
    """sim_run = generate, then oracle.decode_batch, then counting (the restatement of
    test_device_8psk_simulation_counters_match_cpu_pipeline), with straggler pooling on and off"""
    from ldpc_toolbox_amd import sharding
    m = cc.bits_of(name)
    s = simulator(name, max_log, -m, impl="HLMinsumf32")
    msgs, tx = s.pool_data()
    llrs, idx = s.generate(ebn0, 5, FIRST, FRAMES)
    assert same_bits(llrs, cc.chain_llrs(tx[idx], name, max_log, -m, sim.noise_sigma(s.rate, ebn0, m), 5, FIRST))
    bits, its, _ = oracle.decode_batch(oracle.Graph(alist()), "HLMinsumf32", llrs, 25, threads=8, want_posterior=False)
    st = sim.fold_statistics(ebn0, s.k, msgs[idx], bits, its, 25, 1.0)
    want = sharding.counters_from_statistics(st)
    print(f"{name} max_log={max_log} {ebn0} dB: counters {[int(x) for x in want]}")
    assert 0 < want[2] < FRAMES                                     # some frame errors, not all
    first = s.run(ebn0, 5, FIRST, FRAMES, 25)
    again = s.run(ebn0, 5, FIRST, FRAMES, 25)       # (the second call at a point may run a reduced budget and pool)
    assert np.array_equal(first, want) and np.array_equal(again, want), (first, again, want)
    s.set("pooling", 0)
    assert np.array_equal(s.run(ebn0, 5, FIRST, FRAMES, 25), want)
    s.close()


# ---- 4: refusals --------------------------------------------------------------------------------------------

def test_refusals_leave_the_previous_setting_working():
    s = lt.Simulator(alist(), "Minsumf32", device=0, pool_size=16, pool_seed=9, modulation="8PSK", interleaving=3)
    base, _ = s.generate(4.0, 21, FIRST, 8)
    assert (s.get("modulation"), s.get("constellation"), s.get("max_log")) == (3, 0, 0)
    # mean energy 1.1
    hot = lt.Demodulator(cc.TABLES["rings16"][0] * np.sqrt(1.1), energy_term=True, device=0)
    with pytest.raises(ValueError, match="energy"):
        s.set_constellation(hot, True)
    assert (s.get("modulation"), s.get("constellation"), s.get("max_log")) == (3, 0, 0)
    assert same_bits(s.generate(4.0, 21, FIRST, 8)[0], base)
    # a constellation in force survives a refusal too
    q = cc.make_demodulator(lt, "QPSK")
    s.set_constellation(q, True)
    assert (s.get("modulation"), s.get("constellation"), s.get("max_log")) == (2, 1, 1)
    qllrs, _ = s.generate(4.0, 21, FIRST, 8)
    assert not np.array_equal(qllrs, base)
    with pytest.raises(ValueError, match="energy"):
        s.set_constellation(hot, False)
    assert (s.get("modulation"), s.get("constellation"), s.get("max_log")) == (2, 1, 1)
    assert same_bits(s.generate(4.0, 21, FIRST, 8)[0], qllrs)
    # NULL restores "modulation"
    s.set_constellation(None)
    assert (s.get("modulation"), s.get("constellation"), s.get("max_log")) == (3, 0, 0)
    assert same_bits(s.generate(4.0, 21, FIRST, 8)[0], base)
    # a "BPSK" handle selects the BPSK generator
    b = lt.Demodulator("BPSK", device=0)
    s.set_constellation(b)
    assert (s.get("modulation"), s.get("constellation")) == (1, 1)
    plain = lt.Simulator(alist(), "Minsumf32", device=0, pool_size=16, pool_seed=9, interleaving=3)
    assert same_bits(s.generate(4.0, 21, FIRST, 8)[0], plain.generate(4.0, 21, FIRST, 8)[0])
    for d in (hot, q, b):
        d.close()
    plain.close()
    s.close()
    # n_tx not a multiple of m: nr5g:2:6 has n = 312, no multiple of 5
    short = lt.Simulator(lt.code_alist("nr5g:2:6"), "Minsumf32", device=0, pool_size=4, pool_seed=1)
    r32 = cc.make_demodulator(lt, "rings32")
    with pytest.raises(ValueError, match="multiple"):
        short.set_constellation(r32)
    assert (short.get("modulation"), short.get("constellation")) == (1, 0)
    assert short.generate(4.0, 1, 0, 4)[0].shape == (4, 312)
    with pytest.raises(ValueError):
        lt.Simulator(lt.code_alist("nr5g:2:6"), "Minsumf32", device=0, modulation=r32)
    r32.close()
    short.close()
    with pytest.raises(ValueError):
        lt.Simulator(alist(), "Minsumf32", device=0, modulation="16APSK")
    with pytest.raises(ValueError):
        lt.Simulator(alist(), "Minsumf32", device=0, modulation="8PSK", max_log=True)


# ---- 5: the sweep driver --------------------------------------------------------------------------------------

def _sweep_args(extra):
    return ["--code", SPEC, "--decoder", "Minsumf32", "--min-ebn0", "1.0", "--max-ebn0", "2.0", "--step-ebn0", "1.0",
            "--max-iter", "25", "--frame-errors", "1000000", "--max-frames", "512", "--frames-per-batch", "512", "--seed", "3"] + extra


def _counters(results):
    return [(r.num_frames, r.ldpc.bit_errors, r.ldpc.frame_errors, r.false_decodes) for r in results]


def test_ber_driver_qpsk_and_constellation_file(tmp_path, capsys):
    from ldpc_toolbox_amd import ber
    # --modulation QPSK
    res = ber.main(_sweep_args(["--modulation", "QPSK"]))
    out = capsys.readouterr().out
    assert " - Modulation: QPSK\n" in out and "max-log" not in out and "Bits per symbol" not in out
    s = lt.Simulator(alist(), "Minsumf32", device=0, pool_size=64, pool_seed=4, modulation="QPSK")
    direct = ber.sweep(s, [1.0, 2.0], 25, 1000000, max_frames=512, frames_per_batch=512, seed=3)
    assert [r.ebn0_db for r in res] == [1.0, 2.0] and _counters(res) == _counters(direct)
    assert res[0].ldpc.frame_errors > res[1].ldpc.frame_errors and 0 < res[0].ldpc.frame_errors < 512
    s.close()
    # --constellation FILE --max-log: the file's points are scaled to unit mean energy
    pts = cc.TABLES["rings16"][0]
    f = tmp_path / "rings16.txt"
    f.write_text("".join(f"{float((1.7 * p).real)!r} {float((1.7 * p).imag)!r}\n" for p in pts))
    args = _sweep_args(["--constellation", str(f), "--max-log"])
    args[args.index("--min-ebn0") + 1], args[args.index("--max-ebn0") + 1] = "5.0", "6.0"
    res = ber.main(args)
    out = capsys.readouterr().out
    assert f" - Modulation: constellation {f}\n - Bits per symbol: 4\n - Demodulator: max-log\n" in out
    scaled, energy_term = ber.read_constellation(str(f))
    assert energy_term and np.allclose(scaled, pts, rtol=0, atol=1e-14)
    d = lt.Demodulator(scaled, energy_term=True, device=0)
    s = lt.Simulator(alist(), "Minsumf32", device=0, pool_size=64, pool_seed=4, modulation=d, max_log=True)
    direct = ber.sweep(s, [5.0, 6.0], 25, 1000000, max_frames=512, frames_per_batch=512, seed=3)
    assert _counters(res) == _counters(direct) and res[0].ldpc.frame_errors > res[1].ldpc.frame_errors
    d.close()
    s.close()


def test_ber_driver_details_of_a_plain_bpsk_run_are_unchanged(capsys):
    """the parameter block of a run without the new options, line for line as before them"""
    from ldpc_toolbox_amd import ber
    ber.main(_sweep_args([]))
    out = capsys.readouterr().out
    want = ("BER TEST PARAMETERS\n-------------------\nSimulation:\n - Minimum Eb/N0: 1.00 dB\n - Maximum Eb/N0: 2.00 dB\n"
            " - Eb/N0 step: 1.00 dB\n - Number of frame errors: 1000000\n - Maximum number of frames per Eb/N0: 512\n"
            " - Number of GPUs: 1\nChannel:\n - Modulation: BPSK\nLDPC code:\n - alist: nr5g:2:15\n"
            " - Information bits (k): 150\n - Codeword size (N_cw): 780\n - Frame size (N): 780\n - Code rate: 0.192\n"
            "LDPC decoder:\n - Implementation: Minsumf32\n - Maximum iterations: 25\n\n")
    assert out.startswith(want)
