#!/usr/bin/env python3
"""Timings of the NR demapper with a scale per symbol and of the Rayleigh block-fading channel on one MI355X
(profiles/nr_csi_gpu.txt): device entries on one stream, device events around `reps` back-to-back calls after warm-up, 4096
frames of E = 26112 LLRs for each QM, as tools/bench_nr_qam.py -- the max-log f32 CSI demapper beside the scalar max-log f32
demapper, the 8-bit CSI demapper beside the 8-bit scalar one, with the ratio of the times next to the ratio of the bytes
((12 + 4 QM) / (8 + 4 QM) for f32, (12 + QM) / (8 + QM) for soft bits); the exact QM = 4 pair; the fading channel beside the
AWGN channel; and the simulator's fused generator (nr5g:1:384, n = 26112) with and without fading, host time around calls
that synchronise.  --output FILE: the lines go there as well."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ldpc_toolbox_amd as lt  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--frames", type=int, default=4096)
ap.add_argument("--block", type=int, default=12, help="symbols per gain: 12 is one resource block of an OFDM symbol")
ap.add_argument("--no-generator", action="store_true")
ap.add_argument("--output")
a = ap.parse_args()
DEV = torch.device("cuda", 0)
FRAMES, E = a.frames, 26112
stream = torch.cuda.Stream(device=DEV)
st = stream.cuda_stream
out_file = open(a.output, "w") if a.output else None


def say(line):
    print(line, flush=True)
    if out_file:
        out_file.write(line + "\n")
        out_file.flush()


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    stream.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        t0.record()
    for _ in range(reps):
        fn()
    with torch.cuda.stream(stream):
        t1.record()
    stream.synchronize()
    return t0.elapsed_time(t1) / reps      # ms


rng = np.random.default_rng(1)
d_bits = torch.from_numpy(rng.integers(0, 2, (FRAMES, E), dtype=np.uint8)).to(DEV)
chan = lt.Demodulator("QPSK", device=0)      # (the channels read nothing of the handle's table)
SIGMA = 0.1
for qm in (2, 4, 6, 8):
    q = lt.NrQam(qm, device=0)
    S = E // qm
    sym = FRAMES * S
    d_clean = torch.zeros((FRAMES, 2 * S), dtype=torch.float32, device=DEV)
    d_sym = torch.zeros((FRAMES, 2 * S), dtype=torch.float32, device=DEV)
    d_scale = torch.zeros((FRAMES, S), dtype=torch.float32, device=DEV)
    d_llr = torch.zeros((FRAMES, E), dtype=torch.float32, device=DEV)
    d_i8 = torch.zeros((FRAMES, E), dtype=torch.int8, device=DEV)
    q.modulate_device(d_bits.data_ptr(), d_clean.data_ptr(), False, FRAMES, E, -1, st)
    stream.synchronize()
    d_sym.copy_(d_clean)
    # the channels: in place on symbols that grow noisier from call to call, which changes no timing
    ta = timed(lambda: chan.add_noise_device(d_sym.data_ptr(), False, FRAMES, S, SIGMA, 9, 0, st), a.reps)
    tf = timed(lambda: chan.add_fading_device(d_sym.data_ptr(), d_scale.data_ptr(), False, FRAMES, S, SIGMA, a.block, 9, 0, st), a.reps)
    say(f"QM {qm} channel f32, {sym} symbols: AWGN {ta * 1e3:8.1f} us ({sym * 16} B), fading ({a.block} symbols per gain) {tf * 1e3:8.1f} us "
        f"({sym * 20} B); ratio {tf / ta:.2f}, bytes {20 / 16:.2f}")
    d_sym.copy_(d_clean)
    chan.add_fading_device(d_sym.data_ptr(), d_scale.data_ptr(), False, FRAMES, S, SIGMA, a.block, 9, 0, st)
    stream.synchronize()
    td = timed(lambda: q.demodulate_device(d_sym.data_ptr(), d_llr.data_ptr(), False, FRAMES, S, SIGMA, True, -1, st), a.reps)
    tc = timed(lambda: q.demodulate_csi_device(d_sym.data_ptr(), d_scale.data_ptr(), d_llr.data_ptr(), False, FRAMES, S, True, -1, st), a.reps)
    db, cb = sym * (8 + 4 * qm), sym * (12 + 4 * qm)
    say(f"QM {qm} max-log f32: scalar {td * 1e3:8.1f} us, {db / td / 1e9:6.3f} TB/s;  CSI {tc * 1e3:8.1f} us, {cb / tc / 1e9:6.3f} TB/s;  "
        f"ratio {tc / td:.3f}, bytes {cb / db:.3f}")
    td8 = timed(lambda: q.demap_i8_device(d_sym.data_ptr(), d_i8.data_ptr(), FRAMES, S, SIGMA, True, -1, st), a.reps)
    tc8 = timed(lambda: q.demap_csi_i8_device(d_sym.data_ptr(), d_scale.data_ptr(), d_i8.data_ptr(), FRAMES, S, True, -1, st), a.reps)
    db8, cb8 = sym * (8 + qm), sym * (12 + qm)
    say(f"QM {qm} max-log  i8: scalar {td8 * 1e3:8.1f} us, {db8 / td8 / 1e9:6.3f} TB/s;  CSI {tc8 * 1e3:8.1f} us, {cb8 / tc8 / 1e9:6.3f} TB/s;  "
        f"ratio {tc8 / td8:.3f}, bytes {cb8 / db8:.3f}")
    if qm == 4:
        few = max(a.reps // 4, 2)
        tef = timed(lambda: q.demodulate_device(d_sym.data_ptr(), d_llr.data_ptr(), False, FRAMES, S, SIGMA, False, -1, st), few, 1)
        tcf = timed(lambda: q.demodulate_csi_device(d_sym.data_ptr(), d_scale.data_ptr(), d_llr.data_ptr(), False, FRAMES, S, False, -1, st), few, 1)
        d_sym64, d_scale64 = d_sym.to(torch.float64), d_scale.to(torch.float64)
        d_llr64 = torch.zeros((FRAMES, E), dtype=torch.float64, device=DEV)
        te = timed(lambda: q.demodulate_device(d_sym64.data_ptr(), d_llr64.data_ptr(), True, FRAMES, S, SIGMA, False, -1, st), few, 1)
        tce = timed(lambda: q.demodulate_csi_device(d_sym64.data_ptr(), d_scale64.data_ptr(), d_llr64.data_ptr(), True, FRAMES, S, False, -1, st),
                    few, 1)
        say(f"QM 4 exact: f32 entries scalar {tef:7.3f} ms, CSI {tcf:7.3f} ms, ratio {tcf / tef:.3f};  f64 entries scalar {te:7.3f} ms, "
            f"CSI {tce:7.3f} ms, ratio {tce / te:.3f}")
        del d_sym64, d_scale64, d_llr64
    q.close()
    del d_clean, d_sym, d_scale, d_llr, d_i8
chan.close()
del d_bits

if not a.no_generator:
    # the fused generator: frames of nr5g:1:384 (n = 26112) written straight into a device buffer; `generate` synchronises
    s = lt.Simulator(lt.code_alist("nr5g:1:384"), "Minsumf32", device=0, pool_size=16, pool_seed=5)
    assert s.n_tx == E
    d_out = torch.zeros((FRAMES, E), dtype=torch.float32, device=DEV)

    def wall(fn, reps, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3   # ms

    for qm in (2, 4, 6, 8):
        q = lt.NrQam(qm)
        for max_log in (True, False):
            if not max_log and qm not in (4, 8):
                continue
            s.set_nr_qam(q, max_log)
            reps = a.reps if max_log else max(a.reps // 4, 2)
            s.set("fading_block", 0)
            t0 = wall(lambda: s.generate_into(d_out.data_ptr(), 4.0, 7, 0, FRAMES), reps)
            s.set("fading_block", a.block)
            t1 = wall(lambda: s.generate_into(d_out.data_ptr(), 4.0, 7, 0, FRAMES), reps)
            say(f"QM {qm} generator {'max-log' if max_log else 'exact  '}: AWGN {t0:8.3f} ms, fading ({a.block} symbols per gain) {t1:8.3f} ms, "
                f"ratio {t1 / t0:.3f}  ({FRAMES * E // qm} symbols)")
        s.set("fading_block", 0)
        s.set_nr_qam(None)
        q.close()
    s.close()
if out_file:
    out_file.close()
