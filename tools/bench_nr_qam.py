#!/usr/bin/env python3
"""Timings of the NR modulation entries on one MI355X (profiles/nr_qam_gpu.txt): device entries on one stream, device
events around `reps` back-to-back calls after warm-up, 4096 frames of E = 26112 bits / LLRs for each QM -- the f32 mapper
and the f32 max-log demapper with and without scrambling, bytes moved over time; the exact f64 demapper for QM = 4 beside
the table demapper on the same 16 points with the energy term; the Gold kernel for 10^6 bits as the difference between a
mapper call that has to generate the sequence and one that finds it cached."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ldpc_toolbox_amd as lt  # noqa: E402
import nr_qam_reference as nq  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--frames", type=int, default=4096)
a = ap.parse_args()
DEV = torch.device("cuda", 0)
FRAMES, E = a.frames, 26112
stream = torch.cuda.Stream(device=DEV)
st = stream.cuda_stream


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
for qm in (2, 4, 6, 8):
    q = lt.NrQam(qm, device=0)
    S = E // qm
    d_sym = torch.zeros((FRAMES, 2 * S), dtype=torch.float32, device=DEV)
    d_llr = torch.zeros((FRAMES, E), dtype=torch.float32, device=DEV)
    for c_init in (-1, 12345):
        tm = timed(lambda: q.modulate_device(d_bits.data_ptr(), d_sym.data_ptr(), False, FRAMES, E, c_init, st), a.reps)
        d_sym.add_(0.05 * torch.randn_like(d_sym))
        td = timed(lambda: q.demodulate_device(d_sym.data_ptr(), d_llr.data_ptr(), False, FRAMES, S, 0.1, True, c_init, st), a.reps)
        sym = FRAMES * S
        mb, db = sym * (qm + 8), sym * (8 + 4 * qm)
        print(f"QM {qm} c_init {c_init:6d}: mapper f32 {tm * 1e3:8.1f} us, {mb / tm / 1e9:7.3f} TB/s ({mb} B);  "
              f"max-log demapper f32 {td * 1e3:8.1f} us, {db / td / 1e9:7.3f} TB/s ({db} B)", flush=True)
    if qm == 4:
        # the exact f64 path beside the table demapper on the same 16 points with the energy term
        table = lt.Demodulator(nq.points(4), energy_term=True, device=0)
        d_sym64 = d_sym.to(torch.float64)
        d_llr64 = torch.zeros((FRAMES, E), dtype=torch.float64, device=DEV)
        d_llr64b = torch.zeros((FRAMES, E), dtype=torch.float64, device=DEV)
        te = timed(lambda: q.demodulate_device(d_sym64.data_ptr(), d_llr64.data_ptr(), True, FRAMES, S, 0.1, False, -1, st), max(a.reps // 4, 2), 1)
        tt = timed(lambda: table.demodulate_device(d_sym64.data_ptr(), d_llr64b.data_ptr(), True, FRAMES, S, 0.1, 0, False, st), max(a.reps // 4, 2), 1)
        diff = (d_llr64 - d_llr64b).abs().max().item()
        print(f"QM 4 exact f64: per-axis demapper {te:8.3f} ms, table demapper (16 points, energy term) {tt:8.3f} ms, "
              f"ratio {tt / te:.2f}; largest |difference| of the LLRs {diff:.3e}", flush=True)
        tef = timed(lambda: q.demodulate_device(d_sym.data_ptr(), d_llr.data_ptr(), False, FRAMES, S, 0.1, False, -1, st), max(a.reps // 4, 2), 1)
        print(f"QM 4 exact f32 entry (f64 arithmetic): {tef:8.3f} ms", flush=True)
        table.close()
        del d_sym64, d_llr64, d_llr64b
    if qm == 8:
        te = timed(lambda: q.demodulate_device(d_sym.data_ptr(), d_llr.data_ptr(), False, FRAMES, S, 0.1, False, -1, st), max(a.reps // 4, 2), 1)
        print(f"QM 8 exact f32 entry (f64 arithmetic): {te:8.3f} ms", flush=True)
    q.close()
    del d_sym, d_llr

# the Gold kernel for 10^6 bits: one row of 10^6 bits of QPSK, a new c_init every call (generates) against a repeated one
q = lt.NrQam(2, device=0)
n = 1000000
d_b = torch.zeros((1, n), dtype=torch.uint8, device=DEV)
d_s = torch.zeros((1, n), dtype=torch.float32, device=DEV)
state = {"c": 0}


def fresh():
    state["c"] += 1
    q.modulate_device(d_b.data_ptr(), d_s.data_ptr(), False, 1, n, state["c"], st)


t_new = timed(fresh, 50)
t_same = timed(lambda: q.modulate_device(d_b.data_ptr(), d_s.data_ptr(), False, 1, n, 7, st), 50)
print(f"Gold sequence, 10^6 bits: mapper call with a new c_init {t_new * 1e3:.1f} us, with a cached one {t_same * 1e3:.1f} us: "
      f"difference {1e3 * (t_new - t_same):.1f} us; launches {q.get('sequence_launches')}", flush=True)
