#!/usr/bin/env python3
"""Cost of the batched GPU modulator, the AWGN channel and the simulator's fused constellation generator, on the machine
it runs on.

Workload: --frames DVB-S2 normal frames (dvbs2:R1_2, n = 64800 bits: 64800 / m symbols each, interleaving m), device-
resident.  One timing per process (--what), warm, median of --calls calls:
  * mod    `mod_run_f32_device` on a stream of the caller's, hipEvent-timed: n bytes of bits in, 8 n / m bytes of symbols out;
  * awgn   `awgn_run_f32_device`, in place: 8 bytes read and 8 written per symbol;
  * fused  `Simulator(modulation=<constellation>).generate_into` (host wall clock around the synchronous call: one kernel
           launch, a stream synchronisation and the frames' pool indices): 4 n bytes of LLRs out, no symbols stored;
  * psk8   the same call with modulation="8PSK": gen::psk8_llr_kernel, the kernel `--what fused --m 3` is measured against;
  * share  generation's share of a `Simulator.run` at this code (8PSK handle, --iterations iterations).
Constellations: m = 2 QPSK, m = 3 8PSK, m = 4, 5: rings of unequal energy scaled to unit mean energy, energy term on.

    python tools/bench_modulator.py --what fused --m 4 [--max-log] [--frames 4096] [--calls 20] [--out FILE]
    python tools/bench_modulator.py --what all        # every timing in this process, one after the other
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch  # before the library: one HIP runtime per process (tests/conftest.py)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import ldpc_toolbox_amd as lt  # noqa: E402
from ldpc_toolbox_amd import simulation as sim  # noqa: E402


def rings(m):
    n = 1 << m
    r = np.where(np.arange(n) % 2 == 0, 0.6, np.sqrt(2.0 - 0.36))
    return r * np.exp(2j * np.pi * (np.arange(n) + 0.25) / n)


def constellation(m):
    if m in (2, 3):
        return lt.Demodulator({2: "QPSK", 3: "8PSK"}[m], device=0)
    return lt.Demodulator(rings(m), energy_term=True, device=0)


def event_timed(stream, call, calls):
    for _ in range(3):
        call()
    stream.synchronize()
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(times), min(times), max(times)


def wall_timed(call, calls):
    for _ in range(3):
        call()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def fmt(t):
    return f"{t[0] * 1e3:8.3f} ms (min {t[1] * 1e3:.3f}, max {t[2] * 1e3:.3f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", choices=["mod", "awgn", "fused", "psk8", "share", "all"], default="all")
    ap.add_argument("--m", type=int, default=3, choices=[2, 3, 4, 5])
    ap.add_argument("--max-log", action="store_true")
    ap.add_argument("--code", default="dvbs2:R1_2")
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--ebn0", type=float, default=3.0)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures nothing without one")
    dev = torch.device("cuda:0")
    alist = lt.code_alist(args.code)
    B = args.frames

    def bench_mod_awgn(what, m):
        d = constellation(m)
        h = lt.SparseMatrix.from_alist(alist)
        n = h.num_cols()
        S = n // m
        gen = torch.Generator(device=dev).manual_seed(1)
        bits = torch.randint(0, 2, (B, n), dtype=torch.uint8, device=dev, generator=gen)
        syms = torch.zeros((B, S, 2), dtype=torch.float32, device=dev)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        d.modulate_device(bits.data_ptr(), syms.data_ptr(), False, B, n, m, stream.cuda_stream)
        stream.synchronize()
        if what == "mod":
            t = event_timed(stream, lambda: d.modulate_device(bits.data_ptr(), syms.data_ptr(), False, B, n, m, stream.cuda_stream),
                            args.calls)
            nbytes = B * (n + 8 * S)
        else:
            t = event_timed(stream, lambda: d.add_noise_device(syms.data_ptr(), False, B, S, 0.5, 7, 0, stream.cuda_stream), args.calls)
            nbytes = B * 16 * S
        emit(f"  {what:5s} m = {m}  f32, {B} frames x {S} symbols: {fmt(t)} = {B * S / t[0] / 1e9:7.2f} G symbols/s = "
             f"{nbytes / t[0] / 1e9:8.1f} GB/s")
        d.close()

    def bench_fused(m, max_log, named_psk8=False):
        if named_psk8:
            s = lt.Simulator(alist, "Minsumf32", device=0, modulation="8PSK", interleaving=3)
            m = 3
        else:
            d = constellation(m)
            s = lt.Simulator(alist, "Minsumf32", device=0, modulation=d, interleaving=m, max_log=max_log)
            d.close()
        n = s.n_tx
        llrs = torch.zeros((B, n), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        t = wall_timed(lambda: s.generate_into(llrs.data_ptr(), args.ebn0, 7, 0, B), args.calls)
        S = n // m
        kind = "psk8_llr_kernel (modulation=8PSK)" if named_psk8 else f"table_llr_kernel<{m}, {'max-log' if max_log else 'exact'}>"
        emit(f"  fused m = {m}  {kind}, {B} frames x {S} symbols: {fmt(t)} = {B * S / t[0] / 1e9:7.2f} G symbols/s = "
             f"{B * 4 * n / t[0] / 1e9:8.1f} GB/s of LLRs")
        s.close()
        return t[0]

    def bench_share():
        d = constellation(3)
        s = lt.Simulator(alist, "Minsumf32", device=0, modulation=d, interleaving=3)
        d.close()
        llrs = torch.zeros((B, s.n_tx), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        g = wall_timed(lambda: s.generate_into(llrs.data_ptr(), args.ebn0, 7, 0, B), args.calls)
        r = wall_timed(lambda: s.run(args.ebn0, 7, 0, B, args.iterations), max(args.calls // 4, 3))
        emit(f"  share  8PSK handle, {args.code}, Eb/N0 {args.ebn0} dB, {args.iterations} iterations, {B} frames: run {fmt(r)}, "
             f"generation {fmt(g)} = {100 * g[0] / r[0]:.1f} % of a run")
        s.close()

    emit(f"batched GPU modulator / channel / fused generator -- {torch.cuda.get_device_name(0)}; {args.code}, {B} frames, f32")
    if args.what in ("mod", "awgn"):
        bench_mod_awgn(args.what, args.m)
    elif args.what == "fused":
        bench_fused(args.m, args.max_log)
    elif args.what == "psk8":
        bench_fused(3, False, named_psk8=True)
    elif args.what == "share":
        bench_share()
    else:
        for m in (2, 3, 4, 5):
            bench_mod_awgn("mod", m)
            bench_mod_awgn("awgn", m)
            for max_log in (False, True):
                bench_fused(m, max_log)
        old, new = bench_fused(3, False, named_psk8=True), bench_fused(3, False)
        emit(f"  table form / psk8_llr_kernel: {new / old:.3f}")
        bench_share()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
