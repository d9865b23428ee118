#!/usr/bin/env python3
"""Cost of batched NR rate matching and rate recovery, on the machine it runs on, beside a device-to-device copy.

Workload: --frames frames of --code (default nr5g:1:384: n = 26112, L = N = 25344), device-resident, on a stream of the
caller's, hipEvent-timed, warm, median of --calls calls, for each E of --e (default: N, and 2 L + 384 -- every column
twice and 384 of them three times), rv 0, --qm rows, f32:
  * match     `match_device`: codewords [frames][n] bytes -> [frames][E] bytes;
  * recover   `recover_device` (f32, combine = 0): [frames][E] floats -> [frames][n] floats;
  * copy      a device-to-device copy that moves the same bytes (half read, half written), timed in the same run, call
              by call in turn with the kernel it is the yardstick of.
Bytes moved = the input rows plus the output rows of a call.

    python tools/bench_nr_rate_match.py [--code nr5g:1:384] [--frames 8192] [--calls 20] [--qm 2] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch  # before the library: one HIP runtime per process (tests/conftest.py)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import ldpc_toolbox_amd as lt  # noqa: E402


def timed_in_turn(stream, calls_by_name, calls):
    """every callable 3 times warm, then `calls` rounds of one call each in turn -> {name: (median, min, max)} seconds"""
    for _ in range(3):
        for call in calls_by_name.values():
            call()
    stream.synchronize()
    times = {name: [] for name in calls_by_name}
    for _ in range(calls):
        for name, call in calls_by_name.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e-3)
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--code", default="nr5g:1:384")
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--qm", type=int, default=2)
    ap.add_argument("--e", type=int, nargs="*", default=None)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    rm = lt.NrRateMatcher(args.code, device=0)
    n, L, B, qm = rm.n, rm.buffer_len, args.frames, args.qm
    es = args.e or [rm.n_cb, 2 * L + rm.zc]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    emit(f"{args.code}: n = {n}, L = {L}; {B} frames per call, rv 0, Qm {qm}, f32; median of {args.calls} calls (min, max)")
    for e in es:
        cws = torch.randint(0, 2, (B, n), dtype=torch.uint8, device=dev, generator=gen)
        tx = torch.zeros((B, e), dtype=torch.uint8, device=dev)
        rx = torch.randn((B, e), dtype=torch.float32, device=dev, generator=gen)
        llrs = torch.zeros((B, n), dtype=torch.float32, device=dev)
        mbytes, rbytes = B * (n + e), 4 * B * (e + n)
        src = torch.zeros(rbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.zeros(rbytes // 2, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def copy(nbytes):
            with torch.cuda.stream(stream):
                dst[:nbytes // 2].copy_(src[:nbytes // 2], non_blocking=True)

        t = timed_in_turn(stream, {
            "match": lambda: rm.match_device(cws.data_ptr(), tx.data_ptr(), B, e, 0, qm, stream=st),
            "copy(match)": lambda: copy(mbytes),
            "recover": lambda: rm.recover_device(rx.data_ptr(), llrs.data_ptr(), False, B, e, 0, qm, stream=st),
            "copy(recover)": lambda: copy(rbytes),
        }, args.calls)
        stream.synchronize()
        emit(f" E = {e} (rate {rm.k}/{e} = {rm.k / e:.3f}; up to {-(-e // L)} repeats of a column)")
        for name, nbytes in (("match", mbytes), ("copy(match)", mbytes), ("recover", rbytes), ("copy(recover)", rbytes)):
            med, lo, hi = t[name]
            emit(f"  {name:<14} {med * 1e3:8.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})  {nbytes * 1e-6:9.1f} MB moved  "
                 f"{nbytes / med * 1e-9:8.1f} GB/s  {B / med * 1e-6:7.3f} Mframes/s")
        emit(f"  match / copy = {t['match'][0] / t['copy(match)'][0]:.2f}    recover / copy = {t['recover'][0] / t['copy(recover)'][0]:.2f}")
        del cws, tx, rx, llrs, src, dst
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
