#!/usr/bin/env python3
"""Cost of the batched GPU BCH encoder and decoder, on the machine it runs on.

Workload: --frames frames of --code (default dvbs2:R1_2: n = 32400, k = 32208, t = 12), device-resident, on a stream of
the caller's, hipEvent-timed, warm, median of --calls calls:
  * encode        `bch_encode_batch_device`: k bytes in, n bytes out per frame;
  * decode clean  `bch_decode_batch_device` on codewords: the remainder kernel finishes every frame (n bytes in, k out);
  * decode t      ... every frame with t errors: remainder, locator and root search for all of them;
  * decode 1%     ... one frame in a hundred with 1..t errors -- what follows a working LDPC decoder.

    python tools/bench_bch.py [--code dvbs2:R1_2] [--frames 4096] [--calls 20] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--code", default="dvbs2:R1_2")
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    code = lt.BchCode(args.code, device=0)
    n, k, t, B = code.n, code.k, code.t, args.frames
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    msgs = torch.from_numpy(rng.integers(0, 2, (B, k), dtype=np.uint8)).to(dev)
    cws = torch.zeros((B, n), dtype=torch.uint8, device=dev)
    out = torch.zeros((B, k), dtype=torch.uint8, device=dev)
    err = torch.zeros(B, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    st = stream.cuda_stream
    emit(f"{args.code}: n = {n}, k = {k}, t = {t}; {B} frames per call, median of {args.calls} calls (min, max)")

    def report(name, timing, bytes_per_frame):
        med, lo, hi = timing
        emit(f"  {name:<13} {med * 1e3:8.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})  {B / med * 1e-6:7.3f} Mframes/s  "
             f"{B * n / med * 1e-9:7.2f} Gbit/s of code bits  {B * bytes_per_frame / med * 1e-9:7.1f} GB/s moved")

    report("encode", event_timed(stream, lambda: code.encode_device(msgs.data_ptr(), cws.data_ptr(), B, stream=st), args.calls), k + n)
    stream.synchronize()
    clean = cws.cpu().numpy()

    def decode_case(name, rows, want_errors):
        d_in = torch.from_numpy(rows).to(dev)
        torch.cuda.synchronize()
        timing = event_timed(stream, lambda: code.decode_device(d_in.data_ptr(), out.data_ptr(), B, errors_ptr=err.data_ptr(), stream=st),
                             args.calls)
        stream.synchronize()
        assert np.array_equal(err.cpu().numpy(), want_errors) and torch.equal(out, msgs), name
        report(name, timing, n + k)

    decode_case("decode clean", clean, np.zeros(B, dtype=np.int32))
    rows = clean.copy()
    for f in range(B):
        rows[f, rng.choice(n, t, replace=False)] ^= 1
    decode_case("decode t", rows, np.full(B, t, dtype=np.int32))
    rows, want = clean.copy(), np.zeros(B, dtype=np.int32)
    for f in range(0, B, 100):
        want[f] = 1 + (f // 100) % t
        rows[f, rng.choice(n, want[f], replace=False)] ^= 1
    decode_case("decode 1%", rows, want)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
