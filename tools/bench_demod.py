#!/usr/bin/env python3
"""Cost of the batched GPU demodulator in front of the decoder, on the machine it runs on.

Workload: --frames DVB-S2 normal frames (dvbs2:R1_2, 21600 8PSK symbols each, interleaving 3), device-resident, f32.
Encoded on the GPU, mapped and given noise at --ebn0 with torch (set-up only).  hipEvent-timed on a stream of the
caller's, warm, median of --calls calls:
  * exact `demod_run_f32_device`: symbols/s, and its time as a fraction of decoding the same LLRs (Minsumf32,
    --iterations iterations, device entry, measured in the same run);
  * max-log `demod_run_f32_device`: bytes moved (8 B symbol in + 12 B LLRs out = 20 B per symbol) per second, as a
    fraction of the 6.29 TB/s copy rate DESIGN.md section 5 records;
  * host baseline: the oracle's psk8_demodulate, one thread, 64 frames.

    python tools/bench_demod.py [--frames 4096] [--calls 20] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ldpc_toolbox_amd as lt  # noqa: E402
from ldpc_toolbox_amd import simulation as sim  # noqa: E402

COPY_RATE = 6.29e12      # bytes/s, DESIGN.md section 5
A = 0.70710678118654757
PSK8 = [(A, A), (1.0, 0.0), (-1.0, 0.0), (-A, -A), (0.0, 1.0), (A, -A), (-A, A), (0.0, -1.0)]   # at index b0 b1 b2


def timed(stream, call, calls):
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
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--ebn0", type=float, default=3.0)
    ap.add_argument("--host-frames", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures nothing without one")
    dev = torch.device("cuda:0")
    alist = lt.code_alist(args.code)
    enc = lt.Encoder(alist, device=0)
    dec = lt.LdpcDecoder(alist, "Minsumf32", device=0)
    demod = lt.Demodulator("8PSK", device=0)
    n, k, B = dec.n, dec.k, args.frames
    S = n // 3
    sigma = sim.noise_sigma(k / n, args.ebn0, 3.0)
    emit(f"batched GPU demodulator -- {torch.cuda.get_device_name(0)}; {args.code}: n = {n}, {S} 8PSK symbols per frame, "
         f"{B} frames, interleaving 3, Eb/N0 {args.ebn0} dB (sigma {sigma:.4f}), f32")

    # set-up: encode on the GPU, interleave (columns 3), map, add noise
    gen = torch.Generator(device=dev).manual_seed(1)
    msgs = torch.randint(0, 2, (B, k), dtype=torch.uint8, device=dev, generator=gen)
    cws = torch.zeros((B, n), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    enc.encode_batch_device(msgs.data_ptr(), cws.data_ptr(), B)
    bits = cws.view(B, 3, S).transpose(1, 2).to(torch.int64)              # interleaved: symbol s carries cw[c * S + s]
    label = bits[..., 0] * 4 + bits[..., 1] * 2 + bits[..., 2]
    del bits
    table = torch.tensor(PSK8, dtype=torch.float32, device=dev)
    syms = table[label] + float(sigma) * torch.randn((B, S, 2), dtype=torch.float32, device=dev, generator=gen)
    del label
    syms = syms.contiguous()
    llrs = torch.zeros((B, n), dtype=torch.float32, device=dev)
    out_bits = torch.zeros((B, n), dtype=torch.uint8, device=dev)
    its = torch.zeros(B, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def run_demod(max_log):
        demod.demodulate_device(syms.data_ptr(), llrs.data_ptr(), False, B, S, sigma, 3, max_log, stream.cuda_stream)

    def run_decode():
        dec.decode_batch_device(llrs.data_ptr(), False, B, args.iterations, out_bits.data_ptr(), n, its.data_ptr(), 0,
                                stream.cuda_stream)

    ml_s, ml_lo, ml_hi = timed(stream, lambda: run_demod(True), args.calls)
    ex_s, ex_lo, ex_hi = timed(stream, lambda: run_demod(False), args.calls)      # leaves the exact LLRs in place
    # the first frames against the oracle (exact path), then the decode of those LLRs
    import oracle_binding as ob
    head = syms[:2].cpu().numpy().astype(np.float64)
    for f in range(2):
        want = ob.deinterleave(ob.psk8_demodulate(head[f, :, 0] + 1j * head[f, :, 1], sigma), 3).astype(np.float32)
        if not np.array_equal(llrs[f].cpu().numpy(), want):
            raise SystemExit(f"frame {f}: the GPU LLRs differ from the oracle's")
    de_s, de_lo, de_hi = timed(stream, run_decode, max(args.calls // 2, 5))
    failed = int((its < 0).sum().item())
    total = B * S
    emit(f"  exact   demod_run_f32_device, median of {args.calls} calls: {ex_s * 1e3:8.3f} ms (min {ex_lo * 1e3:.3f}, max {ex_hi * 1e3:.3f})"
         f"  = {total / ex_s / 1e9:7.2f} G symbols/s = {B / ex_s:9.0f} frames/s")
    emit(f"  decode  Minsumf32, {args.iterations} iterations, device entry:  {de_s * 1e3:8.3f} ms (min {de_lo * 1e3:.3f}, max {de_hi * 1e3:.3f})"
         f"  = {B / de_s:9.0f} frames/s, {failed} of {B} frames not decoded")
    emit(f"  exact demodulation / decode time: {ex_s / de_s:.3f}  ({'more' if ex_s > 0.1 * de_s else 'not more'} than a tenth)")
    rate = 20.0 * total / ml_s
    emit(f"  max-log demod_run_f32_device, median of {args.calls} calls: {ml_s * 1e3:8.3f} ms (min {ml_lo * 1e3:.3f}, max {ml_hi * 1e3:.3f})"
         f"  = {total / ml_s / 1e9:7.2f} G symbols/s; 20 B per symbol -> {rate / 1e12:.3f} TB/s"
         f" = {100 * rate / COPY_RATE:.1f} % of the {COPY_RATE / 1e12:.2f} TB/s copy rate")
    hf = min(args.host_frames, B)
    host = syms[:hf].cpu().numpy().astype(np.float64)
    host = host[..., 0] + 1j * host[..., 1]
    t0 = time.perf_counter()
    for f in range(hf):
        ob.psk8_demodulate(host[f], sigma)
    host_s = (time.perf_counter() - t0) / hf
    emit(f"  host    oracle psk8_demodulate, 1 thread, {hf} frames: {host_s * 1e3:8.3f} ms / frame = {S / host_s / 1e6:7.2f} M symbols/s"
         f" = {1 / host_s:9.0f} frames/s;  GPU exact / host: {(total / ex_s) / (S / host_s):.0f}x")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
