#!/usr/bin/env python3
"""Cost of the batched NR transport block entries, on the machine it runs on, beside a device-to-device copy.

Workload: for each --shape BG:A:BLOCKS (default 1:8424:8192 -- one code block of 8448 bits per transport block -- and
1:1277992:64 -- 152 code blocks each), device-resident, on a stream of the caller's, hipEvent-timed, warm, median of
--calls calls:
  * segment      `segment_device`: payload [blocks][A] bytes -> rows [C * blocks][K] bytes;
  * desegment    `desegment_device`: rows -> payload, tb_ok, cb_ok;
  * concatenate  `concatenate_device`: packed rows -> [blocks][G] bytes, G = 3 K' C + 2 (one block two bits longer), q 2;
  * split        `split_f32_device`: [blocks][G] floats -> packed rows;
  * copy         a device-to-device copy that moves the same bytes (half read, half written), timed in the same run, call
                 by call in turn with the entry it is the yardstick of.
Bytes moved = the input plus the output of a call.

    python tools/bench_nr_transport_block.py [--shape 1:8424:8192 ...] [--calls 20] [--out FILE]
"""
import argparse
import os
import statistics
import sys

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
    ap.add_argument("--shape", nargs="*", default=["1:8424:8192", "1:1277992:64"], help="BG:A:BLOCKS")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    for shape in args.shape:
        bg, a, B = (int(x) for x in shape.split(":"))
        tb = lt.NrTransportBlock(f"nr5g-tb:{bg}:{a}", device=0)
        c, k = tb.c, tb.k
        q = 2
        g = (3 * (tb.k_prime // 2) * c + 1) * q
        e_lo, e_hi, c_lo = tb.block_lengths(g, q)
        emit(f"nr5g-tb:{bg}:{a}: C = {c}, K' = {tb.k_prime}, K = {k}, F = {tb.fillers}; {B} transport blocks per call; "
             f"G = {g} ({c_lo} blocks of {e_lo}, {c - c_lo} of {e_hi}); median of {args.calls} calls (min, max)")
        payload = torch.randint(0, 2, (B, a), dtype=torch.uint8, device=dev, generator=gen)
        rows = torch.zeros((c * B, k), dtype=torch.uint8, device=dev)
        back = torch.zeros((B, a), dtype=torch.uint8, device=dev)
        tb_ok = torch.zeros(B, dtype=torch.uint8, device=dev)
        cb_ok = torch.zeros((B, c), dtype=torch.uint8, device=dev)
        packed = torch.randint(0, 2, (B * g,), dtype=torch.uint8, device=dev, generator=gen)
        tx = torch.zeros((B, g), dtype=torch.uint8, device=dev)
        rx = torch.randn((B, g), dtype=torch.float32, device=dev, generator=gen)
        sp = torch.zeros(B * g, dtype=torch.float32, device=dev)
        nbytes = {"segment": B * a + c * B * k, "desegment": c * B * tb.k_prime + B * a + B * (c + 1), "concatenate": 2 * B * g,
                  "split": 8 * B * g}
        most = max(nbytes.values())
        src = torch.zeros(most // 2, dtype=torch.uint8, device=dev)
        dst = torch.zeros(most // 2, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def copy(count):
            with torch.cuda.stream(stream):
                dst[:count // 2].copy_(src[:count // 2], non_blocking=True)

        entries = {
            "segment": lambda: tb.segment_device(payload.data_ptr(), rows.data_ptr(), B, stream=st),
            "desegment": lambda: tb.desegment_device(rows.data_ptr(), back.data_ptr(), tb_ok.data_ptr(), cb_ok.data_ptr(), B, stream=st),
            "concatenate": lambda: tb.concatenate_device(packed.data_ptr(), tx.data_ptr(), B, g, q, stream=st),
            "split": lambda: tb.split_device(rx.data_ptr(), sp.data_ptr(), False, B, g, q, stream=st),
        }
        calls = {}
        for name, call in entries.items():
            calls[name] = call
            calls[f"copy({name})"] = (lambda count: lambda: copy(count))(nbytes[name])
        t = timed_in_turn(stream, calls, args.calls)
        stream.synchronize()
        if not (bool(tb_ok.all()) and bool(cb_ok.all()) and torch.equal(back, payload)):
            raise SystemExit("desegment of segment did not return the payload with every flag set")
        for name in entries:
            for label in (name, f"copy({name})"):
                med, lo, hi = t[label]
                emit(f"  {label:<18} {med * 1e3:8.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})  {nbytes[name] * 1e-6:9.1f} MB moved  "
                     f"{nbytes[name] / med * 1e-9:8.1f} GB/s  {B / med * 1e-6:7.3f} Mblocks/s")
        emit("  " + "    ".join(f"{name} / copy = {t[name][0] / t[f'copy({name})'][0]:.2f}" for name in entries))
        tb.close()
        del payload, rows, back, packed, tx, rx, sp, src, dst
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
