#!/usr/bin/env python3
"""Cost of the 8-bit soft-bit receive path (include/ldpc_toolbox.h, PART 9) beside its f32 counterparts, on the machine it
runs on.  Old and new alternate call by call in one process, warm, every call between two device events on the caller's
stream (the host decode entry and run_harq: a host clock around the synchronous call); median of --calls calls (min, max).
Bytes moved = the rows a call reads plus the rows it writes, each with its element size; the share is of --stream-gbs.

  recover   recover_i8_device against recover_f32_device on --code, E = N and 2 N (Qm 6), combine 0 and 1:
            (E + n [+ n]) x element bytes
  demap     demap_i8_device against demod_f32_device, QM 6 and 8, exact and max-log: symbols 8 bytes + QM x element bytes
  decode    decode_batch_i8[_device] against the f32 entries on the same frames, --decoder on --decode-codes, 15 iterations,
            early termination off (random frames: none converges): input rows x element bytes, in and (host entry) over the bus
  harq      run_harq with "soft_bits" 8 and 32 on the configuration of tools/bench_harq.py with --decoder

    python tools/bench_soft_i8.py [--only recover demap decode harq] [--out FILE]
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


def in_turn(stream, calls_by_name, calls, host_clock=False):
    """every callable twice warm, then `calls` rounds of one call each in turn -> {name: (median, min, max)} seconds"""
    for _ in range(2):
        for call in calls_by_name.values():
            call()
    stream.synchronize()
    times = {name: [] for name in calls_by_name}
    for _ in range(calls):
        for name, call in calls_by_name.items():
            if host_clock:
                t0 = time.perf_counter()
                call()
                times[name].append(time.perf_counter() - t0)
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e-3)
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", nargs="*", default=["recover", "demap", "decode", "harq"])
    ap.add_argument("--code", default="nr5g:1:384")
    ap.add_argument("--decode-codes", nargs="*", default=["dvbs2:R1_2", "nr5g:1:384"])
    ap.add_argument("--decoder", default="Minsumi8Offset")
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--decode-frames", type=int, default=4096)
    ap.add_argument("--symbols", type=int, default=4224)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--stream-gbs", type=float, default=6290.0, help="the device's stream bandwidth, GB/s")
    ap.add_argument("--harq-frames", type=int, default=0, help="frames per run_harq call (0: eight preferred batches)")
    ap.add_argument("--out", default=None, help="also append the report to this file")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def row(name, t, nbytes):
        med, lo, hi = t
        emit(f"  {name:<28} {med * 1e3:9.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})  {nbytes * 1e-6:9.1f} MB  {nbytes / med * 1e-9:8.1f} GB/s  "
             f"{100.0 * nbytes / med * 1e-9 / args.stream_gbs:5.1f} % of {args.stream_gbs:.0f} GB/s")

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)

    if "recover" in args.only:
        rm = lt.NrRateMatcher(args.code, device=0)
        n, B = rm.n, args.frames
        emit(f"recover: {args.code}, n = {n}, {B} frames, rv 0, Qm 6; bytes = (E + n [+ n with combine]) x element bytes")
        for e in (rm.n_cb, 2 * rm.n_cb):
            rx8 = torch.randint(-128, 128, (B, e), dtype=torch.int8, device=dev, generator=gen)
            rx32 = rx8.to(torch.float32)
            out8 = torch.zeros((B, n), dtype=torch.int8, device=dev)
            out32 = torch.zeros((B, n), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            for combine in (False, True):
                t = in_turn(stream, {
                    "f32": lambda: rm.recover_device(rx32.data_ptr(), out32.data_ptr(), False, B, e, 0, 6, filler_llr=20.0, combine=combine, stream=st),
                    "i8": lambda: rm.recover_i8_device(rx8.data_ptr(), out8.data_ptr(), B, e, 0, 6, combine=combine, stream=st),
                }, args.calls)
                elems = B * (e + n + (n if combine else 0))
                emit(f" E = {e}, combine {int(combine)}")
                row("recover_f32_device", t["f32"], 4 * elems)
                row("recover_i8_device", t["i8"], elems)
                emit(f"  time i8 / f32 = {t['i8'][0] / t['f32'][0]:.2f}")
            del rx8, rx32, out8, out32
        rm.close()

    if "demap" in args.only:
        B, S = args.frames, args.symbols
        emit(f"demap: {B} x {S} symbols, sigma 0.2, no scrambling; bytes = symbols x (8 + QM x element bytes)")
        for qm in (6, 8):
            qam = lt.NrQam(qm, device=0)
            sym = torch.randn((B, S, 2), dtype=torch.float32, device=dev, generator=gen) * 0.7
            out8 = torch.zeros((B, S * qm), dtype=torch.int8, device=dev)
            out32 = torch.zeros((B, S * qm), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            for max_log in (False, True):
                t = in_turn(stream, {
                    "f32": lambda: qam.demodulate_device(sym.data_ptr(), out32.data_ptr(), False, B, S, 0.2, max_log, -1, st),
                    "i8": lambda: qam.demap_i8_device(sym.data_ptr(), out8.data_ptr(), B, S, 0.2, max_log, -1, st),
                }, args.calls)
                emit(f" QM {qm}, {'max-log' if max_log else 'exact'}")
                row("demod_f32_device", t["f32"], B * S * (8 + 4 * qm))
                row("demap_i8_device", t["i8"], B * S * (8 + qm))
                emit(f"  time i8 / f32 = {t['i8'][0] / t['f32'][0]:.2f}")
            qam.close()
            del sym, out8, out32

    if "decode" in args.only:
        B = args.decode_frames
        for spec in args.decode_codes:
            dec = lt.LdpcDecoder(lt.code_alist(spec), args.decoder, device=0)
            n = dec.n
            v = np.random.default_rng(2).integers(-127, 128, (B, n)).astype(np.int8)       # random frames: all 15 iterations
            f = (v.astype(np.float32) / np.float32(8.0)).astype(np.float32)
            d_v, d_f = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
            d_bits = torch.zeros((B, dec.k), dtype=torch.uint8, device=dev)
            d_its = torch.zeros(B, dtype=torch.int32, device=dev)
            bits, its = np.zeros((B, dec.k), dtype=np.uint8), np.zeros(B, dtype=np.int32)
            torch.cuda.synchronize()
            emit(f"decode: {args.decoder} on {spec} (n = {n}), {B} frames, 15 iterations, none converges; bytes = the input rows")
            t = in_turn(stream, {
                "f32": lambda: dec.decode_batch_device(d_f.data_ptr(), False, B, 15, d_bits.data_ptr(), dec.k, d_its.data_ptr(), 0, st),
                "i8": lambda: dec.decode_batch_device(d_v.data_ptr(), False, B, 15, d_bits.data_ptr(), dec.k, d_its.data_ptr(), 0, st, i8=True),
            }, args.calls)
            row("decode_batch_f32_device", t["f32"], 4 * B * n)
            row("decode_batch_i8_device", t["i8"], B * n)
            emit(f"  time i8 / f32 = {t['i8'][0] / t['f32'][0]:.3f}")
            t = in_turn(stream, {
                "f32": lambda: dec.decode_batch(f, 15, output_len=dec.k, out=(bits, its)),
                "i8": lambda: dec.decode_batch(v, 15, output_len=dec.k, out=(bits, its)),
            }, args.calls, host_clock=True)
            row("decode_batch_f32 (host)", t["f32"], 4 * B * n)
            row("decode_batch_i8 (host)", t["i8"], B * n)
            emit(f"  time i8 / f32 = {t['i8'][0] / t['f32'][0]:.3f}")
            dec.close()
            del d_v, d_f

    if "harq" in args.only:
        sim = lt.Simulator(lt.code_alist(args.code), args.decoder, device=0, pool_size=64, pool_seed=1)
        rm = lt.NrRateMatcher(args.code, device=0)
        qam = lt.NrQam(6, device=0)
        e = (sim.k * 9 // 8 + 3) // 6 * 6
        seq = [(e, rv) for rv in (0, 2, 3, 1)]
        sim.set_rate_match(rm, e, 0, 6)
        sim.set_nr_qam(qam)
        sim.set_harq(rm, seq, 6)
        chunk = sim.get("preferred_batch")
        frames = args.harq_frames or 8 * chunk
        ebn0 = None
        for half in range(40, 0, -1):
            c, tx = sim.run_harq(0.5 * half, 1, 0, 1024, 30)
            if tx[1][0] >= 0.3 * 1024:
                ebn0 = 0.5 * half
                break
        emit(f"harq: {args.code}, {args.decoder}, NR 64QAM, E = {e} x 4 (rv 0, 2, 3, 1), 30 iterations, {ebn0} dB (the highest of a 0.5 dB grid with "
             f"30 % second transmissions under float soft buffers), {frames} frames per call ({frames // chunk} chunks of {chunk}), pooling 1")

        def run(bits):
            sim.set("soft_bits", bits)
            return sim.run_harq(ebn0, 20, 0, frames, 30)

        t = in_turn(stream, {"32": lambda: run(32), "8": lambda: run(8)}, max(args.calls // 2, 3), host_clock=True)
        for bits in (32, 8):
            c, tx = run(bits)
            med, lo, hi = t[str(bits)]
            pools = 3 * 2 * chunk * sim.n * (bits // 8)
            emit(f"  soft_bits {bits:2d}: {med:.3f} s per call (min {lo:.3f}, max {hi:.3f}) = {frames / med:10.0f} frames/s; attempts per transmission "
                 f"{tx[:, 0].tolist()}; frame errors {int(c[2])}; stage pools 3 x 2 x {chunk} x {sim.n} x {bits // 8} bytes = {pools * 1e-6:.1f} MB")
        sim.set("soft_bits", 32)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
