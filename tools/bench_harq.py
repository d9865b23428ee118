#!/usr/bin/env python3
"""Throughput of the HARQ simulator (Simulator.run_harq), on the machine it runs on.

Configuration: --code (default nr5g:1:384, n = 26112, k = 8448), --decoder (default HLMinsumf32), NR 64QAM, rv 0, 2, 3, 1,
every E the multiple of 6 nearest to k * 9 / 8 (rate 8/9 on the first transmission), --max-iter iterations.
Operating point: the highest Eb/N0 of a 0.5 dB grid at which at least 30 % of --scan-frames frames need a second transmission.
Frames per call: a multiple of the simulator's preferred batch that makes a call last at least --seconds.  Every time is a
host clock around a call that ends in a device synchronise; three warm-up calls, then the median of --calls calls.

  * informational: frames/s of run_harq with "pooling" 1 and with "pooling" 0, and the mean rows per flush of each stage;
  * the one condition: run_harq with T = 1 is not slower than run -- same build, point and frames, the two alternating
    in one process -- by more than the spread run itself shows: the largest deviation of its calls from their median.

    python tools/bench_harq.py [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_harq.py --one-call --ebn0 X --frames F
    python tools/bench_harq.py --stats-csv DIR/.../..._kernel_stats.csv [--out FILE]     (the decoder's share of the kernel time)
"""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import ldpc_toolbox_amd as lt  # noqa: E402

# the kernels of a HARQ run that are not the decoder's: generators, rate recovery, collecting and counting
NOT_DECODER = ("awgn_llr", "qam_llr", "nr_rm_", "harq_collect", "harq_count", "count_errors", "straggler_collect")


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return time.perf_counter() - t0, out


def decoder_share(path, emit):
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    other = sum(float(r["TotalDurationNs"]) for r in rows if any(key in r["Name"] for key in NOT_DECODER))
    emit(f"kernel time of one traced process (its sizing and warm-up calls and one timed-size run_harq call): {total * 1e-6:.1f} ms; generators, recovery, collect and count kernels "
         f"{other * 1e-6:.1f} ms; the decoder's kernels {100.0 * (total - other) / total:.1f} %")
    for r in rows:
        if any(key in r["Name"] for key in NOT_DECODER):
            emit(f"  {r['Name'].split('(')[0][:70]:70s} calls {int(r['Calls']):6d} total {float(r['TotalDurationNs']) * 1e-6:9.2f} ms")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--code", default="nr5g:1:384")
    ap.add_argument("--decoder", default="HLMinsumf32")
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--scan-frames", type=int, default=1024)
    ap.add_argument("--ebn0", type=float, default=None, help="the operating point, instead of the scan")
    ap.add_argument("--frames", type=int, default=None, help="frames per call, instead of the --seconds rule")
    ap.add_argument("--one-call", action="store_true", help="one warm-up and one run_harq call with pooling (to be traced)")
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if args.out:
            with open(args.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")

    if args.stats_csv:
        decoder_share(args.stats_csv, emit)
        return finish()
    sim = lt.Simulator(lt.code_alist(args.code), args.decoder, device=0, pool_size=64, pool_seed=1)
    rm = lt.NrRateMatcher(args.code, device=0)
    qam = lt.NrQam(6, device=0)
    e = (sim.k * 9 // 8 + 3) // 6 * 6
    seq = [(e, rv) for rv in (0, 2, 3, 1)]
    sim.set_rate_match(rm, e, 0, 6)
    sim.set_nr_qam(qam)
    sim.set_harq(rm, seq, 6)
    chunk = sim.get("preferred_batch")
    ebn0 = args.ebn0
    if ebn0 is None:
        for half in range(40, 0, -1):
            c, tx = sim.run_harq(0.5 * half, 1, 0, args.scan_frames, args.max_iter)
            if tx[1][0] >= 0.3 * args.scan_frames:
                ebn0 = 0.5 * half
                emit(f"operating point {ebn0} dB: {tx[1][0]} of {args.scan_frames} frames need a second transmission; per_tx {tx.tolist()}")
                break
        else:
            raise SystemExit("no point of the grid has 30 % second transmissions")
    frames = args.frames
    if frames is None:
        timed(lambda: sim.run_harq(ebn0, 1, 0, 2 * chunk, args.max_iter))
        t, _ = timed(lambda: sim.run_harq(ebn0, 1, 0, 2 * chunk, args.max_iter))
        frames = chunk * max(2, int(args.seconds * 1.25 / (t / 2)) + 1)
    if args.one_call:
        sim.run_harq(ebn0, 1, 0, frames, args.max_iter)
        c, tx = sim.run_harq(ebn0, 2, 0, frames, args.max_iter)
        print(f"one run_harq call: {frames} frames at {ebn0} dB, counters {c.tolist()}")
        return
    emit(f"{args.code}, {args.decoder}, NR 64QAM, E = {e} x 4 (rv 0, 2, 3, 1), {args.max_iter} iterations, {ebn0} dB; {frames} frames per call "
         f"({frames // chunk} chunks of {chunk}); 3 warm-up calls, median of {args.calls} (min, max)")
    for pooling in (1, 0):
        sim.set("pooling", pooling)
        for w in range(3):
            sim.run_harq(ebn0, 10 + w, 0, frames, args.max_iter)
        times = []
        for call in range(args.calls):
            t, (c, tx) = timed(lambda: sim.run_harq(ebn0, 20 + call, 0, frames, args.max_iter))
            times.append(t)
        med = statistics.median(times)
        flushes = [(sim.get(f"harq_rows_t{t}"), sim.get(f"harq_flushes_t{t}")) for t in range(1, 4)]
        emit(f"  pooling {pooling}: {med:.3f} s per call (min {min(times):.3f}, max {max(times):.3f}) = {frames / med:10.0f} frames/s; "
             f"attempts per transmission {tx[:, 0].tolist()}; mean rows per flush of stages 1..3: "
             + ", ".join(f"{rows / n:.0f} ({n} flushes)" if n else "- (0 flushes)" for rows, n in flushes))
    sim.set("pooling", 1)
    # the condition: T = 1 against run, alternating
    sim.set_harq(rm, seq[:1], 6)
    for w in range(3):
        sim.run(ebn0, 10 + w, 0, frames, args.max_iter)
        sim.run_harq(ebn0, 10 + w, 0, frames, args.max_iter)
    t_run, t_harq = [], []
    for call in range(max(args.calls, 5)):
        t, c_run = timed(lambda: sim.run(ebn0, 20 + call, 0, frames, args.max_iter))
        t_run.append(t)
        t, (c_harq, _) = timed(lambda: sim.run_harq(ebn0, 20 + call, 0, frames, args.max_iter))
        t_harq.append(t)
        assert c_run.tolist() == c_harq.tolist(), "T = 1 is run"
    m_run, m_harq = statistics.median(t_run), statistics.median(t_harq)
    spread = max(abs(t - m_run) for t in t_run)
    emit(f"T = 1 at the same point, {frames} frames, alternating: run {m_run:.4f} s (min {min(t_run):.4f}, max {max(t_run):.4f}; largest deviation "
         f"from the median {spread:.4f} s), run_harq {m_harq:.4f} s (min {min(t_harq):.4f}, max {max(t_harq):.4f})")
    ok = m_harq <= m_run + spread
    emit(f"condition (run_harq with T = 1 not slower than run by more than run's spread): {'met' if ok else 'NOT met'} "
         f"({m_harq - m_run:+.4f} s against {spread:.4f} s)")
    finish()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
