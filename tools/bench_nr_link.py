#!/usr/bin/env python3
"""Cost of the NR link handle (include/ldpc_toolbox.h, PART 11) beside the composition of the stage handles that defines it,
on the machine it runs on.  Everything is device-resident, on one stream of the caller's, hipEvent-timed, 3 calls warm, median
of --calls calls with the min-max spread; the two sides of a comparison run call by call in turn, in the same run.

Workload: --spec (default nr5g-link:1:16896:33792:6 -- three code blocks of n = 19584 per transport block, two lengths,
64QAM, rate 1/2), --batch transport blocks per call (default 1024), Minsumf32, 30 iterations.
  (a) first reception   `receive_device(combine=False)` at --ebn0 against the six receive calls of the chain: demodulate,
                        split, recover at e_lo, recover at e_hi, decode_batch, desegment (and the transmit side: one call
                        against six);
  (b) recover alone     `recover_device`, the fused de-concatenation and rate recovery kernel, against split + two recover calls;
  (c) retransmission    `receive_device(combine=True)` where about one block in ten is not done -- the first reception of one
                        transport block in ten was noise alone -- against the same call where the first reception of every
                        transport block was noise alone, so every block is decoded.  The first receptions are not timed.

With --soft-bits 8 (include/ldpc_toolbox.h, PART 12; --implementation one of the 8-bit names) the two sides are the 8-bit
handle and the float handle with the same implementation, call by call in turn:
  (a) first reception   `receive_device(combine=False)` of the 8-bit handle against the float handle's;
  (b) recover alone     `recover_i8_device` against `recover_device` on the same LLRs, as bytes and as floats;
  (c) retransmission    the pair above, on the 8-bit handle.

    python tools/bench_nr_link.py [--spec S] [--batch 1024] [--ebn0 12] [--calls 20] [--out profiles/nr_link_gpu.txt]
                                  [--implementation Minsumf32] [--soft-bits 32]
"""
import argparse
import os
import statistics
import sys

import torch  # before the library: one HIP runtime per process (tests/conftest.py)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import ldpc_toolbox_amd as lt  # noqa: E402
from ldpc_toolbox_amd import simulation as sim  # noqa: E402

MAX_ITER, FILLER = 30, 20.0


def timed_in_turn(stream, calls_by_name, calls, before=None):
    """every callable 3 times warm, then `calls` rounds of one call each in turn -> {name: (median, min, max)} seconds;
    before[name]: run (and waited for) ahead of each call of that name, untimed"""
    times = {name: [] for name in calls_by_name}
    for i in range(3 + calls):
        for name, call in calls_by_name.items():
            if before and name in before:
                before[name]()
                stream.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            if i >= 3:
                times[name].append(a.elapsed_time(b) * 1e-3)
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def report(emit, t, B):
    for name, (med, lo, hi) in t.items():
        emit(f"  {name:<26} {med * 1e3:9.3f} ms (min {lo * 1e3:.3f} .. max {hi * 1e3:.3f})  {B / med * 1e-3:9.1f} k transport blocks/s")


def main_i8(args, emit):
    """the 8-bit handle beside the float handle with the same 8-bit implementation"""
    B = args.batch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    links = {"i8": lt.NrLink(args.spec, args.implementation, B, device=0, soft_bits=8), "f32": lt.NrLink(args.spec, args.implementation, B, device=0)}
    for link in links.values():
        link.set_filler_llr(FILLER)
    link = links["i8"]
    a, c, k, n, g, qm, S = link.a, link.c, link.k, link.n, link.g, link.qm, link.symbols
    e_lo, e_hi, c_lo = link.block_lengths
    qam = lt.NrQam(qm, device=0)
    sigma = sim.noise_sigma(a / g, args.ebn0, qm)
    emit(f"{args.spec}: C = {c}, K = {k}, n = {n}, G = {g} ({c_lo} blocks of {e_lo}, {c - c_lo} of {e_hi}), {S} symbols of {qm} bits; "
         f"{B} transport blocks = {c * B} code blocks per call; {args.implementation}, soft_bits 8 against 32, {MAX_ITER} iterations, "
         f"Eb/N0 {args.ebn0} dB; median of {args.calls} calls (min .. max)")
    emit(f"  soft_bytes of the {B} slots: {links['i8'].soft_bytes} with soft_bits 8, {links['f32'].soft_bytes} with 32")
    u8 = dict(dtype=torch.uint8, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    payload = torch.randint(0, 2, (B, a), generator=gen, **u8)
    sym = {rv: torch.zeros((B, S, 2), **f32) for rv in (0, 2)}
    llrs, llrs_i8 = torch.zeros((B, g), **f32), torch.zeros((B, g), dtype=torch.int8, device=dev)
    out = {name: (torch.zeros((B, a), **u8), torch.zeros(B, **u8), torch.zeros((B, c), **u8), torch.zeros((B, c), dtype=torch.int32, device=dev))
           for name in links}
    torch.cuda.synchronize()

    def receive(name, rx, rv, combine):
        p, t_ok, c_ok, it = out[name]
        links[name].receive_device(rx.data_ptr(), p.data_ptr(), t_ok.data_ptr(), c_ok.data_ptr(), it.data_ptr(), B, sigma, rv=rv, combine=combine,
                                   max_iterations=MAX_ITER, stream=st)

    for rv in (0, 2):
        link.transmit_device(payload.data_ptr(), sym[rv].data_ptr(), B, rv=rv, stream=st)
    stream.synchronize()
    rx = {rv: sym[rv] + sigma * torch.randn(sym[rv].shape, generator=gen, **f32) for rv in (0, 2)}
    junk = torch.randn(sym[0].shape, generator=gen, **f32)
    tenth = rx[0].clone()
    tenth[::10] = junk[::10]
    torch.cuda.synchronize()
    t = timed_in_turn(stream, {"receive, soft_bits 8": lambda: receive("i8", rx[0], 0, False), "receive, soft_bits 32": lambda: receive("f32", rx[0], 0, False)},
                      args.calls)
    stream.synchronize()
    for name in links:
        emit(f"  first reception, {name}: {int(out[name][1].sum())} of {B} transport blocks pass, {int(out[name][2].sum())} of {c * B} code blocks")
    qam.demodulate_device(rx[0].data_ptr(), llrs.data_ptr(), False, B, S, sigma, False, -1, st)
    qam.demap_i8_device(rx[0].data_ptr(), llrs_i8.data_ptr(), B, S, sigma, False, -1, st)
    stream.synchronize()
    t.update(timed_in_turn(stream, {"recover_i8_device": lambda: links["i8"].recover_i8_device(llrs_i8.data_ptr(), B, rv=0, combine=False, stream=st),
                                    "recover_device (f32)": lambda: links["f32"].recover_device(llrs.data_ptr(), B, rv=0, combine=False, stream=st)},
                           args.calls))
    stream.synchronize()
    counts = {}

    def retransmission(name):
        receive("i8", rx[2], 2, True)
        counts[name] = (link.decoded_rows, link.skipped_rows)

    t.update(timed_in_turn(stream, {"retransmission, 1 in 10": lambda: retransmission("tenth"), "retransmission, all": lambda: retransmission("all")},
                           args.calls, before={"retransmission, 1 in 10": lambda: receive("i8", tenth, 0, False),
                                               "retransmission, all": lambda: receive("i8", junk, 0, False)}))
    stream.synchronize()
    emit(f"  retransmission, 1 in 10: {counts['tenth'][0]} code blocks decoded, {counts['tenth'][1]} skipped;  all: {counts['all'][0]} decoded, "
         f"{counts['all'][1]} skipped")
    report(emit, t, B)

    def ratio(x, y):
        (m, lo, hi), (m2, lo2, hi2) = t[x], t[y]
        return f"{x} / {y} = {m / m2:.3f} (min/max {lo / hi2:.3f} .. max/min {hi / lo2:.3f})"

    emit("  (a) " + ratio("receive, soft_bits 8", "receive, soft_bits 32"))
    emit("  (b) " + ratio("recover_i8_device", "recover_device (f32)"))
    emit("  (c) " + ratio("retransmission, 1 in 10", "retransmission, all"))
    behind = t["receive, soft_bits 8"][0] - t["receive, soft_bits 32"][0]
    spread = t["receive, soft_bits 32"][2] - t["receive, soft_bits 32"][1]
    emit(f"  (a) the 8-bit first reception is {behind * 1e3:+.3f} ms against the float handle's, whose own min-max spread is {spread * 1e3:.3f} ms")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--spec", default="nr5g-link:1:16896:33792:6")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--ebn0", type=float, default=12.0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    ap.add_argument("--implementation", default="Minsumf32")
    ap.add_argument("--soft-bits", type=int, choices=(32, 8), default=32)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if args.soft_bits == 8:
        main_i8(args, emit)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")
        return

    B = args.batch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    link = lt.NrLink(args.spec, args.implementation, B, device=0)
    link.set_filler_llr(FILLER)
    a, c, k, n, g, qm, S = link.a, link.c, link.k, link.n, link.g, link.qm, link.symbols
    e_lo, e_hi, c_lo = link.block_lengths
    tb = lt.NrTransportBlock(f"nr5g-tb:{link.base_graph}:{a}", device=0)
    alist = lt.code_alist(tb.code_spec)
    enc, dec = lt.Encoder(alist), lt.LdpcDecoder(alist, args.implementation, device=0)
    rm, qam = lt.NrRateMatcher(tb.rate_match_spec, device=0), lt.NrQam(qm, device=0)
    sigma = sim.noise_sigma(a / g, args.ebn0, qm)
    emit(f"{args.spec}: C = {c}, K = {k}, n = {n}, G = {g} ({c_lo} blocks of {e_lo}, {c - c_lo} of {e_hi}), {S} symbols of {qm} bits; "
         f"{B} transport blocks = {c * B} code blocks per call; {args.implementation}, {MAX_ITER} iterations, Eb/N0 {args.ebn0} dB; "
         f"median of {args.calls} calls (min .. max)")
    u8 = dict(dtype=torch.uint8, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    payload = torch.randint(0, 2, (B, a), generator=gen, **u8)
    sym = {rv: torch.zeros((B, S, 2), **f32) for rv in (0, 2)}
    # the chain's buffers
    rows, cws, packed, tx = torch.zeros((c * B, k), **u8), torch.zeros((c * B, n), **u8), torch.zeros(B * g, **u8), torch.zeros((B, g), **u8)
    sym_chain = torch.zeros((B, S, 2), **f32)
    llrs, split, soft = torch.zeros((B, g), **f32), torch.zeros(B * g, **f32), torch.zeros((c * B, n), **f32)
    bits, its = torch.zeros((c * B, k), **u8), torch.zeros(c * B, dtype=torch.int32, device=dev)
    out = {name: (torch.zeros((B, a), **u8), torch.zeros(B, **u8), torch.zeros((B, c), **u8), torch.zeros((B, c), dtype=torch.int32, device=dev))
           for name in ("link", "chain")}
    lo_rows, hi_rows = c_lo * B, (c - c_lo) * B
    torch.cuda.synchronize()

    def chain_transmit():
        tb.segment_device(payload.data_ptr(), rows.data_ptr(), B, stream=st)
        enc.encode_batch_device(rows.data_ptr(), cws.data_ptr(), c * B, st)
        rm.match_device(cws.data_ptr(), packed.data_ptr(), lo_rows, e_lo, 0, qm, stream=st)
        rm.match_device(cws.data_ptr() + lo_rows * n, packed.data_ptr() + lo_rows * e_lo, hi_rows, e_hi, 0, qm, stream=st)
        tb.concatenate_device(packed.data_ptr(), tx.data_ptr(), B, g, link.q, stream=st)
        qam.modulate_device(tx.data_ptr(), sym_chain.data_ptr(), False, B, g, -1, st)

    def chain_split_recover(rx):
        tb.split_device(rx.data_ptr(), split.data_ptr(), False, B, g, link.q, stream=st)
        rm.recover_device(split.data_ptr(), soft.data_ptr(), False, lo_rows, e_lo, 0, qm, filler_llr=FILLER, stream=st)
        if hi_rows:
            rm.recover_device(split.data_ptr() + 4 * lo_rows * e_lo, soft.data_ptr() + 4 * lo_rows * n, False, hi_rows, e_hi, 0, qm,
                              filler_llr=FILLER, stream=st)

    def chain_receive(rx):
        p, t_ok, c_ok, _ = out["chain"]
        qam.demodulate_device(rx.data_ptr(), llrs.data_ptr(), False, B, S, sigma, False, -1, st)
        chain_split_recover(llrs)
        dec.decode_batch_device(soft.data_ptr(), False, c * B, MAX_ITER, bits.data_ptr(), k, its.data_ptr(), 0, st)
        tb.desegment_device(bits.data_ptr(), p.data_ptr(), t_ok.data_ptr(), c_ok.data_ptr(), B, stream=st)

    def link_receive(rx, rv, combine):
        p, t_ok, c_ok, it = out["link"]
        link.receive_device(rx.data_ptr(), p.data_ptr(), t_ok.data_ptr(), c_ok.data_ptr(), it.data_ptr(), B, sigma, rv=rv, combine=combine,
                            max_iterations=MAX_ITER, stream=st)

    # the transmissions, and what is received: the symbols behind the AWGN channel; noise alone for (c)
    for rv in (0, 2):
        link.transmit_device(payload.data_ptr(), sym[rv].data_ptr(), B, rv=rv, stream=st)
    stream.synchronize()
    rx = {rv: sym[rv] + sigma * torch.randn(sym[rv].shape, generator=gen, **f32) for rv in (0, 2)}
    junk = torch.randn(sym[0].shape, generator=gen, **f32)
    tenth = rx[0].clone()
    tenth[::10] = junk[::10]
    torch.cuda.synchronize()

    t = timed_in_turn(stream, {"link transmit": lambda: link.transmit_device(payload.data_ptr(), sym[0].data_ptr(), B, rv=0, stream=st),
                               "chain transmit": chain_transmit}, args.calls)
    stream.synchronize()
    if not torch.equal(sym[0], sym_chain):
        raise SystemExit("the link's symbols are not the chain's")
    t.update(timed_in_turn(stream, {"link receive": lambda: link_receive(rx[0], 0, False), "chain receive": lambda: chain_receive(rx[0])}, args.calls))
    stream.synchronize()
    for x, y in zip(out["link"][:3], out["chain"]):
        if not torch.equal(x, y):
            raise SystemExit("the link's first reception is not the chain's")
    passed = int(out["link"][1].sum())
    emit(f"  first reception: {passed} of {B} transport blocks pass, {int(out['link'][2].sum())} of {c * B} code blocks")
    torch.cuda.synchronize()
    qam.demodulate_device(rx[0].data_ptr(), llrs.data_ptr(), False, B, S, sigma, False, -1, st)
    stream.synchronize()
    t.update(timed_in_turn(stream, {"fused recover": lambda: link.recover_device(llrs.data_ptr(), B, rv=0, combine=False, stream=st),
                                    "split + 2 recover": lambda: chain_split_recover(llrs)}, args.calls))
    stream.synchronize()
    if not torch.equal(torch.from_numpy(link.slot_state()[0]).to(dev).view(torch.int32), soft.view(torch.int32)):
        raise SystemExit("the fused kernel's soft rows are not those of split and recover")
    counts = {}

    def retransmission(name):
        link_receive(rx[2], 2, True)
        counts[name] = (link.decoded_rows, link.skipped_rows)

    t.update(timed_in_turn(stream, {"retransmission, 1 in 10": lambda: retransmission("tenth"), "retransmission, all": lambda: retransmission("all")},
                           args.calls, before={"retransmission, 1 in 10": lambda: link_receive(tenth, 0, False),
                                               "retransmission, all": lambda: link_receive(junk, 0, False)}))
    stream.synchronize()
    emit(f"  retransmission, 1 in 10: {counts['tenth'][0]} code blocks decoded, {counts['tenth'][1]} skipped;  all: {counts['all'][0]} decoded, "
         f"{counts['all'][1]} skipped")
    report(emit, t, B)

    def ratio(x, y):
        return f"{x} / {y} = {t[x][0] / t[y][0]:.3f}"

    emit("  (a) " + ratio("link receive", "chain receive") + ";  " + ratio("link transmit", "chain transmit"))
    emit("  (b) " + ratio("fused recover", "split + 2 recover"))
    emit("  (c) " + ratio("retransmission, 1 in 10", "retransmission, all"))
    behind = t["fused recover"][0] - t["split + 2 recover"][0]
    spread = t["split + 2 recover"][2] - t["split + 2 recover"][1]
    emit(f"  (b) the fused kernel is {behind * 1e3:+.3f} ms against the composition, whose own min-max spread is {spread * 1e3:.3f} ms: "
         + ("it earns its place" if behind <= spread else "slower by more than that spread"))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
