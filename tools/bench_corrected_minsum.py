#!/usr/bin/env python3
"""What the normalized / offset min-sum correction costs, measured as bench.py --full measures the headline: frames resident
in HBM, a fixed iteration count at an Eb/N0 where no frame converges, so every variant does the same work.

  python tools/bench_corrected_minsum.py [--parent-lib /path/to/the/previous/libldpc_toolbox.so] [--rounds 5]

Every timing is a child process of its own (one library per process: LDPC_TOOLBOX_LIB), and the variants ALTERNATE round by
round, so that drift of the box lands on all of them.  Per case it prints each variant's codewords/s per round, then
min / median / max and the ratio of the medians to plain min-sum of this build.  With --parent-lib the first variant is
plain min-sum from that library (has plain min-sum moved?)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("dvbs2:R1_2", "", 0.0, ("Minsumf32", "NormMinsumf32", "OffsetMinsumf32")),
         ("nr5g:1:384", "HL", -2.0, ("HLMinsumf32", "HLNormMinsumf32", "HLOffsetMinsumf32"))]
BATCH, MAX_ITER = 4096, 50


def child(spec, impl, ebn0, steps, warmup):
    import time

    import torch
    sys.path.insert(0, ROOT)
    import ldpc_toolbox_amd as lt
    device = torch.device("cuda", 0)
    alist = lt.code_alist(spec)
    gen = lt.Simulator(alist, "Minsumf32", "", device=0, pool_size=16, pool_seed=1000)
    llrs = torch.empty((BATCH, gen.n_tx), dtype=torch.float32, device=device)
    gen.generate_into(llrs.data_ptr(), ebn0, 1000, 0, BATCH)
    gen.close()
    dec = lt.LdpcDecoder(alist, impl, device=0)
    bits = torch.zeros((BATCH, dec.k), dtype=torch.uint8, device=device)
    its = torch.zeros(BATCH, dtype=torch.int32, device=device)
    stream = torch.cuda.Stream(device)
    torch.cuda.synchronize(device)

    def step():
        dec.decode_batch_device(llrs.data_ptr(), False, BATCH, MAX_ITER, bits.data_ptr(), dec.k, its.data_ptr(), 0, stream.cuda_stream)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    print(json.dumps({"cw_s": BATCH * steps / dt, "all_failed": bool((its.cpu().numpy() == -1).all())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], float(a.child[2]), a.steps, a.warmup)
    for spec, _, ebn0, impls in CASES:
        variants = ([("parent " + impls[0], a.parent_lib, impls[0])] if a.parent_lib else []) + [(i, None, i) for i in impls]
        runs = {v[0]: [] for v in variants}
        for r in range(a.rounds):
            for label, lib, impl in variants:
                env = dict(os.environ)
                if lib:
                    env["LDPC_TOOLBOX_LIB"] = lib
                else:
                    env.pop("LDPC_TOOLBOX_LIB", None)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup),
                                      "--child", spec, impl, str(ebn0)], env=env, capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    sys.exit(f"{label}: child failed ({out.returncode})\n{out.stderr[-2000:]}")
                res = json.loads(out.stdout.strip().splitlines()[-1])
                assert res["all_failed"], f"{spec} {impl}: not a fixed-work point"
                runs[label].append(res["cw_s"])
                print(f"  round {r} {spec:12s} {label:28s} {res['cw_s']:10.0f} cw/s", flush=True)
        base = statistics.median(runs[impls[0]])
        print(f"{spec}, {BATCH} frames resident in HBM, {MAX_ITER} iterations, Eb/N0 {ebn0} dB, {a.rounds} alternating rounds of {a.steps} steps:")
        for label, v in runs.items():
            print(f"  {label:28s} min {min(v):9.0f}  median {statistics.median(v):9.0f}  max {max(v):9.0f} cw/s   "
                  f"median / plain {statistics.median(v) / base:6.4f}   spread {(max(v) - min(v)) / statistics.median(v) * 100:4.2f} %", flush=True)


if __name__ == "__main__":
    main()
