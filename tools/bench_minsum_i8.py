#!/usr/bin/env python3
"""The 8-bit min-sum names beside Minsumf32 and Minstarapproxi8, measured as bench.py --full measures the headline: frames
resident in HBM, a fixed iteration count at an Eb/N0 where no frame converges, so every rule does the same number of iterations.

  python tools/bench_minsum_i8.py [--parent-lib /path/to/the/previous/libldpc_toolbox.so] [--rounds 5]

Every timing is a child process of its own (one library per process: LDPC_TOOLBOX_LIB), and the variants ALTERNATE round by
round, so that drift of the box lands on all of them.  Per case it prints each variant's codewords/s per round, then
min / median / max, the ratio of the medians to the case's f32 min-sum, and for the 8-bit names the achieved share of the
HBM peak by the byte model of the path: per codeword and iteration 5 E + 3 N bytes (check nodes read a 2-byte posterior and a
message and write a message per edge, variable nodes read a message per edge, a channel byte and write a 2-byte posterior per
variable) against the (4 E + N) * 4 bytes of the f32 path.  With --parent-lib the f32 min-sum and Minstarapproxi8 are also
run from that library (have the untouched kernels moved?).  It ends with the checks the numbers must pass; a failed check
is printed as FAILED and makes the exit status 1."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (code, frames, Eb/N0, f32 rule, 8-bit sum-product rule, plain 8-bit min-sum, corrected forms)
CASES = [("dvbs2:R1_2", 4096, 0.0, "Minsumf32", "Minstarapproxi8", "Minsumi8", ("Minsumi8Norm", "Minsumi8Offset")),
         ("nr5g:1:384", 8192, -2.0, "HLMinsumf32", "HLMinstarapproxi8", "HLMinsumi8", ("HLMinsumi8Norm",))]
MAX_ITER = 50
HBM_PEAK_GBPS = 8000.0


def child(spec, impl, ebn0, batch, steps, warmup):
    import time

    import torch
    sys.path.insert(0, ROOT)
    import ldpc_toolbox_amd as lt
    device = torch.device("cuda", 0)
    alist = lt.code_alist(spec)
    gen = lt.Simulator(alist, "Minsumf32", "", device=0, pool_size=16, pool_seed=1000)
    llrs = torch.empty((batch, gen.n_tx), dtype=torch.float32, device=device)
    gen.generate_into(llrs.data_ptr(), ebn0, 1000, 0, batch)
    gen.close()
    dec = lt.LdpcDecoder(alist, impl, device=0)
    bits = torch.zeros((batch, dec.k), dtype=torch.uint8, device=device)
    its = torch.zeros(batch, dtype=torch.int32, device=device)
    stream = torch.cuda.Stream(device)
    torch.cuda.synchronize(device)

    def step():
        dec.decode_batch_device(llrs.data_ptr(), False, batch, MAX_ITER, bits.data_ptr(), dec.k, its.data_ptr(), 0, stream.cuda_stream)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    print(json.dumps({"cw_s": batch * steps / dt, "all_failed": bool((its.cpu().numpy() == -1).all()), "n": dec.n, "edges": dec.edges}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child", nargs=4, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], float(a.child[2]), int(a.child[3]), a.steps, a.warmup)
    failed = []

    def check(ok, text):
        print(("  ok      " if ok else "  FAILED  ") + text, flush=True)
        if not ok:
            failed.append(text)
    for spec, batch, ebn0, f32, star, plain, corrected in CASES:
        impls = (f32, star, plain) + corrected
        variants = ([("parent " + i, a.parent_lib, i) for i in (f32, star)] if a.parent_lib else []) + [(i, None, i) for i in impls]
        runs = {v[0]: [] for v in variants}
        n = edges = 0
        for r in range(a.rounds):
            for label, lib, impl in variants:
                env = dict(os.environ)
                if lib:
                    env["LDPC_TOOLBOX_LIB"] = lib
                else:
                    env.pop("LDPC_TOOLBOX_LIB", None)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup),
                                      "--child", spec, impl, str(ebn0), str(batch)], env=env, capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    sys.exit(f"{label}: child failed ({out.returncode})\n{out.stderr[-2000:]}")
                res = json.loads(out.stdout.strip().splitlines()[-1])
                assert res["all_failed"], f"{spec} {impl}: not a fixed-work point"
                n, edges = res["n"], res["edges"]
                runs[label].append(res["cw_s"])
                print(f"  round {r} {spec:12s} {label:28s} {res['cw_s']:10.0f} cw/s", flush=True)
        med = {k: statistics.median(v) for k, v in runs.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in runs.items()}
        bytes_i8, bytes_f32 = 5 * edges + 3 * n, (4 * edges + n) * 4
        print(f"{spec}, {batch} frames resident in HBM, {MAX_ITER} iterations, Eb/N0 {ebn0} dB, {a.rounds} alternating rounds of {a.steps} steps;")
        print(f"  N = {n}, E = {edges}: {bytes_i8} B per codeword-iteration on the 8-bit path (5 E + 3 N), {bytes_f32} B in f32 ((4 E + N) * 4): "
              f"ceiling ratio {bytes_f32 / bytes_i8:.2f}")
        for label, v in runs.items():
            model = bytes_f32 if label.endswith("f32") else bytes_i8
            print(f"  {label:28s} min {min(v):9.0f}  median {med[label]:9.0f}  max {max(v):9.0f} cw/s   median / {f32} {med[label] / med[f32]:6.3f}   "
                  f"spread {spread[label] * 100:5.2f} %   whole-job byte model / HBM peak {med[label] * MAX_ITER * model / 1e9 / HBM_PEAK_GBPS:5.3f}", flush=True)
        check(med[plain] >= med[star], f"{plain} median {med[plain]:.0f} >= {star} median {med[star]:.0f} cw/s ({med[plain] / med[star]:.2f} x)")
        for c in corrected:
            print(f"  cost of {c} over {plain}: {(1 - med[c] / med[plain]) * 100:+.2f} % (spreads {spread[c] * 100:.2f} % / {spread[plain] * 100:.2f} %)")
        if a.parent_lib:
            for i in (f32, star):
                tol = max(spread[i], spread["parent " + i], 0.01)
                check(abs(med[i] / med["parent " + i] - 1) <= tol,
                      f"{i}: this build / parent = {med[i] / med['parent ' + i]:.4f}, within the run-to-run spread ({tol * 100:.2f} %)")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
