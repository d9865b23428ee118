"""CPU: the host half of the library (alist reader, code constructions, encoders, parsers) built
with AddressSanitizer + UndefinedBehaviorSanitizer and driven over valid and malformed inputs.
(GPU sanitizers are not available on the pool; the device code is covered by the parity tests.)"""
import os
import subprocess

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "ldpc_toolbox_amd", "csrc")


def test_host_code_is_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "host_sanitizer_driver")
    srcs = [os.path.join(ROOT, "tests", "host_sanitizer_driver.cpp")] + \
           [os.path.join(CSRC, f) for f in ("sparse.cpp", "codes.cpp", "encoder.cpp", "implementation.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe] + srcs, check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "host sanitizer driver: ok" in r.stdout


def test_oracle_is_clean_under_asan_ubsan(tmp_path):
    """the checker itself: every implementation name on a small 5G NR graph (rows of degree 3..19)"""
    import ldpc_toolbox_amd as lt
    exe = str(tmp_path / "oracle_sanitizer_driver")
    subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-pthread", "-o", exe,
                    os.path.join(ROOT, "tests", "oracle_sanitizer_driver.c"), os.path.join(ROOT, "oracle", "ldpc_oracle.c"),
                    "-lm"], check=True, capture_output=True)
    alist = tmp_path / "h.alist"
    alist.write_text(lt.code_alist("nr5g:1:4"))
    r = subprocess.run([exe, str(alist)] + list(lt.ALL_IMPLEMENTATIONS), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "oracle sanitizer driver: ok" in r.stdout


def test_layered_level_tables_under_asan_ubsan(tmp_path):
    """dependency levels and the row records of the register-resident level kernels (csrc/slice_tasks.h): rows of one
    level share no variable, levels follow the row order, and every record lists its row's first edge, degree and
    variables -- for codes with short rows only, with rows of 19 (5G NR BG1), with rows too long for a record (DVB-S2
    short 8/9), and a staircase code"""
    import ldpc_toolbox_amd as lt
    exe = str(tmp_path / "slice_tasks_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "slice_tasks_driver.cpp"),
                    os.path.join(CSRC, "sparse.cpp")], check=True, capture_output=True)
    files = []
    for spec in ("nr5g:1:8", "nr5g:2:24", "ar4ja:1/2:1024", "dvbs2:R8_9short", "nr5g:1:384"):
        f = tmp_path / (spec.replace(":", "_").replace("/", "_") + ".alist")
        f.write_text(lt.code_alist(spec))
        files.append(str(f))
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "slice tasks driver: ok" in r.stdout


def test_graph_tables_under_asan_ubsan(tmp_path):
    """the decoder's graph tables as pure functions of the CSR form (csrc/graph_tables.h): the L-free / keep split, the
    peer words of the row records, the sliced-ELLPACK tables and the wavefront lane packing of the small-batch paths, the
    depuncture map -- on a code whose degree-2 variables join distant rows (AR4JA: no row records by default), a
    staircase code (neighbouring rows), rows too long for a packed record (DVB-S2 short 8/9), two 5G NR graphs, and the
    driver's own matrix with an empty row, a degree-1 variable and a variable in no row"""
    import ldpc_toolbox_amd as lt
    exe = str(tmp_path / "graph_tables_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "graph_tables_driver.cpp"),
                    os.path.join(CSRC, "sparse.cpp")], check=True, capture_output=True)
    args = []
    for spec, peers in (("ar4ja:1/2:1024", "far:"), ("dvbs2:R1_2short", "near:"), ("dvbs2:R8_9short", ""), ("nr5g:1:8", ""),
                        ("nr5g:2:24", "")):
        f = tmp_path / (spec.replace(":", "_").replace("/", "_") + ".alist")
        f.write_text(lt.code_alist(spec))
        args.append(peers + str(f))
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "hand-made" in r.stdout and "graph tables driver: ok" in r.stdout


_TSAN_BUILD = {}


def _tsan_driver(tmp_path_factory):
    """tests/tsan_driver: the library's host code + tests/hip_stub under ThreadSanitizer, built once for the module"""
    if "exe" not in _TSAN_BUILD:
        out = str(tmp_path_factory.mktemp("tsan"))
        b = subprocess.run([os.path.join(ROOT, "tests", "hip_stub", "build.sh"), out], capture_output=True, text=True, timeout=900)
        assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-4000:]
        _TSAN_BUILD["exe"] = os.path.join(out, "tsan_driver")
    return _TSAN_BUILD["exe"]


def test_host_threads_are_clean_under_tsan(tmp_path_factory):
    """SURVEY section 5 "Race detection": the library's real host code (c_api.cpp, device_decoder.hip, simulator.hip
    compiled host-only) under ThreadSanitizer against tests/hip_stub -- streams are worker threads, events are counters,
    kernels publish the progress word.  Scenarios: every group runs all its iterations; the device "finishes" at
    iteration 3 / 1 (the enqueuing threads' early exits and pacing); a HIP call fails somewhere in the middle (the
    error returns of decode_host / decode_device with lane threads alive).  Round 4 found and fixed two unsynchronised
    writes this way (skew_record_ and another member written by both lanes' threads)."""
    exe = _tsan_driver(tmp_path_factory)
    scenarios = [({}, "0"), ({"HIP_STUB_DONE_AT": "3"}, "0"), ({"HIP_STUB_DONE_AT": "1"}, "0")]
    scenarios += [({"HIP_STUB_FAIL": f}, "1") for f in ("hipEventRecord:3", "hipEventRecord:40", "hipStreamWaitEvent:2",
                                                        "hipStreamWaitEvent:25", "hipLaunchKernel:7000", "hipMemcpyAsync:9",
                                                        "hipMalloc:12", "hipStreamSynchronize:6")]
    # Failures where something is being acquired, by the first handle's allocation trace (HIP_STUB_TRACE: mallocs 1-7 and
    # memcpys 1-7 are create()'s uploads, malloc 8 the two lanes' workspace slab, pinned allocations 1-2 the progress words
    # -- tolerated by design, never aimed at -- and 3 the first staging chunk; events 1-3 and streams 1-2 are create()'s,
    # events 4-15 and streams 3-4 the host pipe's): an upload's copy, an upload's allocation, the slab, a staging chunk,
    # one of the pipe's events, the pipe's first stream.  The driver ends every scenario with the stub's count of live
    # allocations, events and streams: zero, or it fails.
    scenarios += [({"HIP_STUB_FAIL": f}, "1") for f in ("hipMemcpy:3", "hipMalloc:6", "hipMalloc:8", "hipHostMalloc:3",
                                                        "hipEventCreateWithFlags:9", "hipStreamCreateWithFlags:3")]
    # ... and in the small-batch path's first call, which the driver makes after all the others (allocation 153 of the run
    # is the fourth sliced table of latency.hip.h's handle: `grep -n ^malloc` in the trace of a run without failures): the
    # call after the failed one uploads the tables again.  The raw pointers this code held before the owning types were
    # overwritten there, and three allocations stayed live at exit (profiles/owned_resources.txt).
    scenarios.append(({"HIP_STUB_FAIL": "hipMalloc:153"}, "1"))
    for extra, expect_error in scenarios:
        env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66", **extra)
        r = subprocess.run([exe, expect_error], capture_output=True, text=True, env=env, timeout=600)
        text = r.stdout + r.stderr
        assert "ThreadSanitizer" not in text, (extra, text[-6000:])
        assert r.returncode == 0 and "tsan driver: ok" in r.stdout, (extra, text[-3000:])


def test_stage_handles_under_tsan(tmp_path_factory, tmp_path):
    """The six stage handles beside the decoder (rate matcher, transport block, NR modulation, BCH, demodulator, batched
    encoder; csrc/device_stage.h holds what they share) and the simulator's NR generators, driven through the C ABI by
    `tsan_driver stages`: host entry and _device entry of every call, single-stage shapes.  Plainly: no report, nothing
    live at the end.  Then with one HIP call failing inside a stage-handle call -- the ordinals are read from the plain
    run's call trace (HIP_STUB_TRACE_CALLS), by the driver's note of the call they fall into:
      hipMalloc             the Gold sequence buffer of the first scrambled 16QAM call (DeviceNrQam::sequence);
      hipMemcpyAsync        the first strided copy to the device of a two-block transport block's desegment (copy_rows);
      hipStreamSynchronize  the wait that closes the stage of a BCH decode_host (the staging loop of device_stage.h);
      hipEventRecord        the record behind a 64QAM launch that read the cached sequence (DeviceNrQam::end), the second
                            record of that call after begin()'s.
    Each must surface as LDPC_TOOLBOX_ERR_DEVICE from that call alone, with the failed expression as the message, the
    calls after it succeeding and nothing live at the end."""
    exe = _tsan_driver(tmp_path_factory)
    trace = tmp_path / "stages.txt"
    base = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66")
    nothing_live = "live after the last handle: device 0 pinned 0 events 0 streams 0"

    r = subprocess.run([exe, "stages"], capture_output=True, text=True, timeout=600,
                       env=dict(base, HIP_STUB_TRACE=str(trace), HIP_STUB_TRACE_CALLS="1"))
    text = r.stdout + r.stderr
    assert "ThreadSanitizer" not in text, text[-6000:]
    assert r.returncode == 0 and "stages: ok" in r.stdout and nothing_live in r.stdout, text[-3000:]
    lines = trace.read_text().splitlines()

    def ordinal(note, prefix, nth=1):
        """of all `prefix` lines of the trace, the 1-based position of the nth one within the call `note`"""
        at = lines.index("# " + note)
        end = next(i for i in range(at + 1, len(lines)) if lines[i].startswith("# "))
        inside = [i for i in range(at + 1, end) if lines[i].startswith(prefix)]
        return sum(1 for line in lines[:inside[nth - 1] + 1] if line.startswith(prefix))

    failures = [
        ("hipMalloc", ordinal("nr_qam QM=4 mod f32 host c_init=7", "malloc "),
         "nr_qam QM=4 mod f32 host c_init=7", "d_gold_.ensure("),
        ("hipMemcpyAsync", ordinal("nr_tb C=2 desegment host cb_ok", "memcpyasync "),
         "nr_tb C=2 desegment host cb_ok", "hipMemcpyAsync(dst + dev_at, src + host_at"),
        ("hipStreamSynchronize", ordinal("bch decode host, errors", "streamsync "),
         "bch decode host, errors", "hipStreamSynchronize(stream_)"),
        ("hipEventRecord", ordinal("nr_qam QM=6 demod f64 device max-log c_init=7", "eventrecord ", 2),
         "nr_qam QM=6 demod f64 device max-log c_init=7", "hipEventRecord(ev_gold_read_, s)"),
    ]
    for function, n, note, expression in failures:
        r = subprocess.run([exe, "stages", "1"], capture_output=True, text=True, timeout=600,
                           env=dict(base, HIP_STUB_FAIL="%s:%d" % (function, n)))
        text = r.stdout + r.stderr
        assert "ThreadSanitizer" not in text, (function, n, text[-6000:])
        assert r.returncode == 0 and "stages: ok" in r.stdout and nothing_live in r.stdout, (function, n, text[-3000:])
        failed = [line for line in r.stdout.splitlines() if line.startswith("stages: ") and ": rc " in line]
        assert len(failed) == 1 and failed[0].startswith("stages: %s: rc -2: %s" % (note, expression)), (function, n, failed)


def test_launch_trace_keeps_the_arithmetic_and_the_pack_width(tmp_path_factory, tmp_path):
    """Which kernel a launch names decides the arithmetic (normalized / offset min-sum: the x_kernel<..., MinsumCorr<T>>
    instantiations) and must respect the pack width of the type (f64: at most two codewords per lane).  `tsan_driver
    trace` walks every such choice of launch.hip.h, run_group.hip.h and run_group_i8.hip on the CPU -- the stub writes
    down stream, geometry and kernel name of every launch -- with "poll" 0 and "lane_threads" 0, so that the host's
    enqueue order depends on the inputs alone."""
    import re
    exe = _tsan_driver(tmp_path_factory)
    trace = tmp_path / "launches.txt"
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66", HIP_STUB_TRACE=str(trace))
    r = subprocess.run([exe, "trace"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "trace: ok" in r.stdout and "ThreadSanitizer" not in r.stdout + r.stderr, (r.stdout + r.stderr)[-4000:]
    rules = dict(re.findall(r"(kRuleMinsum(?:Corr)?) = (\d+)", open(os.path.join(CSRC, "kernels_common.hip.h")).read()))
    minsum_rules = {rules["kRuleMinsum"], rules["kRuleMinsumCorr"]}
    sections = []  # (implementation, [kernel names])
    for line in trace.read_text().splitlines():
        if line.startswith("# "):
            sections.append((line.split()[1], []))
        elif not line.startswith(("malloc ", "hostmalloc ", "h2d ")):  # (allocations and uploads: not launches)
            stream, name = re.fullmatch(r"(\d+) grid \d+ \d+ \d+ block \d+ \d+ \d+ lds \d+ (.*)", line).groups()
            sections[-1][1].append(name)
    assert all(names for _, names in sections)

    def arithmetic_is_minsum(name):
        staged = re.search(r"(?:cn_staged|hl_level|hl_level_reg)_kernel<(\d+),", name)
        return "minsum" in name or (staged is not None and staged.group(1) in minsum_rules)

    corrected = [names for impl, names in sections if re.fullmatch(r"(HL)?(Norm|Offset)Minsumf(32|64)", impl)]
    plain = [names for impl, names in sections if re.fullmatch(r"(HL)?Minsumf(32|64)", impl)]
    f64 = [names for impl, names in sections if impl.endswith("f64")]
    assert len(corrected) >= 2 and len(plain) >= 2 and len(f64) >= 2
    for names in corrected:
        hot = [k for k in names if arithmetic_is_minsum(k)]
        assert hot and all("MinsumCorr<" in k for k in hot), [k for k in hot if "MinsumCorr<" not in k][:3]
    for names in plain:
        assert any(arithmetic_is_minsum(k) for k in names)
        assert not any("MinsumCorr<" in k for k in names), [k for k in names if "MinsumCorr<" in k][:3]
    for names in f64:
        assert not any(re.search(r"_kernel<double, 4,", k) for k in names)
    # (the test's own eyes: the f32 sections do launch four codewords per lane, under the name the f64 check looks for)
    assert any(re.search(r"_kernel<float, 4,", k) for _, names in sections for k in names)
