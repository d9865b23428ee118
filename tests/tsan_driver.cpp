// ThreadSanitizer driver for the library's host threading (tests/test_host_sanitizers.py): the real c_api.cpp /
// device_decoder.hip / simulator.hip host code, compiled host-only with -fsanitize=thread and linked against
// tests/hip_stub (streams = worker threads, kernels = no-ops that publish the progress word).  Exercises what round 3
// added -- two execution lanes enqueued by two host threads, the staging thread of the host-buffer entry, the per-lane
// task queues and their event / counter hand-shakes, the progress-word polling with early exits -- and the error
// returns (HIP_STUB_FAIL).  Results are meaningless (no kernel runs); return codes and the absence of TSan reports are
// what is checked.  The reference's contract for a handle is `Send`, one call at a time (src/decoder.rs:19); two
// handles driven by two threads must not interfere either.
// `tsan_driver trace` (with HIP_STUB_TRACE=<file>) instead walks a fixed list of (code, implementation, options) through
// every launch choice the host makes from run-time values, with the host's enqueue order a function of the inputs alone
// ("poll" 0, "lane_threads" 0): the stub writes the launches down, test_launch_trace_* reads them.  The same file lists
// every allocation and every uploaded table (size and hash), so two builds of the library can be compared line by line.
// `tsan_driver stages [1]` drives the six stage handles beside the decoder -- rate matcher, transport block, NR modulation,
// BCH, demodulator, batched encoder -- and the simulator's NR generators through the C ABI, a note line per call; with
// HIP_STUB_TRACE_CALLS the stub writes every runtime call of theirs down.  1: a failure is injected (HIP_STUB_FAIL) and
// must surface as LDPC_TOOLBOX_ERR_DEVICE.
// All modes end with the stub's count of live device allocations, pinned allocations, events and streams: all zero once
// the last handle is gone, also after an injected failure.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../include/ldpc_toolbox.h"

extern "C" unsigned long long hip_stub_launches(void);
extern "C" void hip_stub_trace_note(const char *text);
extern "C" void hip_stub_live(long long counts[4]);

static int leaked() {
  long long c[4];
  hip_stub_live(c);
  std::printf("live after the last handle: device %lld pinned %lld events %lld streams %lld\n", c[0], c[1], c[2], c[3]);
  return (c[0] || c[1] || c[2] || c[3]) ? 1 : 0;
}

static std::string alist_of(const char *spec) {
  const size_t need = ldpc_toolbox_code_alist(spec, nullptr, 0);
  std::string s(need + 1, '\0');
  ldpc_toolbox_code_alist(spec, &s[0], s.size());
  s.resize(need);
  return s;
}

static int64_t get(void *dec, const char *key) {
  int64_t v = -1;
  ldpc_toolbox_decoder_get(dec, key, &v);
  return v;
}

static std::atomic<int> g_errors{0};

// one handle, a sequence of calls; every return code is 0 or a fault code below -1 (never -1: no frame "fails to decode"
// at this level), and without an injected failure it is 0
static int drive(const char *spec, const char *impl, size_t batch, int lanes, int expect_error) {
  const std::string alist = alist_of(spec);
  void *dec = ldpc_toolbox_decoder_ctor_alist_string(alist.c_str(), impl, "");
  if (!dec) {
    if (expect_error) g_errors++;
    else std::fprintf(stderr, "ctor failed: %s\n", ldpc_toolbox_last_error());
    return expect_error ? 0 : 1;
  }
  const size_t n = size_t(get(dec, "n")), k = size_t(get(dec, "k"));
  ldpc_toolbox_decoder_set(dec, "latency", 0);      // the batched paths (the single-launch kernels wait for device flags)
  ldpc_toolbox_decoder_set(dec, "group_size", 256);
  ldpc_toolbox_decoder_set(dec, "lanes", lanes);
  std::vector<float> llrs(batch * n, 1.0f), post(batch * n);
  std::vector<uint8_t> out(batch * k);
  std::vector<int32_t> its(batch);
  int bad = 0;
  auto check = [&](int rc, const char *what) {
    if (rc < -1) g_errors++;
    if (rc == -1 || rc > 0 || (rc != 0 && !expect_error)) {
      std::fprintf(stderr, "%s %s %s: rc %d (%s)\n", spec, impl, what, rc, ldpc_toolbox_last_error());
      bad++;
    }
  };
  for (int threads : {1, 0}) {
    ldpc_toolbox_decoder_set(dec, "lane_threads", threads);
    // host buffers: staging thread + (layered, two lanes) one enqueuing thread per lane
    check(ldpc_toolbox_decoder_decode_batch_f32(dec, out.data(), k, llrs.data(), n, batch, 12, its.data(), post.data()), "host");
    check(ldpc_toolbox_decoder_decode_batch_f32(dec, out.data(), k, llrs.data(), n, batch / 3 + 1, 12, its.data(), nullptr), "host, ragged");
    // "device" buffers (host memory under the stub), the library's own stream, with and without pacing
    for (int throttle : {0, 1}) {
      ldpc_toolbox_decoder_set(dec, "throttle", throttle);
      check(ldpc_toolbox_decoder_decode_batch_f32_device(dec, out.data(), k, llrs.data(), n, batch, 12, its.data(), post.data(), nullptr),
            "device");
    }
  }
  ldpc_toolbox_decoder_set(dec, "profiling", 1);
  check(ldpc_toolbox_decoder_decode_batch_f32(dec, out.data(), k, llrs.data(), n, 300, 6, its.data(), nullptr), "host, profiling");
  uint64_t launches = 0;
  double ms = 0;
  ldpc_toolbox_decoder_kernel_stats(dec, 2, &launches, &ms, 1);
  ldpc_toolbox_decoder_dtor(dec);
  return bad;
}

// The single-launch small-batch paths (four frames; under the stub their kernels do nothing and the error word stays zero):
// each call twice, so that a first call that failed while it uploaded its tables is followed by one that uploads them again.
static int drive_small_batch(const char *spec, const char *impl, int expect_error) {
  const std::string alist = alist_of(spec);
  void *dec = ldpc_toolbox_decoder_ctor_alist_string(alist.c_str(), impl, "");
  if (!dec) {
    std::fprintf(stderr, "ctor failed: %s\n", ldpc_toolbox_last_error());
    return 1;
  }
  const size_t n = size_t(get(dec, "n")), k = size_t(get(dec, "k")), batch = 4;
  std::vector<float> llrs(batch * n, 1.0f), post(batch * n);
  std::vector<uint8_t> out(batch * k);
  std::vector<int32_t> its(batch);
  int bad = 0;
  for (int call = 0; call < 4; call++) {
    const int rc = call < 2 ? ldpc_toolbox_decoder_decode_batch_f32(dec, out.data(), k, llrs.data(), n, batch, 12, its.data(), post.data())
                            : ldpc_toolbox_decoder_decode_batch_f32_device(dec, out.data(), k, llrs.data(), n, batch, 12, its.data(), post.data(), nullptr);
    if (rc < -1) g_errors++;
    if (rc == -1 || rc > 0 || (rc != 0 && !expect_error)) {
      std::fprintf(stderr, "%s %s small batch, call %d: rc %d (%s)\n", spec, impl, call, rc, ldpc_toolbox_last_error());
      bad++;
    }
  }
  ldpc_toolbox_decoder_dtor(dec);
  return bad;
}

// ---- trace mode ------------------------------------------------------------------------------------------------------

// a 14 x n matrix with eight long rows of base .. base + 3 * spread edges and six shorter ones, every column in at least one
// row (as test_rows_beyond_the_lds_limit builds, without the random numbers).  "long-rows": 330..420 edges, beyond the 320
// the LDS-staged kernels hold; "wide-rows": at most 64, beyond a 32-bit sign mask and a three-word row record
static std::string synthetic_alist(size_t n, size_t base, size_t spread) {
  const size_t m = 14;
  const size_t step[14] = {7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 49, 53};  // coprime to n: a row's columns are distinct
  std::vector<std::vector<size_t>> col_rows(n);
  for (size_t r = 0; r < m; r++) {
    const size_t deg = r < 8 ? base + spread * (r % 4) : 5 + r;
    for (size_t i = 0; i < deg; i++) col_rows[(r * 101 + i * step[r]) % n].push_back(r);
  }
  for (size_t c = 0; c < n; c++)
    if (col_rows[c].empty()) col_rows[c].push_back(8 + c % 6);
  std::string a = std::to_string(n) + " 14\n\n\n\n";  // (the reader takes the dimensions and the column lists)
  for (size_t c = 0; c < n; c++) {
    for (size_t r : col_rows[c]) a += std::to_string(r + 1) + " ";
    a += "\n";
  }
  return a;
}

struct TraceCase {
  const char *spec, *impl;
  std::vector<std::vector<std::pair<const char *, int>>> option_sets;  // each on top of the defaults
  int llrs_f64 = -1;  // the caller's LLRs: -1 = in the implementation's precision
  size_t small_batch = 0;  // not 0: a call of this many frames with the single-launch small-batch paths left on
};

// 300 frames in groups of 256 (one full group, one ragged), 3 iterations (a first one and later ones), host and device entry
// (small_batch: that many frames through latency.hip.h / latency_edge.hip.h -- under the stub their kernels do nothing and
// the error word stays zero, so the calls stage, launch once and copy back)
static int trace_case(const TraceCase &tc) {
  const std::string alist = std::strcmp(tc.spec, "long-rows") == 0   ? synthetic_alist(1500, 330, 30)
                            : std::strcmp(tc.spec, "wide-rows") == 0 ? synthetic_alist(500, 40, 3)
                                                                     : alist_of(tc.spec);
  const bool f64 = tc.llrs_f64 < 0 ? std::strstr(tc.impl, "f64") != nullptr : tc.llrs_f64 != 0;
  int bad = 0;
  for (const auto &options : tc.option_sets) {
    void *dec = ldpc_toolbox_decoder_ctor_alist_string(alist.c_str(), tc.impl, "");
    if (!dec) {
      std::fprintf(stderr, "%s %s: ctor failed: %s\n", tc.spec, tc.impl, ldpc_toolbox_last_error());
      return 1;
    }
    std::string note = std::string(tc.impl) + " " + tc.spec + (f64 ? " llrs=f64" : " llrs=f32");
    for (const auto &kv : {std::pair<const char *, int>{"latency", 0}, {"latency_edge", 0}, {"group_size", 256}, {"poll", 0}, {"lane_threads", 0}})
      if (!tc.small_batch || std::strncmp(kv.first, "latency", 7) != 0) ldpc_toolbox_decoder_set(dec, kv.first, kv.second);
    if (tc.small_batch) note += " small-batch";
    for (const auto &kv : options) {
      if (ldpc_toolbox_decoder_set(dec, kv.first, kv.second) != 0) {
        std::fprintf(stderr, "%s: option %s refused\n", tc.impl, kv.first);
        bad++;
      }
      note += std::string(" ") + kv.first + "=" + std::to_string(kv.second);
    }
    hip_stub_trace_note(note.c_str());
    const size_t n = size_t(get(dec, "n")), k = size_t(get(dec, "k")), batch = tc.small_batch ? tc.small_batch : 300;
    std::vector<uint8_t> out(batch * k);
    std::vector<int32_t> its(batch);
    int rc_host, rc_device;
    if (f64) {
      std::vector<double> llrs(batch * n, 1.0), post(batch * n);
      rc_host = ldpc_toolbox_decoder_decode_batch_f64(dec, out.data(), k, llrs.data(), n, batch, 3, its.data(), post.data());
      rc_device = ldpc_toolbox_decoder_decode_batch_f64_device(dec, out.data(), k, llrs.data(), n, batch, 3, its.data(), post.data(), nullptr);
    } else {
      std::vector<float> llrs(batch * n, 1.0f), post(batch * n);
      rc_host = ldpc_toolbox_decoder_decode_batch_f32(dec, out.data(), k, llrs.data(), n, batch, 3, its.data(), post.data());
      rc_device = ldpc_toolbox_decoder_decode_batch_f32_device(dec, out.data(), k, llrs.data(), n, batch, 3, its.data(), post.data(), nullptr);
    }
    if (rc_host != 0 || rc_device != 0) {
      std::fprintf(stderr, "%s: rc %d / %d (%s)\n", note.c_str(), rc_host, rc_device, ldpc_toolbox_last_error());
      bad++;
    }
    ldpc_toolbox_decoder_dtor(dec);
  }
  return bad;
}

static int trace_main() {
  std::vector<std::vector<std::pair<const char *, int>>> flooding_minsum;
  for (int vec : {4, 2, 1})
    for (int records : {0, 2})
      for (int lfree : {0, 1}) flooding_minsum.push_back({{"vec", vec}, {"records", records}, {"lfree", lfree}});
  flooding_minsum.push_back({{"records", 2}, {"rec_long", 1}});
  flooding_minsum.push_back({{"staged_minsum", 1}});
  // the layered min-sum forms: row records, register-resident rows, streaming, the two-pass level kernel (x register-resident)
  const std::vector<std::vector<std::pair<const char *, int>>> layered_minsum = {
      {}, {{"vec", 2}}, {{"vec", 1}}, {{"hl_records", 0}}, {{"hl_records", 0}, {"vec", 1}}, {{"hl_reg", 0}}, {{"hl_reg", 0}, {"vec", 2}}, {{"hl_reg", 0}, {"vec", 1}}, {{"staged_minsum", 1}},
      {{"staged_minsum", 1}, {"hl_reg", 0}}, {{"serial_levels", 0}}, {{"serial_levels", 0}, {"hl_reg", 0}}};
  const std::vector<std::vector<std::pair<const char *, int>>> layered_staged = {
      {}, {{"hl_reg", 0}}, {{"serial_levels", 0}}, {{"serial_levels", 0}, {"hl_reg", 0}}};
  const std::vector<TraceCase> cases = {
      {"ar4ja:1/2:1024", "Minsumf32", flooding_minsum},
      {"ar4ja:1/2:1024", "Minsumf64", {{{"vec", 4}}, {{"vec", 4}, {"records", 2}}, {{"vec", 4}, {"lfree", 0}}}},
      {"ar4ja:1/2:1024", "NormMinsumf32", flooding_minsum},
      {"nr5g:1:8", "HLOffsetMinsumf64", layered_minsum},
      {"wide-rows", "Minsumf32", {{{"lfree", 0}, {"records", 0}}, {{"records", 0}}, {{"records", 2}}, {{"records", 2}, {"vn_event", 0}}}},
      {"wide-rows", "OffsetMinsumf64", {{{"lfree", 0}, {"records", 0}}, {{"records", 2}}}},
      {"ar4ja:1/2:1024", "Tanhf32", {{{"cn_reg", 0}}, {{"cn_reg", 1}}}},
      {"dvbs2:R3_5short", "Tanhf32", {{}}},
      {"ar4ja:1/2:1024", "Phif32@fast", {{}}, 1},
      {"nr5g:1:8", "HLTanhf32@fast", {{}}},
      {"nr5g:1:8", "HLTanhf32", layered_staged},
      {"nr5g:1:8", "HLMinsumf32", layered_minsum},
      {"dvbs2:R1_2short", "HLMinsumf32", {{}, {{"hl_records", 0}}, {{"hl_reg", 0}}}},
      {"dvbs2:R8_9short", "HLNormMinsumf32", {{}}},
      {"dvbs2:R8_9short", "Minsumf32", {{{"records", 2}}, {{"records", 2}, {"vn_event", 0}}}},
      {"long-rows", "Phif32", {{}}},
      {"long-rows", "HLPhif32", {{}}},
      {"long-rows", "Minsumf32", {{}, {{"staged_minsum", 1}}}},
      {"long-rows", "HLOffsetMinsumf32", {{}, {{"staged_minsum", 1}}}},
      {"long-rows", "Minstarapproxi8", {{}}},
      {"long-rows", "HLAminstari8", {{}}},
      {"nr5g:1:8", "Minstarapproxi8", {{}}, 1},
      {"nr5g:1:8", "HLAminstari8", {{}, {{"hl_reg", 0}}, {{"serial_levels", 0}}}},
      {"nr5g:1:8", "Minsumi8Norm", {{}}},
      {"nr5g:1:8", "HLMinsumi8Offset", {{}, {{"hl_reg", 0}}, {{"serial_levels", 0}}}},
      // the small-batch paths: LatencyPath (flooding Minsumf32), EdgeLatencyPath layered and flooding
      {"dvbs2:R1_2short", "Minsumf32", {{}}, -1, 4},
      {"nr5g:1:8", "HLTanhf32", {{}}, -1, 4},
      {"ar4ja:1/2:1024", "Tanhf32", {{}}, -1, 4},
  };
  int bad = 0;
  size_t scenarios = 0;
  for (const auto &tc : cases) {
    bad += trace_case(tc);
    scenarios += tc.option_sets.size();
  }
  bad += leaked();
  std::printf("trace: %s (%zu scenarios, %llu kernel launches through the stub)\n", bad ? "FAILED" : "ok", scenarios, hip_stub_launches());
  return bad ? 1 : 0;
}

// ---- stages mode -----------------------------------------------------------------------------------------------------

// One call of a stage handle: the note goes into the trace before the call, so the stub's lines of the call follow it.  A
// return code other than 0 is written out with the library's message; it counts as a fault unless a failure was injected
// and the code is LDPC_TOOLBOX_ERR_DEVICE (-2).
struct StageRun {
  bool expect_error;
  int bad = 0, errors = 0;
  template <typename F>
  void operator()(const std::string &what, F call) {
    hip_stub_trace_note(what.c_str());
    const int rc = call();
    if (rc == 0) return;
    std::printf("stages: %s: rc %d: %s\n", what.c_str(), rc, ldpc_toolbox_last_error());
    if (expect_error && rc == LDPC_TOOLBOX_ERR_DEVICE)
      errors++;
    else
      bad++;
  }
};

static int64_t tb_get(void *tb, const char *key) {
  int64_t v = -1;
  ldpc_toolbox_nr_tb_get(tb, key, &v);
  return v;
}

// Every stage handle (rate matcher, transport block, NR modulation, BCH, demodulator, batched encoder) through its host
// entry and its _device entry with a null stream, at the smallest shapes that reach every branch of the launch plumbing,
// then the simulator's two NR generators.  Under the stub every pointer is host memory, so the _device entries take the
// same buffers.  All stages are single: the multi-stage loops need 2^28-byte buffers and are covered on the GPU.
static int stages_main(bool expect_error) {
  StageRun run{expect_error};
  const size_t batch = 3;
  // (16-byte aligned storage for every element type)
  std::vector<double> store_a(1 << 14), store_b(1 << 14), store_c(1 << 14);
  void *const a = store_a.data(), *const b = store_b.data(), *const c = store_c.data();
  uint8_t *const a8 = static_cast<uint8_t *>(a), *const b8 = static_cast<uint8_t *>(b), *const c8 = static_cast<uint8_t *>(c);
  float *const af = static_cast<float *>(a), *const bf = static_cast<float *>(b), *const cf = static_cast<float *>(c);
  double *const ad = static_cast<double *>(a), *const bd = static_cast<double *>(b), *const cd = static_cast<double *>(c);
  int8_t *const ai = static_cast<int8_t *>(a), *const bi = static_cast<int8_t *>(b);

  {  // rate matcher: n = 104
    void *rm = ldpc_toolbox_nr_rm_ctor("nr5g:2:2", 0);
    if (!rm) return 1;
    const size_t n = 104, e = 96;
    run("nr_rm match host", [&] { return ldpc_toolbox_nr_rm_match(rm, b8, e, a8, n, batch, 0, 2); });
    run("nr_rm match device", [&] { return ldpc_toolbox_nr_rm_match_device(rm, b8, e, a8, n, batch, 0, 2, nullptr); });
    for (int combine : {0, 1}) {
      const std::string tail = combine ? " combine" : "";
      run("nr_rm recover f32 host" + tail, [&] { return ldpc_toolbox_nr_rm_recover_f32(rm, bf, n, af, e, batch, 2, 2, 20.0, combine); });
      run("nr_rm recover f64 host" + tail, [&] { return ldpc_toolbox_nr_rm_recover_f64(rm, bd, n, ad, e, batch, 2, 2, 20.0, combine); });
      run("nr_rm recover f32 device" + tail,
          [&] { return ldpc_toolbox_nr_rm_recover_f32_device(rm, bf, n, af, e, batch, 2, 2, 20.0, combine, nullptr); });
      run("nr_rm recover f64 device" + tail,
          [&] { return ldpc_toolbox_nr_rm_recover_f64_device(rm, bd, n, ad, e, batch, 2, 2, 20.0, combine, nullptr); });
      run("nr_rm recover i8 host" + tail, [&] { return ldpc_toolbox_nr_rm_recover_i8(rm, bi, n, ai, e, batch, 0, 2, 100, combine); });
      // (an odd address: the kernel's pieces follow the address)
      run("nr_rm recover i8 device" + tail,
          [&] { return ldpc_toolbox_nr_rm_recover_i8_device(rm, bi + 1, n, ai, e, batch, 0, 2, 100, combine, nullptr); });
    }
    ldpc_toolbox_nr_rm_dtor(rm);
  }

  for (const char *spec : {"nr5g-tb:2:100", "nr5g-tb:2:4000"}) {  // transport block: C = 1 and C = 2
    void *tb = ldpc_toolbox_nr_tb_ctor(spec, 0);
    if (!tb) return 1;
    const size_t ta = size_t(tb_get(tb, "a")), tc = size_t(tb_get(tb, "c")), tk = size_t(tb_get(tb, "k"));
    const size_t q = 2, g = q * (50 * tc + tc - 1);  // (C = 2: one block of 100 and one of 102)
    const std::string name = std::string("nr_tb C=") + std::to_string(tc) + " ";
    run(name + "segment host", [&] { return ldpc_toolbox_nr_tb_segment(tb, b8, tk, a8, ta, batch); });
    run(name + "segment device", [&] { return ldpc_toolbox_nr_tb_segment_device(tb, b8, tk, a8, ta, batch, nullptr); });
    for (int flags : {1, 0}) {
      uint8_t *const tb_ok = c8, *const cb_ok = flags ? c8 + 64 : nullptr;
      const std::string tail = flags ? " cb_ok" : "";
      run(name + "desegment host" + tail, [&] { return ldpc_toolbox_nr_tb_desegment(tb, a8, ta, tb_ok, cb_ok, b8, tk, batch); });
      run(name + "desegment device" + tail,
          [&] { return ldpc_toolbox_nr_tb_desegment_device(tb, a8, ta, tb_ok, cb_ok, b8, tk, batch, nullptr); });
    }
    run(name + "concatenate host", [&] { return ldpc_toolbox_nr_tb_concatenate(tb, b8, g, a8, q, batch); });
    run(name + "concatenate device", [&] { return ldpc_toolbox_nr_tb_concatenate_device(tb, b8 + 1, g, a8, q, batch, nullptr); });
    run(name + "split f32 host", [&] { return ldpc_toolbox_nr_tb_split_f32(tb, bf, af, g, q, batch); });
    run(name + "split f64 host", [&] { return ldpc_toolbox_nr_tb_split_f64(tb, bd, ad, g, q, batch); });
    run(name + "split f32 device", [&] { return ldpc_toolbox_nr_tb_split_f32_device(tb, bf, af, g, q, batch, nullptr); });
    run(name + "split f64 device", [&] { return ldpc_toolbox_nr_tb_split_f64_device(tb, bd, ad, g, q, batch, nullptr); });
    ldpc_toolbox_nr_tb_dtor(tb);
  }

  for (int qm : {2, 4, 6, 8}) {  // NR modulation: 5 symbols
    void *qam = ldpc_toolbox_nr_qam_ctor(("nr5g-qam:" + std::to_string(qm)).c_str(), 0);
    if (!qam) return 1;
    const size_t sl = 5, ll = sl * size_t(qm);
    const std::string name = "nr_qam QM=" + std::to_string(qm) + " ";
    for (int64_t c_init : {int64_t(-1), int64_t(7)}) {
      const std::string ci = " c_init=" + std::to_string(c_init);
      run(name + "mod f32 host" + ci, [&] { return ldpc_toolbox_nr_qam_mod_f32(qam, bf, sl, a8, ll, batch, c_init); });
      run(name + "mod f64 host" + ci, [&] { return ldpc_toolbox_nr_qam_mod_f64(qam, bd, sl, a8, ll, batch, c_init); });
      run(name + "mod f32 device" + ci, [&] { return ldpc_toolbox_nr_qam_mod_f32_device(qam, bf, sl, a8, ll, batch, c_init, nullptr); });
      run(name + "mod f64 device" + ci, [&] { return ldpc_toolbox_nr_qam_mod_f64_device(qam, bd, sl, a8, ll, batch, c_init, nullptr); });
      for (int max_log : {0, 1}) {
        const std::string tail = std::string(max_log ? " max-log" : " exact") + ci;
        run(name + "demod f32 host" + tail, [&] { return ldpc_toolbox_nr_qam_demod_f32(qam, bf, ll, af, sl, batch, 0.5, max_log, c_init); });
        run(name + "demod f64 host" + tail, [&] { return ldpc_toolbox_nr_qam_demod_f64(qam, bd, ll, ad, sl, batch, 0.5, max_log, c_init); });
        run(name + "demod f32 device" + tail,
            [&] { return ldpc_toolbox_nr_qam_demod_f32_device(qam, bf, ll, af, sl, batch, 0.5, max_log, c_init, nullptr); });
        run(name + "demod f64 device" + tail,
            [&] { return ldpc_toolbox_nr_qam_demod_f64_device(qam, bd, ll, ad, sl, batch, 0.5, max_log, c_init, nullptr); });
        run(name + "demap_i8 host" + tail, [&] { return ldpc_toolbox_nr_demap_i8(qam, bi, ll, af, sl, batch, 0.5, max_log, c_init); });
        run(name + "demap_i8 device, aligned" + tail,
            [&] { return ldpc_toolbox_nr_demap_i8_device(qam, bi, ll, af, sl, batch, 0.5, max_log, c_init, nullptr); });
        run(name + "demap_i8 device, odd address" + tail,
            [&] { return ldpc_toolbox_nr_demap_i8_device(qam, bi + 1, ll, af, sl, batch, 0.5, max_log, c_init, nullptr); });
        run(name + "demap_csi f32 host" + tail, [&] { return ldpc_toolbox_nr_demap_csi_f32(qam, bf, ll, af, cf, sl, batch, max_log, c_init); });
        run(name + "demap_csi f64 host" + tail, [&] { return ldpc_toolbox_nr_demap_csi_f64(qam, bd, ll, ad, cd, sl, batch, max_log, c_init); });
        run(name + "demap_csi i8 host" + tail, [&] { return ldpc_toolbox_nr_demap_csi_i8(qam, bi, ll, af, cf, sl, batch, max_log, c_init); });
        run(name + "demap_csi f32 device" + tail,
            [&] { return ldpc_toolbox_nr_demap_csi_f32_device(qam, bf, ll, af, cf, sl, batch, max_log, c_init, nullptr); });
        run(name + "demap_csi f64 device" + tail,
            [&] { return ldpc_toolbox_nr_demap_csi_f64_device(qam, bd, ll, ad, cd, sl, batch, max_log, c_init, nullptr); });
        run(name + "demap_csi i8 device, aligned" + tail,
            [&] { return ldpc_toolbox_nr_demap_csi_i8_device(qam, bi, ll, af, cf, sl, batch, max_log, c_init, nullptr); });
        run(name + "demap_csi i8 device, odd address" + tail,
            [&] { return ldpc_toolbox_nr_demap_csi_i8_device(qam, bi + 1, ll, af, cf, sl, batch, max_log, c_init, nullptr); });
      }
    }
    // the cached sequence: (7, ll) is there; another c_init and another length generate it again
    run(name + "demod f32 host, the same sequence", [&] { return ldpc_toolbox_nr_qam_demod_f32(qam, bf, ll, af, sl, batch, 0.5, 1, 7); });
    run(name + "demod f32 host, another c_init", [&] { return ldpc_toolbox_nr_qam_demod_f32(qam, bf, ll, af, sl, batch, 0.5, 1, 9); });
    run(name + "mod f32 device, another length",
        [&] { return ldpc_toolbox_nr_qam_mod_f32_device(qam, bf, sl - 1, a8, ll - size_t(qm), batch, 9, nullptr); });
    run(name + "sequence", [&] { return ldpc_toolbox_nr_qam_sequence(qam, b8, 100, 9); });
    ldpc_toolbox_nr_qam_dtor(qam);
  }

  {  // BCH: n = 15, k = 7, t = 2
    void *bch = ldpc_toolbox_bch_ctor("bch:4:13:2:15", 0);
    if (!bch) return 1;
    int32_t *const errs = static_cast<int32_t *>(c);
    run("bch encode host", [&] { return ldpc_toolbox_bch_encode_batch(bch, b8, 15, a8, 7, batch); });
    run("bch encode device", [&] { return ldpc_toolbox_bch_encode_batch_device(bch, b8, 15, a8, 7, batch, nullptr); });
    run("bch decode host", [&] { return ldpc_toolbox_bch_decode_batch(bch, a8, 7, b8, 15, batch, nullptr); });
    run("bch decode host, errors", [&] { return ldpc_toolbox_bch_decode_batch(bch, a8, 15, b8, 15, batch, errs); });
    run("bch decode device", [&] { return ldpc_toolbox_bch_decode_batch_device(bch, a8, 7, b8, 15, batch, nullptr, nullptr); });
    run("bch decode device, errors", [&] { return ldpc_toolbox_bch_decode_batch_device(bch, a8, 15, b8, 15, batch, errs, nullptr); });
    ldpc_toolbox_bch_dtor(bch);
  }

  for (const char *modulation : {"BPSK", "8PSK"}) {  // demodulator: reals, and a table constellation
    void *demod = ldpc_toolbox_demod_ctor(modulation, 0);
    if (!demod) return 1;
    const bool bpsk = std::strcmp(modulation, "BPSK") == 0;
    const size_t sl = 5, ll = bpsk ? sl : 3 * sl;
    const std::string name = std::string("demod ") + modulation + " ";
    for (int max_log : {0, 1}) {
      const std::string tail = max_log ? " max-log" : " exact";
      run(name + "run f32 host" + tail, [&] { return ldpc_toolbox_demod_run_f32(demod, bf, ll, af, sl, batch, 0.5, 0, max_log); });
      run(name + "run f64 host" + tail, [&] { return ldpc_toolbox_demod_run_f64(demod, bd, ll, ad, sl, batch, 0.5, 0, max_log); });
      run(name + "run f32 device" + tail, [&] { return ldpc_toolbox_demod_run_f32_device(demod, bf, ll, af, sl, batch, 0.5, 0, max_log, nullptr); });
      run(name + "run f64 device" + tail, [&] { return ldpc_toolbox_demod_run_f64_device(demod, bd, ll, ad, sl, batch, 0.5, 0, max_log, nullptr); });
    }
    run(name + "mod f32 host", [&] { return ldpc_toolbox_mod_run_f32(demod, bf, sl, a8, ll, batch, 0); });
    run(name + "mod f64 host", [&] { return ldpc_toolbox_mod_run_f64(demod, bd, sl, a8, ll, batch, 0); });
    run(name + "mod f32 device", [&] { return ldpc_toolbox_mod_run_f32_device(demod, bf, sl, a8, ll, batch, 0, nullptr); });
    run(name + "mod f64 device", [&] { return ldpc_toolbox_mod_run_f64_device(demod, bd, sl, a8, ll, batch, 0, nullptr); });
    run(name + "awgn f32 host", [&] { return ldpc_toolbox_awgn_run_f32(demod, bf, sl, batch, 0.5, 1, 0); });
    run(name + "awgn f64 host", [&] { return ldpc_toolbox_awgn_run_f64(demod, bd, sl, batch, 0.5, 1, 0); });
    run(name + "awgn f32 device", [&] { return ldpc_toolbox_awgn_run_f32_device(demod, bf, sl, batch, 0.5, 1, 0, nullptr); });
    run(name + "awgn f64 device", [&] { return ldpc_toolbox_awgn_run_f64_device(demod, bd, sl, batch, 0.5, 1, 0, nullptr); });
    if (!bpsk) {  // (the fading channel takes complex symbols)
      run(name + "fading f32 host", [&] { return ldpc_toolbox_fading_run_f32(demod, bf, cf, sl, batch, 0.5, 2, 1, 0); });
      run(name + "fading f64 host", [&] { return ldpc_toolbox_fading_run_f64(demod, bd, cd, sl, batch, 0.5, 2, 1, 0); });
      run(name + "fading f32 device", [&] { return ldpc_toolbox_fading_run_f32_device(demod, bf, cf, sl, batch, 0.5, 2, 1, 0, nullptr); });
      run(name + "fading f64 device", [&] { return ldpc_toolbox_fading_run_f64_device(demod, bd, cd, sl, batch, 0.5, 2, 1, 0, nullptr); });
    }
    ldpc_toolbox_demod_dtor(demod);
  }

  // batched encoder: a staircase code and a dense one, without and with a puncturing pattern
  for (const char *spec : {"dvbs2:R1_2short", "nr5g:2:2"})
    for (const char *pattern : {"", "1,1,1,0"}) {
      const std::string alist = alist_of(spec);
      void *enc = ldpc_toolbox_encoder_ctor_alist_string_on_device(alist.c_str(), pattern, 0);
      if (!enc) {
        std::fprintf(stderr, "%s [%s]: encoder ctor failed: %s\n", spec, pattern, ldpc_toolbox_last_error());
        return 1;
      }
      int64_t k = 0, out_len = 0;
      ldpc_toolbox_encoder_get(enc, "k", &k);
      ldpc_toolbox_encoder_get(enc, "output_len", &out_len);
      const std::string name = std::string("encoder ") + spec + " [" + pattern + "] ";
      run(name + "host", [&] { return ldpc_toolbox_encoder_encode_batch(enc, b8, size_t(out_len), a8, size_t(k), batch); });
      run(name + "device", [&] { return ldpc_toolbox_encoder_encode_batch_device(enc, b8, size_t(out_len), a8, size_t(k), batch, nullptr); });
      ldpc_toolbox_encoder_dtor(enc);
    }

  {  // the simulator's two NR generators, over AWGN and over the block-fading channel, either fold step
    const std::string alist = alist_of("nr5g:2:2");
    void *sim = ldpc_toolbox_sim_ctor(alist.c_str(), "Minsumf32", "", 0, 4, 1);
    void *qam = ldpc_toolbox_nr_qam_ctor("nr5g-qam:4", 0);
    void *rm = ldpc_toolbox_nr_rm_ctor("nr5g:2:2", 0);
    if (!sim || !qam || !rm) {
      std::fprintf(stderr, "simulator: ctor failed: %s\n", ldpc_toolbox_last_error());
      return 1;
    }
    const uint64_t e[2] = {96, 48};
    const uint32_t rv[2] = {0, 2};
    for (int max_log : {0, 1}) {
      run("sim set_nr_qam", [&] { return ldpc_toolbox_sim_set_nr_qam(sim, qam, max_log); });
      run("sim set_harq", [&] { return ldpc_toolbox_sim_set_harq(sim, rm, e, rv, 2, 4); });
      for (int fading_block : {0, 3}) {
        const std::string tail = std::string(max_log ? " max-log" : " exact") + " fading_block=" + std::to_string(fading_block);
        run("sim set fading_block", [&] { return ldpc_toolbox_sim_set(sim, "fading_block", fading_block); });
        run("sim generate" + tail, [&] { return ldpc_toolbox_sim_generate(sim, 3.0, 1, 0, batch, af, nullptr); });
        run("sim generate_harq" + tail, [&] { return ldpc_toolbox_sim_generate_harq(sim, 3.0, 1, 0, batch, 1, af, nullptr); });
      }
    }
    ldpc_toolbox_nr_rm_dtor(rm);
    ldpc_toolbox_nr_qam_dtor(qam);
    ldpc_toolbox_sim_dtor(sim);
  }

  if (expect_error && run.errors == 0) {
    std::fprintf(stderr, "the injected failure never surfaced\n");
    run.bad++;
  }
  run.bad += leaked();
  std::printf("stages: %s (%llu kernel launches through the stub)\n", run.bad ? "FAILED" : "ok", hip_stub_launches());
  return run.bad ? 1 : 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "trace") == 0) return trace_main();
  if (argc > 1 && std::strcmp(argv[1], "stages") == 0) return stages_main(argc > 2 && std::atoi(argv[2]) != 0);
  const int expect_error = argc > 1 ? std::atoi(argv[1]) : 0;
  int bad = 0;
  bad += drive("nr5g:1:8", "HLMinsumf32", 2048, 2, expect_error);   // layered: lane threads
  bad += drive("nr5g:2:8", "HLTanhf32", 1500, 2, expect_error);
  bad += drive("ar4ja:1/2:1024", "Minsumf32", 1024, 2, expect_error);  // flooding, two lanes
  bad += drive("nr5g:1:8", "Minstarapproxi8", 1024, 1, expect_error);
  // two handles on two threads at once
  int rc_a = 0, rc_b = 0;
  std::thread a([&] { rc_a = drive("nr5g:1:8", "HLTanhf32", 1024, 2, expect_error); });
  std::thread b([&] { rc_b = drive("nr5g:2:8", "HLMinsumf32", 1024, 2, expect_error); });
  a.join();
  b.join();
  bad += rc_a + rc_b;
  bad += drive_small_batch("dvbs2:R1_2short", "Minsumf32", expect_error);  // latency.hip.h
  bad += drive_small_batch("nr5g:1:8", "HLTanhf32", expect_error);         // latency_edge.hip.h
  if (expect_error && g_errors.load() == 0) {
    std::fprintf(stderr, "the injected failure never surfaced\n");
    bad++;
  }
  bad += leaked();
  std::printf("tsan driver: %s (%llu kernel launches through the stub)\n", bad ? "FAILED" : "ok", hip_stub_launches());
  return bad ? 1 : 0;
}
