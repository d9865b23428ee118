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
// Both modes end with the stub's count of live device allocations, pinned allocations, events and streams: all zero once
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

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "trace") == 0) return trace_main();
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
