// A host-only stand-in for the HIP runtime, for ThreadSanitizer runs of the library's HOST threading on a machine
// without a GPU (tests/test_host_sanitizers.py; SURVEY.md section 5 "Race detection").  Test infrastructure only.
//   * a stream is an in-order worker thread executing queued closures;
//   * an event is a pair of counters (records issued / completed): hipStreamWaitEvent waits for the record issued
//     last before the call, as HIP does;
//   * device memory is host memory; copies and memsets run on the stream's thread;
//   * a kernel launch is a no-op -- except that a launch carrying a decoder State with a progress word publishes
//     (epoch, iteration, codewords running) there as the real kernels do, with "running" scripted by HIP_STUB_DONE_AT
//     (0 from that iteration on: the host's early-termination paths run);
//   * HIP_STUB_FAIL=<function>:<n> makes the n-th call of that function return hipErrorUnknown (the functions with a
//     STUB_FAIL line below);
//   * HIP_STUB_TRACE=<file> appends one line per kernel launch, in the host's enqueue order: the stream's ordinal in
//     creation order, grid, block, dynamic LDS bytes and the kernel's demangled name (hip_stub_trace_note adds a "# ..."
//     line) -- and "malloc <bytes>" per hipMalloc, "hostmalloc <bytes>" per hipHostMalloc, "h2d <bytes> <FNV-1a of the
//     bytes, 64 bits>" per synchronous host-to-device hipMemcpy: what the library allocates and the tables it uploads;
//   * HIP_STUB_TRACE_CALLS (beside HIP_STUB_TRACE) adds one line for each hipSetDevice, hipMemcpyAsync (kind, bytes, stream
//     ordinal), hipMemsetAsync, hipEventRecord and hipStreamWaitEvent (the event's ordinal in creation order, the stream's),
//     hipStreamSynchronize and hipGetLastError, written as the call is entered: the host's whole call sequence around its
//     launches, so that two builds of the library can be compared call by call (`tsan_driver stages`);
//   * hip_stub_live counts what has been created and not yet given back: device and pinned allocations, events, streams.
// Built with the same host-only clang mode as the library objects it is linked with (it needs dev::State).
#include <cxxabi.h>
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>

// (the kernel header defines non-template kernels: a private copy of its namespace keeps the stub from clashing with
// the library objects it is linked with; only dev::State and dev::progress_word are used here)
#define dev dev_for_the_stub
#include "../../ldpc_toolbox_amd/csrc/kernels.hip.h"
#undef dev

namespace {

std::atomic<unsigned> g_streams{0};

struct Stream {
  const unsigned ordinal = g_streams++;  // in creation order (HIP_STUB_TRACE)
  std::thread worker;
  std::mutex m;
  std::condition_variable cv, idle;
  std::deque<std::function<void()>> q;
  bool closing = false;
  uint64_t submitted = 0, completed = 0;
  Stream() {
    worker = std::thread([this] {
      for (;;) {
        std::function<void()> f;
        {
          std::unique_lock<std::mutex> lock(m);
          cv.wait(lock, [&] { return closing || !q.empty(); });
          if (q.empty()) return;
          f = std::move(q.front());
          q.pop_front();
        }
        f();
        {
          std::lock_guard<std::mutex> lock(m);
          completed++;
        }
        idle.notify_all();
      }
    });
  }
  void push(std::function<void()> f) {
    {
      std::lock_guard<std::mutex> lock(m);
      q.push_back(std::move(f));
      submitted++;
    }
    cv.notify_one();
  }
  void sync() {
    std::unique_lock<std::mutex> lock(m);
    idle.wait(lock, [&] { return completed == submitted; });
  }
  bool busy() {
    std::lock_guard<std::mutex> lock(m);
    return completed != submitted;
  }
  ~Stream() {
    {
      std::lock_guard<std::mutex> lock(m);
      closing = true;
    }
    cv.notify_all();
    if (worker.joinable()) worker.join();
  }
};

struct EventState {
  std::mutex m;
  std::condition_variable cv;
  uint64_t issued = 0, completed = 0;
};
// (the handle owns a reference, and so does every queued closure: destroying an event that streams still refer to is
// legal in HIP)
std::atomic<unsigned> g_events{0};
struct Event {
  const unsigned ordinal = g_events++;  // in creation order (HIP_STUB_TRACE_CALLS)
  std::shared_ptr<EventState> st = std::make_shared<EventState>();
};

Stream *default_stream() {
  static Stream *s = new Stream();  // (leaked on purpose: outlives every static destructor)
  return s;
}
Stream *as_stream(hipStream_t s) { return s ? reinterpret_cast<Stream *>(s) : default_stream(); }

std::mutex g_reg_mutex;
std::map<const void *, std::string> &kernel_names() {
  static std::map<const void *, std::string> m;
  return m;
}

struct LaunchConfig {
  dim3 grid, block;
  size_t shmem;
  hipStream_t stream;
};
thread_local LaunchConfig t_config;

std::atomic<uint64_t> g_launches{0};
// live device allocations, pinned allocations, events and streams (the stub's own default stream is not counted)
std::atomic<long long> g_live[4];
enum { kLiveDevice = 0, kLivePinned = 1, kLiveEvents = 2, kLiveStreams = 3 };

// HIP_STUB_TRACE: one line at a time, appended by whichever host thread makes the launch
void trace_line(const std::string &line) {
  static const char *path = std::getenv("HIP_STUB_TRACE");
  if (!path) return;
  static std::mutex m;
  std::lock_guard<std::mutex> lock(m);
  static std::FILE *f = std::fopen(path, "a");
  if (!f) return;
  std::fputs(line.c_str(), f);
  std::fputc('\n', f);
  std::fflush(f);
}
// HIP_STUB_TRACE_CALLS: the runtime calls around the launches as well
bool trace_calls() {
  static const bool on = std::getenv("HIP_STUB_TRACE_CALLS") != nullptr;
  return on;
}
std::string demangled(const std::string &name) {
  int status = 0;
  char *d = abi::__cxa_demangle(name.c_str(), nullptr, nullptr, &status);
  std::string out = (status == 0 && d) ? d : name;
  std::free(d);
  return out;
}

bool fail_now(const char *fn) {
  static const char *spec = std::getenv("HIP_STUB_FAIL");
  if (!spec) return false;
  static std::mutex m;
  static std::map<std::string, uint64_t> calls;
  const char *colon = std::strchr(spec, ':');
  if (!colon || std::strncmp(spec, fn, size_t(colon - spec)) != 0 || std::strlen(fn) != size_t(colon - spec)) return false;
  std::lock_guard<std::mutex> lock(m);
  return ++calls[fn] == std::strtoull(colon + 1, nullptr, 10);
}
#define STUB_FAIL(fn) \
  if (fail_now(fn)) return hipErrorUnknown

// index of the dev::State argument of the kernels that publish the progress word, -1 for the others
int state_arg(const std::string &name) {
  for (const char *k : {"cn_minsum_kernel", "cn_minsum_lfree_kernel", "cn_minsum_rec_kernel", "cn_staged_kernel", "hl_level_kernel",
                        "hl_level_reg_kernel", "hl_minsum_kernel", "hl_minsum_reg_kernel", "hl_minsum_rec_kernel", "cn_i8_kernel",
                        "hl_i8_kernel", "hl_i8_reg_kernel"})
    if (name.find(k) != std::string::npos) return 2;  // (Graph, Sched, State, ...)
  if (name.find("compact_plan_kernel") != std::string::npos) return 0;
  return -1;
}

}  // namespace

extern "C" {

hipError_t hipGetDeviceCount(int *count) {
  *count = 1;
  return hipSuccess;
}
hipError_t hipSetDevice(int device) {
  if (trace_calls()) trace_line("setdevice " + std::to_string(device));
  STUB_FAIL("hipSetDevice");
  return hipSuccess;
}
hipError_t hipDeviceGetAttribute(int *value, hipDeviceAttribute_t attr, int) {
  *value = attr == hipDeviceAttributeMultiprocessorCount ? 256 : 0;
  return hipSuccess;
}
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int *blocks, const void *, int, size_t) {
  *blocks = 1;
  return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void *, hipFuncAttribute, int) { return hipSuccess; }
std::atomic<int> g_last_error{0};  // a failed kernel launch is reported by the next hipGetLastError, as in HIP
hipError_t hipGetLastError(void) {
  if (trace_calls()) trace_line("getlasterror");
  return static_cast<hipError_t>(g_last_error.exchange(0));
}
const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "injected by the HIP stub"; }

static hipError_t allocate(void **p, size_t bytes, const char *what, int live) {
  if (std::getenv("HIP_STUB_TRACE")) trace_line(std::string(what) + " " + std::to_string(bytes));
  *p = std::calloc(std::max<size_t>(bytes, 1), 1);
  if (!*p) return hipErrorOutOfMemory;
  g_live[live]++;
  return hipSuccess;
}
hipError_t hipMalloc(void **p, size_t bytes) {
  STUB_FAIL("hipMalloc");
  return allocate(p, bytes, "malloc", kLiveDevice);
}
hipError_t hipFree(void *p) {
  if (p) g_live[kLiveDevice]--;
  std::free(p);
  return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) {
  STUB_FAIL("hipHostMalloc");
  return allocate(p, bytes, "hostmalloc", kLivePinned);
}
hipError_t hipHostFree(void *p) {
  if (p) g_live[kLivePinned]--;
  std::free(p);
  return hipSuccess;
}
// (every pointer of the stand-in runtime is host memory: Simulator::generate then takes its copy-out path)
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *attr, const void *) {
  std::memset(attr, 0, sizeof(*attr));
  attr->type = hipMemoryTypeHost;
  return hipSuccess;
}
hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned int) {
  *dev = host;
  return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int) {
  STUB_FAIL("hipStreamCreateWithFlags");
  *s = reinterpret_cast<hipStream_t>(new Stream());
  g_live[kLiveStreams]++;
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  g_live[kLiveStreams]--;
  delete reinterpret_cast<Stream *>(s);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
  if (trace_calls()) trace_line("streamsync " + std::to_string(as_stream(s)->ordinal));
  as_stream(s)->sync();
  STUB_FAIL("hipStreamSynchronize");
  return hipSuccess;
}
hipError_t hipStreamQuery(hipStream_t s) { return as_stream(s)->busy() ? hipErrorNotReady : hipSuccess; }

hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned int) {
  STUB_FAIL("hipEventCreateWithFlags");
  *e = reinterpret_cast<hipEvent_t>(new Event());
  g_live[kLiveEvents]++;
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e) {
  g_live[kLiveEvents]--;
  delete reinterpret_cast<Event *>(e);
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t s) {
  if (trace_calls())
    trace_line("eventrecord " + std::to_string(reinterpret_cast<Event *>(ev)->ordinal) + " " + std::to_string(as_stream(s)->ordinal));
  STUB_FAIL("hipEventRecord");
  std::shared_ptr<EventState> e = reinterpret_cast<Event *>(ev)->st;
  uint64_t gen;
  {
    std::lock_guard<std::mutex> lock(e->m);
    gen = ++e->issued;
  }
  as_stream(s)->push([e, gen] {
    {
      std::lock_guard<std::mutex> lock(e->m);
      e->completed = std::max(e->completed, gen);
    }
    e->cv.notify_all();
  });
  return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t ev, unsigned int) {
  if (trace_calls())
    trace_line("streamwaitevent " + std::to_string(as_stream(s)->ordinal) + " " + std::to_string(reinterpret_cast<Event *>(ev)->ordinal));
  STUB_FAIL("hipStreamWaitEvent");
  std::shared_ptr<EventState> e = reinterpret_cast<Event *>(ev)->st;
  uint64_t target;
  {
    std::lock_guard<std::mutex> lock(e->m);
    target = e->issued;  // the record made last before this call (none: the wait is a no-op)
  }
  as_stream(s)->push([e, target] {
    std::unique_lock<std::mutex> lock(e->m);
    e->cv.wait(lock, [&] { return e->completed >= target; });
  });
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t ev) {
  std::shared_ptr<EventState> e = reinterpret_cast<Event *>(ev)->st;
  std::unique_lock<std::mutex> lock(e->m);
  e->cv.wait(lock, [&] { return e->completed >= e->issued; });
  return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) {
  *ms = 0.01f;
  return hipSuccess;
}

hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
  if (trace_calls()) {
    const char *k = kind == hipMemcpyHostToDevice ? "h2d" : kind == hipMemcpyDeviceToHost ? "d2h" : kind == hipMemcpyDeviceToDevice ? "d2d" : "other";
    trace_line(std::string("memcpyasync ") + k + " " + std::to_string(bytes) + " " + std::to_string(as_stream(s)->ordinal));
  }
  STUB_FAIL("hipMemcpyAsync");
  as_stream(s)->push([=] { std::memcpy(dst, src, bytes); });
  return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
  STUB_FAIL("hipMemcpy");
  default_stream()->sync();
  if (kind == hipMemcpyHostToDevice && std::getenv("HIP_STUB_TRACE")) {
    uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a
    for (size_t i = 0; i < bytes; i++) h = (h ^ static_cast<const unsigned char *>(src)[i]) * 0x100000001b3ull;
    char line[64];
    std::snprintf(line, sizeof(line), "h2d %zu %016llx", bytes, static_cast<unsigned long long>(h));
    trace_line(line);
  }
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t s) {
  if (trace_calls()) trace_line("memsetasync " + std::to_string(bytes) + " " + std::to_string(as_stream(s)->ordinal));
  as_stream(s)->push([=] { std::memset(dst, value, bytes); });
  return hipSuccess;
}

hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t stream) {
  t_config = LaunchConfig{grid, block, shmem, stream};
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *shmem, hipStream_t *stream) {
  *grid = t_config.grid;
  *block = t_config.block;
  *shmem = t_config.shmem;
  *stream = t_config.stream;
  return hipSuccess;
}
void **__hipRegisterFatBinary(const void *) {
  static void *handle = nullptr;
  return &handle;
}
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host_fun, char *, const char *device_name, unsigned int, void *, void *, void *,
                           void *, int *) {
  std::lock_guard<std::mutex> lock(g_reg_mutex);
  kernel_names()[host_fun] = device_name;
}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}

hipError_t hipLaunchKernel(const void *fun, dim3 grid, dim3 block, void **args, size_t shmem, hipStream_t s) {
  if (fail_now("hipLaunchKernel")) {
    g_last_error = static_cast<int>(hipErrorUnknown);
    return hipErrorUnknown;
  }
  g_launches++;
  int at = -1;
  {
    std::lock_guard<std::mutex> lock(g_reg_mutex);
    auto it = kernel_names().find(fun);
    if (it != kernel_names().end()) {
      at = state_arg(it->second);
      if (std::getenv("HIP_STUB_TRACE")) {
        char geometry[128];
        std::snprintf(geometry, sizeof(geometry), "%u grid %u %u %u block %u %u %u lds %zu ", as_stream(s)->ordinal, grid.x, grid.y,
                      grid.z, block.x, block.y, block.z, shmem);
        trace_line(geometry + demangled(it->second));
      }
    }
  }
  if (at < 0) {
    as_stream(s)->push([] {});
    return hipSuccess;
  }
  const ldpc::dev_for_the_stub::State st = *static_cast<const ldpc::dev_for_the_stub::State *>(args[at]);  // (args live on the caller's stack)
  static const unsigned long done_at = std::getenv("HIP_STUB_DONE_AT") ? std::strtoul(std::getenv("HIP_STUB_DONE_AT"), nullptr, 10) : ~0ul;
  as_stream(s)->push([st] {
    if (st.publish != nullptr) {
      const uint32_t running = st.tick >= done_at ? 0u : 1u;
      __atomic_store_n(st.publish, ldpc::dev_for_the_stub::progress_word(st.epoch, st.tick, running), __ATOMIC_RELEASE);
    }
  });
  return hipSuccess;
}

unsigned long long hip_stub_launches(void) { return g_launches.load(); }
void hip_stub_live(long long counts[4]) {
  for (int i = 0; i < 4; i++) counts[i] = g_live[i].load();
}
void hip_stub_trace_note(const char *text) { trace_line(std::string("# ") + text); }

}  // extern "C"
