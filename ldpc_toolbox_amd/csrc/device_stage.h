// What the stage handles beside the decoder share (DeviceDemodulator, DeviceEncoder, DeviceBch, DeviceNrRm, DeviceNrTb,
// DeviceNrQam): the device, the handle's stream with the event that orders it after the legacy default stream, the last
// error, the protocol of a _device entry (begin / end) and the staging loop of a _host entry.  Host only.
// A handle derives from DeviceStage, so its own buffers and events are destroyed before the stream here (DESIGN.md,
// "Ownership") -- and its destructor calls wait_idle() first: this base's destructor runs after the handle's members are
// gone, too late to wait for the launches that still use them.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <utility>

#include "hip_owned.h"

namespace ldpc {

// inside a member of a stage handle: -2 with the failed expression as the handle's last error
#define STAGE_TRY(expr)               \
  do {                                \
    hipError_t _e = (expr);           \
    if (_e != hipSuccess) {           \
      fail(#expr, _e);                \
      return -2;                      \
    }                                 \
  } while (0)

// A run-time small integer as a compile-time one, for the template arguments of a launch: fn(std::integral_constant<int,
// V>{}) for the V of the list that equals v -- for the last V of the list when none does.  with_bool: the same for a flag.
template <int V, int... Rest, typename F>
void with_int(int v, F &&fn) {
  if constexpr (sizeof...(Rest) == 0) {
    fn(std::integral_constant<int, V>{});
  } else {
    if (v == V) return fn(std::integral_constant<int, V>{});
    with_int<Rest...>(v, std::forward<F>(fn));
  }
}
template <typename F>
void with_bool(bool v, F &&fn) {
  if (v)
    fn(std::true_type{});
  else
    fn(std::false_type{});
}

class DeviceStage {
 public:
  DeviceStage(const DeviceStage &) = delete;
  DeviceStage &operator=(const DeviceStage &) = delete;

  int device() const { return device_; }
  const std::string &last_error() const { return error_; }

 protected:
  // prefix: the handle's word in the stderr line of fail()
  DeviceStage(const char *prefix, int device) : prefix_(prefix), device_(device) {}
  ~DeviceStage() = default;

  // The opening of a create(): is `device` a usable GPU?  Selects it.  who: "the rate matcher has", for the message.
  static bool select_device(int device, const char *who, std::string *err) {
    auto bail = [&](const std::string &m) {
      if (err) *err = m;
      return false;
    };
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return bail(std::string("no HIP device available: ") + who + " no CPU path");
    if (device < 0 || device >= count) return bail("HIP device index out of range");
    if (hipSetDevice(device) != hipSuccess) return bail("hipSetDevice failed");
    return true;
  }
  // the stream, the default-stream event and then the handle's further events
  hipError_t create_stream(std::initializer_list<Event *> more = {}) {
    hipError_t e = stream_.create();
    if (e == hipSuccess) e = ev_default_.create();
    for (Event *ev : more)
      if (e == hipSuccess) e = ev->create();
    return e;
  }
  // ... with the message of a create() that fails there; whose: "the rate matcher's"
  bool create_stream(const char *whose, std::string *err, std::initializer_list<Event *> more = {}) {
    if (create_stream(more) == hipSuccess) return true;
    if (err) *err = std::string("creating ") + whose + " stream failed";
    return false;
  }
  // first in the handle's destructor: nothing on the handle's stream uses a member any more
  void wait_idle() {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
  }

  bool fail(const std::string &m, hipError_t e = hipSuccess) {
    error_ = m;
    if (e != hipSuccess) error_ += std::string(": ") + hipGetErrorString(e);
    std::fprintf(stderr, "ldpc_toolbox (hip): %s: %s\n", prefix_, error_.c_str());
    return false;
  }

  // A _device entry: *s = the launch stream -- the caller's, or (nullptr) the handle's own, ordered after everything the
  // legacy default stream holds now and synchronised by end().  0, or -2.
  int begin(hipStream_t stream, hipStream_t *s) {
    STAGE_TRY(hipSetDevice(device_));
    *s = stream ? stream : static_cast<hipStream_t>(stream_);
    if (!stream) {
      // (the handle's stream is non-blocking: ordered explicitly after what the legacy default stream holds now)
      STAGE_TRY(hipEventRecord(ev_default_, nullptr));
      STAGE_TRY(hipStreamWaitEvent(*s, ev_default_, 0));
    }
    return 0;
  }
  int end(hipStream_t stream, hipStream_t s) {
    STAGE_TRY(hipGetLastError());
    return finish(stream, s);
  }
  // (end()'s second half, for a handle with a step of its own between the two)
  int finish(hipStream_t stream, hipStream_t s) {
    if (!stream) STAGE_TRY(hipStreamSynchronize(s));
    return 0;
  }

  // A _host entry: `batch` frames in stages of at most `stage`.  Each buffer is made to hold `stage` rows of its row_bytes;
  // then body(first frame, frames) per stage -- its copies and its _device entry, all on stream_ -- and the wait for the
  // stream: the next stage overwrites the buffers this one reads.  A failure in a later stage leaves the earlier ones done.
  struct Rows {
    DeviceBuffer &buffer;
    size_t row_bytes;
  };
  template <typename F>
  int staged(size_t batch, size_t stage, std::initializer_list<Rows> buffers, F body) {
    STAGE_TRY(hipSetDevice(device_));
    for (const Rows &r : buffers) STAGE_TRY(r.buffer.ensure(stage * r.row_bytes, 256));
    for (size_t b0 = 0; b0 < batch; b0 += stage) {
      const size_t frames = std::min(stage, batch - b0);
      if (int rc = body(b0, frames)) return rc;
      STAGE_TRY(hipStreamSynchronize(stream_));
    }
    return 0;
  }
  // Dense rows: in [batch][in_row bytes] -> d_in_, body(frames) from d_in_ to d_out_, d_out_ -> out [batch][out_row bytes].
  // preload: the rows of `out` go to d_out_ first (a body that combines into them).  The copy out is the only write to the
  // caller's buffer: after a failure before it nothing of the stage has been written.
  template <typename F>
  int staged_rows(const void *in, size_t in_row, void *out, size_t out_row, size_t batch, size_t stage, bool preload, F body) {
    const char *src = static_cast<const char *>(in);
    char *dst = static_cast<char *>(out);
    return staged(batch, stage, {{d_in_, in_row}, {d_out_, out_row}}, [&](size_t b0, size_t frames) {
      if (in_row > 0) STAGE_TRY(hipMemcpyAsync(d_in_.get(), src + b0 * in_row, frames * in_row, hipMemcpyHostToDevice, stream_));
      if (preload) STAGE_TRY(hipMemcpyAsync(d_out_.get(), dst + b0 * out_row, frames * out_row, hipMemcpyHostToDevice, stream_));
      if (int rc = body(frames)) return rc;
      if (out_row > 0) STAGE_TRY(hipMemcpyAsync(dst + b0 * out_row, d_out_.get(), frames * out_row, hipMemcpyDeviceToHost, stream_));
      return 0;
    });
  }

  const char *const prefix_;
  int device_;
  std::string error_;
  // what every handle owns (hip_owned.h): the stream is declared first and so destroyed last, after the derived handle's members
  Stream stream_;
  Event ev_default_;
  DeviceBuffer d_in_, d_out_;  // the staging buffers of the host entries
};

}  // namespace ldpc
