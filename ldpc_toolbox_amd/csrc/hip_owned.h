// Owners of what the HIP runtime hands out: device memory, pinned host memory, streams and events.  Move-only; each frees
// what it holds when it goes.  A handle's members are declared streams first, so that they are destroyed after every
// buffer and event ("Ownership").
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace ldpc {

namespace owned {
// one raw handle and the call that gives it back
template <typename H, hipError_t (*Release)(H)>
class Handle {
 public:
  Handle() = default;
  Handle(Handle &&o) noexcept : h_(std::exchange(o.h_, H{})) {}
  Handle &operator=(Handle &&o) noexcept {
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, H{});
    }
    return *this;
  }
  ~Handle() { reset(); }
  void reset() {
    if (h_) (void)Release(h_);
    h_ = H{};
  }
  explicit operator bool() const { return h_ != H{}; }

 protected:
  H h_{};
};

// memory with the size its owner last asked for
template <hipError_t (*Release)(void *)>
class Memory : public Handle<void *, Release> {
 public:
  Memory() = default;
  Memory(Memory &&o) noexcept : Handle<void *, Release>(std::move(o)), cap_(std::exchange(o.cap_, 0)) {}
  Memory &operator=(Memory &&o) noexcept {
    if (this != &o) {
      Handle<void *, Release>::operator=(std::move(o));
      cap_ = std::exchange(o.cap_, 0);
    }
    return *this;
  }
  template <typename T = void>
  T *get() const {
    return static_cast<T *>(this->h_);
  }
  size_t capacity() const { return cap_; }

 protected:
  size_t cap_ = 0;
};
}  // namespace owned

class DeviceBuffer : public owned::Memory<hipFree> {
 public:
  // Keeps the buffer when its capacity suffices; else frees it and allocates max(bytes, floor) anew -- the contents are
  // not preserved -- and records `bytes` as the capacity.
  hipError_t ensure(size_t bytes, size_t floor = 0) {
    if (cap_ >= bytes) return hipSuccess;
    reset();
    cap_ = 0;
    const hipError_t e = hipMalloc(&h_, std::max(bytes, floor));
    if (e == hipSuccess) cap_ = bytes;
    return e;
  }
};

class PinnedBuffer : public owned::Memory<hipHostFree> {
 public:
  // The same for pinned host memory, in whole granules and never more than `cap` bytes; the capacity is what was allocated.
  hipError_t ensure(size_t need, size_t granule, size_t cap = SIZE_MAX, unsigned flags = hipHostMallocDefault) {
    if (cap_ >= need) return hipSuccess;
    reset();
    cap_ = 0;
    const size_t bytes = std::min(cap, (need + granule - 1) / granule * granule);
    const hipError_t e = hipHostMalloc(&h_, bytes, flags);
    if (e == hipSuccess) cap_ = bytes;
    return e;
  }
};

class Stream : public owned::Handle<hipStream_t, hipStreamDestroy> {
 public:
  hipError_t create() { return hipStreamCreateWithFlags(&h_, hipStreamNonBlocking); }
  operator hipStream_t() const { return h_; }
};

class Event : public owned::Handle<hipEvent_t, hipEventDestroy> {
 public:
  hipError_t create(unsigned flags = hipEventDisableTiming) { return hipEventCreateWithFlags(&h_, flags); }
  operator hipEvent_t() const { return h_; }
};

// a vector's elements in device memory (at least one element's worth for an empty vector); on failure *e says why
template <typename T>
DeviceBuffer upload(const std::vector<T> &v, hipError_t *e, size_t floor = 0) {
  DeviceBuffer b;
  *e = b.ensure(std::max<size_t>(v.size(), 1) * sizeof(T), floor);
  if (*e == hipSuccess && !v.empty()) *e = hipMemcpy(b.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  return b;
}

}  // namespace ldpc
