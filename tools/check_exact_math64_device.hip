// Device-side check of the double-precision half of csrc/exact_math.h: exp, log, log1p, expm1, tanh, phi and the three
// compositions the f64 kernels form, evaluated ON THE GPU (gfx950) on the argument set of tests/exact_math64_cases.h --
// every double within 4096 ulps of each class boundary plus 2^26 seeded random arguments per function -- and compared, bit
// for bit, with the host's glibc AND with the host build of the same header (all NaNs count as equal).  A difference from
// the host build alone is device code generation (fmax with a NaN, the saturating double -> int32 conversion, the f64
// division sequence, fma, subnormal results, the select forms that evaluate every class for every lane); a difference of
// both builds from glibc is another libm generation (tests/test_libm_contract.py).
// tools/check_exact_math_device.hip is the f32 counterpart, exhaustive over all 2^32 floats.
//   hipcc -O3 -std=c++17 -ffp-contract=off -fno-fast-math --offload-arch=gfx950 -pthread tools/check_exact_math64_device.hip -o tools/mb/check_device64
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <vector>
#include "../tests/exact_math64_cases.h"
using namespace ldpc;

__global__ void eval_kernel(int f, const double *edge, uint64_t base, uint64_t count, uint64_t *out) {
  const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < count) out[i] = em::as_u64(em64::mine(f, em64::arg(f, edge, base + i)));
}

#define HIP_OK(call)                                                            \
  do {                                                                          \
    const hipError_t e_ = (call);                                               \
    if (e_ != hipSuccess) {                                                     \
      fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                \
      return 2;                                                                 \
    }                                                                           \
  } while (0)

int main(int argc, char **argv) {
  const uint64_t chunk = 1ull << 24;
  const std::vector<double> edge = em64::edges();
  if (edge.size() != em64::kEdges) {
    fprintf(stderr, "%zu edges, expected %zu\n", edge.size(), em64::kEdges);
    return 2;
  }
  double *d_edge;
  uint64_t *d_out;
  HIP_OK(hipMalloc(&d_edge, edge.size() * sizeof(double)));
  HIP_OK(hipMemcpy(d_edge, edge.data(), edge.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_OK(hipMalloc(&d_out, chunk * sizeof(uint64_t)));
  hipEvent_t start, stop;
  HIP_OK(hipEventCreate(&start));
  HIP_OK(hipEventCreate(&stop));
  std::vector<uint64_t> got(chunk);
  const unsigned nthreads = std::min(std::max(1u, std::thread::hardware_concurrency()), 16u);
  const uint64_t total = em64::kCountPerFunction;
  int bad_functions = 0;
  double device_ms = 0.0;
  const auto wall0 = std::chrono::steady_clock::now();
  for (int f = 0; f < em64::kCount; f++) {
    if (argc > 1 && strcmp(em64::name(f), argv[1]) != 0) continue;
    std::atomic<unsigned long long> bad_glibc{0}, bad_host{0};
    std::atomic<uint64_t> first_bad{~0ull};
    for (uint64_t base = 0; base < total; base += chunk) {
      const uint64_t count = std::min(chunk, total - base);
      HIP_OK(hipEventRecord(start, 0));
      eval_kernel<<<dim3(unsigned((count + 255) / 256)), dim3(256)>>>(f, d_edge, base, count, d_out);
      HIP_OK(hipGetLastError());
      HIP_OK(hipEventRecord(stop, 0));
      HIP_OK(hipMemcpy(got.data(), d_out, count * sizeof(uint64_t), hipMemcpyDeviceToHost));
      float ms = 0.0f;
      HIP_OK(hipEventElapsedTime(&ms, start, stop));
      device_ms += ms;
      std::vector<std::thread> th;
      for (unsigned t = 0; t < nthreads; t++)
        th.emplace_back([&, t] {
          unsigned long long lg = 0, lh = 0;
          for (uint64_t i = t; i < count; i += nthreads) {
            const double x = em64::arg(f, edge.data(), base + i), have = em::as_f64(got[i]);
            const bool g = !em64::same(have, em64::glibc(f, x)), h = !em64::same(have, em64::mine(f, x));
            if (g || h) {
              uint64_t seen = first_bad.load();
              while (base + i < seen && !first_bad.compare_exchange_weak(seen, base + i)) {
              }
            }
            lg += g;
            lh += h;
          }
          bad_glibc += lg;
          bad_host += lh;
        });
      for (auto &x : th) x.join();
    }
    printf("%-22s %llu arguments: %llu mismatches vs glibc, %llu mismatches vs the host build", em64::name(f),
           static_cast<unsigned long long>(total), bad_glibc.load(), bad_host.load());
    if (bad_glibc.load() || bad_host.load()) {
      // (the device value of one argument, again: a one-thread launch)
      const uint64_t i = first_bad.load();
      const double x = em64::arg(f, edge.data(), i);
      eval_kernel<<<dim3(1), dim3(1)>>>(f, d_edge, i, 1, d_out);
      uint64_t bits = 0;
      HIP_OK(hipMemcpy(&bits, d_out, sizeof bits, hipMemcpyDeviceToHost));
      printf("   first at x=%a (argument %llu): device %a glibc %a host build %a", x, static_cast<unsigned long long>(i),
             em::as_f64(bits), em64::glibc(f, x), em64::mine(f, x));
      bad_functions++;
    }
    printf("\n");
    fflush(stdout);
  }
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count();
  printf("device kernels %.1f ms in all, %.1f s with the copies and the host comparison on %u threads\n", device_ms, wall, nthreads);
  return bad_functions ? 1 : 0;
}
