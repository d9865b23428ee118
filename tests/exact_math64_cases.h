// The double-precision half of ldpc_toolbox_amd/csrc/exact_math.h on a fixed argument set: the function list and the
// arguments of tests/test_exact_math.py's f64 checks, for the host (g++, against glibc) and for the device
// (tools/check_exact_math64_device.hip evaluates the same list on the same arguments in a HIP kernel).  Plain C++: every
// argument is a pure function of (function, index), so host and device name the same double by the same number and no
// argument array travels.  Needs -ffp-contract=off, as the header under test does.
//
//   set (a)  every double within +-4096 ulps of each class boundary of the routines, both signs of the boundary
//            (tools/check_exact_math64.cpp's edges, the Tanh rule's clamp and phi's / tanh's / expm1's further thresholds,
//            the 128 bucket starts of log's table): 2731 edges x 2 signs x 8193 neighbours = 44 750 166 arguments
//   set (b)  2^26 seeded random arguments over the eight classes of tools/check_exact_math64.cpp (any bit pattern twice,
//            [-32, 32), [-800, 0], [0, 1), near 1, 2^-60..2^9 with either sign, (-1, 1)); for phi every other block of
//            eight draws instead from its positive log-scale class 2^-120..2^7 and around 2 * {1, 19.4, 22}
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../ldpc_toolbox_amd/csrc/exact_math.h"

namespace em64 {

enum { kExp, kLog, kLog1p, kExpm1, kTanh, kPhi, kCorr, kAtanh, kTanhClamped, kCount };

inline const char *name(int f) {
  static const char *const names[kCount] = {"exp", "log", "log1p", "expm1", "tanh", "phi", "log1p(exp(-|x|))",
                                            "0.5*log1p(2x/(1-x))", "tanh(clamp(x,-18,18))"};
  return names[f];
}

// the header under test (host or device code, whichever this is compiled as)
EM_FN double mine(int f, double x) {
  namespace em = ldpc::em;
  switch (f) {
    case kExp: return em::exp(x);
    case kLog: return em::log(x);
    case kLog1p: return em::log1p(x);
    case kExpm1: return em::expm1(x);
    case kTanh: return em::tanh(x);
    case kPhi: return em::phi(x);
    // kernels_common.hip.h:212  `double m_corr(double a) { return m_log1p(m_exp(-a)); }`, a = |x|
    case kCorr: return em::log1p(em::exp(-__builtin_fabs(x)));
    // kernels_common.hip.h:287  `double atanh_rs(double x) { return 0.5 * m_log1p((2.0 * x) / (1.0 - x)); }`
    case kAtanh: return 0.5 * em::log1p((2.0 * x) / (1.0 - x));
    // kernels_common.hip.h:284  `double m_tanh_clamped(double x) { return m_tanh(x); }` behind the clamp of :413-417
    // (`if (h < -c) h = -c; if (h > c) h = c;`, c = 18: a NaN stays a NaN)
    default: return em::tanh(x < -18.0 ? -18.0 : (x > 18.0 ? 18.0 : x));
  }
}

// the same list on the host libm
inline double glibc(int f, double x) {
  switch (f) {
    case kExp: return ::exp(x);
    case kLog: return ::log(x);
    case kLog1p: return ::log1p(x);
    case kExpm1: return ::expm1(x);
    case kTanh: return ::tanh(x);
    case kPhi: return -(::log(::tanh(0.5 * ::fmax(x, 1e-30))));
    case kCorr: return ::log1p(::exp(-::fabs(x)));
    case kAtanh: return 0.5 * ::log1p((2.0 * x) / (1.0 - x));
    default: return ::tanh(x < -18.0 ? -18.0 : (x > 18.0 ? 18.0 : x));
  }
}

// bit equality; all NaNs count as equal
EM_FN bool same(double a, double b) { return ldpc::em::as_u64(a) == ldpc::em::as_u64(b) || (a != a && b != b); }

// ---- set (a) ---------------------------------------------------------------------------------------------------------------
constexpr int kUlps = 4096;
constexpr uint64_t kPerEdge = 2ull * (2 * kUlps + 1);
constexpr size_t kEdges = 2731;
constexpr uint64_t kBoundaryCount = kEdges * kPerEdge;   // 44 750 166

inline std::vector<double> edges() {
  // tools/check_exact_math64.cpp:89-105
  std::vector<double> e = {0.0, 0x1p-54, 0x1p-55, 0x1p-29, 0x1p-28, 0x1p-20, 0.41421356237309503, -0.29289321881345248, 1.0, -1.0,
                           2.0, 22.0, 0x1p53, 709.782712893384, -745.13321910194111, 0x1p-1022, 0.5, 0.25, -0.25,
                           1.4142135623730951, 0.70710678118654757, 2.8284271247461903, 0.41421356237309515 * 2 + 1};
  for (double hb : {0x1p-55, 1.0, 22.0, 19.407, 1.7166400194, 0.5 * 0.34657359027997264, 0.5 * 1.0397207708399179})
    e.push_back(2.0 * hb);                               // phi: the classes of tanh(x / 2), expm1 and log under it
  e.push_back(1e-30);
  e.push_back(2e-30);
  for (int k = 1; k <= 1100; k++) {
    e.push_back((k - 0.5) * 0.69314718055994529);        // rounding boundary of k = round(x / ln2)
    e.push_back(k * 0.69314718055994529);
  }
  for (int p = -60; p <= 60; p++) {                      // 1 + x crossing sqrt(2) * 2^p, and powers of two
    e.push_back(ldexp(1.4142135623730951, p) - 1.0);
    e.push_back(ldexp(1.0, p) - 1.0);
    e.push_back(ldexp(1.0, p));
  }
  // the Tanh rule's clamp (18) and twice it, phi's h >= 19.4 class (its select of expm1's k > 56 formula) as h, x = 2h and
  // 2x, tanh's saturation as x = 2 * 22, ln(2^-1022) where exp's results turn subnormal, 0.9375 where log's "close to 1" window begins and
  // 1.06464 just inside its upper end (1 + 0x1.09p-4)
  for (double x : {18.0, 36.0, 38.8, 44.0, -708.39641853226408, 0.9375, 1.06464, 19.4}) e.push_back(x);
  for (uint64_t i = 0; i < 128; i++) e.push_back(ldpc::em::as_f64(0x3fe6000000000000ull + (i << 45)));   // log's table buckets
  return e;
}

// argument i of set (a), i < kBoundaryCount: edge i / kPerEdge, then its sign, then the neighbour -4096..4096 (in bit
// patterns: around +-0.0 the far side is the NaNs of the other end, which every function must also agree on)
EM_FN double boundary_arg(const double *edge, uint64_t i) {
  const uint64_t rem = i % kPerEdge;
  const double c = edge[i / kPerEdge];
  const uint64_t centre = ldpc::em::as_u64(rem / (2 * kUlps + 1) ? -c : c);
  return ldpc::em::as_f64(centre + (rem % (2 * kUlps + 1)) - uint64_t(kUlps));
}

// ---- set (b) ---------------------------------------------------------------------------------------------------------------
constexpr uint64_t kRandomCount = 1ull << 26;

EM_FN uint64_t mix(uint64_t z) {   // splitmix64's output function on a counter
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// argument i of set (b) for function f: the classes of tools/check_exact_math64.cpp:53-66
EM_FN double random_arg(int f, uint64_t i) {
  namespace em = ldpc::em;
  const uint64_t r = mix((i + 1) * 0x9E3779B97F4A7C15ull + uint64_t(f) * 0xD1B54A32D192ED03ull);
  const double u = static_cast<double>(r >> 11) * 0x1p-53;                         // [0, 1)
  const double s = static_cast<double>(static_cast<int64_t>(r >> 11)) * 0x1p-53;   // the same, as the tool writes it
  if (f == kPhi && (i & 8)) {
    if ((i & 0x30) == 0x30) return 2.0 * ((i & 0x40) ? 19.4 : ((i & 0x80) ? 22.0 : 1.0)) + (s - 0.5) * 0.01;
    return em::as_f64((r & 0x000fffffffffffffull) | ((0x3ffull - 120 + (r >> 52) % 128) << 52));   // 2^-120 .. 2^7
  }
  switch (i & 7) {
    case 0: case 1: return em::as_f64(r);                                          // any bit pattern
    case 2: return s * 64.0 - 32.0;                                                // [-32, 32)
    case 3: return -u * 800.0;                                                     // [-800, 0]
    case 4: return u;                                                              // [0, 1)
    case 5: return 1.0 + (s - 0.5) * 0.25;                                         // near 1
    case 6: return em::as_f64((r & 0x800fffffffffffffull) | ((0x3ffull - 60 + (r >> 52) % 70) << 52));   // 2^-60 .. 2^9
    default: return (s - 0.5) * 2.0;                                               // (-1, 1)
  }
}

constexpr uint64_t kCountPerFunction = kBoundaryCount + kRandomCount;   // 111 859 030

// argument i of the whole set: (a), then (b)
EM_FN double arg(int f, const double *edge, uint64_t i) {
  return i < kBoundaryCount ? boundary_arg(edge, i) : random_arg(f, i - kBoundaryCount);
}

}  // namespace em64
