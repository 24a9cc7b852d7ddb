// cv::RNG and the pieces of OpenCV 4.4's RANSACPointSetRegistrator that every RANSAC kernel of
// the library shares (pnp.hip, detector.hip): the multiply-with-carry stream, its jump-ahead
//  and RANSACUpdateNumIters.
#pragma once

#include "common.h"

namespace onepose {

// cv::RNG (multiply-with-carry): state' = (state & 0xffffffff) * kMwcA + (state >> 32)
constexpr unsigned long long kMwcA = 4164903690ull;
constexpr unsigned long long kMwcM = kMwcA * 4294967296ull - 1ull;   // < 2^64

constexpr unsigned long long mwc_mulmod_c(unsigned long long a, unsigned long long b) {
  return (unsigned long long)((unsigned __int128)a * b % kMwcM);
}
// A^(STEP l) mod kMwcM, l = 0..63 (compile time): lane l's start when every lane of a wave
// takes STEP consecutive draws
template <int STEP>
struct MwcJumps {
  unsigned long long v[64];
  constexpr MwcJumps() : v() {
    unsigned long long as = 1ull;
    for (int i = 0; i < STEP; ++i) as = mwc_mulmod_c(as, kMwcA);
    unsigned long long x = 1ull;
    for (int l = 0; l < 64; ++l) {
      v[l] = x;
      x = mwc_mulmod_c(x, as);
    }
  }
};

__device__ __forceinline__ unsigned rng_next(unsigned long long& s) {
  s = (unsigned long long)(unsigned)s * 4164903690ull + (unsigned)(s >> 32);
  return (unsigned)s;
}

// cv::RNG is a lag-1 multiply-with-carry generator: for a state z = c * 2^32 + x below
// m = A * 2^32 - 1, the next state A x + c equals A z mod m (A 2^32 = 1 mod m), so the state
// k draws ahead is A^k z mod m -- lane l of a wave starts its STEP draws at A^(STEP l) z.
__device__ __forceinline__ unsigned long long mwc_mulmod(unsigned long long a,
                                                         unsigned long long b) {
  // a b mod m for a, b < m: fold the high word with 2^64 = r (mod m), r = (2^32 - A) 2^32 + 1
  constexpr unsigned long long r = ((4294967296ull - kMwcA) << 32) | 1ull;
  unsigned long long lo = a * b, hi = __umul64hi(a, b);
  while (hi != 0ull) {
    const unsigned long long l2 = hi * r, h2 = __umul64hi(hi, r);
    lo += l2;
    hi = h2 + (lo < l2 ? 1ull : 0ull);
  }
  return lo >= kMwcM ? lo - kMwcM : lo;
}

// RANSACUpdateNumIters (ptsetreg.cpp)
__device__ __forceinline__ int update_num_iters(double p, double ep, int model_points, int max_iters) {
  p = fmin(fmax(p, 0.0), 1.0);
  ep = fmin(fmax(ep, 0.0), 1.0);
  double num = fmax(1. - p, 2.2250738585072014e-308);
  double denom = 1. - pow(1. - ep, (double)model_points);
  if (denom < 2.2250738585072014e-308) return 0;
  num = log(num);
  denom = log(denom);
  return (denom >= 0 || -num >= max_iters * (-denom)) ? max_iters : __double2int_rn(num / denom);
}

}  // namespace onepose
