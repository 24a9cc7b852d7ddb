// What the library's RANSAC kernels share (pnp.hip, detector.hip): cv::RNG as a
// multiply-with-carry stream with its jump-ahead, and the scaffold of OpenCV
// 4.4's RANSACPointSetRegistrator loop replayed 64 iterations per round by one workgroup of
// 256 threads -- a round's draws, the per-hypothesis inlier count, the acceptance rule in
// iteration order -- plus the block-wide compaction that frame_ops.hip's select_kernel uses too.
// Device-only pieces the kernel bodies call; how subsets are dealt and models solved stays there.
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
template <int STEP>
__constant__ const MwcJumps<STEP> kMwcJumps = MwcJumps<STEP>();

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

// One trip of a block-wide compaction in ascending thread order, by every thread of a
// workgroup of WAVES waves: the slot of this thread's element (meaningful where `valid`).
// `base` is the count of the earlier trips, advanced by this trip's in every thread.
// wave_cnt: WAVES ints of LDS; two barriers, so the caller stores after the second.
template <int WAVES>
__device__ __forceinline__ int compact_step(bool valid, int* wave_cnt, int& base) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(valid);
  if (lane == 0) wave_cnt[wave] = __popcll(bal);
  __syncthreads();
  int off = base;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const int c = wave_cnt[w];
    if (w < wave) off += c;
    base += c;
  }
  __syncthreads();
  return off + __popcll(bal & ((1ull << lane) - 1ull));
}

// The loop's state, in LDS: OpenCV's iteration counter, niters, the best inlier count, the
// stop flag and the cv::RNG state at the round's start.
struct RansacCtl {
  unsigned long long rng;
  int iter, niters, max_good, done;
};
// By one thread, before a barrier.  cv::RNG((uint64)-1), as RANSACPointSetRegistrator::run.
__device__ __forceinline__ void ransac_ctl_init(RansacCtl& c, int max_iters, bool done) {
  c.iter = 0;
  c.niters = max(max_iters, 1);
  c.max_good = 0;
  c.done = done ? 1 : 0;
  c.rng = 0xFFFFFFFFFFFFFFFFull;
}

// A round's generated draws: the state after each and the draw % n, STEP per lane of one wave
// after up to kRngPrefix stepped one by one.
constexpr int kRngPrefix = 8;
template <int STEP>
struct RansacDraws {
  static constexpr int kPos = kRngPrefix + STEP * 64;
  unsigned long long rst[kPos];
  int rii[kPos];
  unsigned long long rz;
  int rk, rP;
};
// By every lane of one wave: generates the round's draws from ctl.rng by jump-ahead (states at
// or above m -- the first draws from RNG((uint64)-1) -- are stepped by lane 0 first) and
// returns their number P (also in d.rP; a stream still above m after the prefix gives only
// the prefix).  The wave's own later reads of d need a wave_lds_sync, other waves' a barrier.
template <int STEP>
__device__ __forceinline__ int ransac_round_draws(RansacDraws<STEP>& d, const RansacCtl& ctl, int n) {
  const int lane = threadIdx.x & 63;
  if (lane == 0) {
    unsigned long long z = ctl.rng;
    int k = 0;
    while (z >= kMwcM && k < kRngPrefix) {
      const unsigned v = rng_next(z);
      d.rst[k] = z;
      d.rii[k] = (int)(v % (unsigned)n);
      ++k;
    }
    d.rk = k;
    d.rz = z;
  }
  wave_lds_sync();
  const int k = d.rk;
  const unsigned long long z0 = d.rz;
  if (z0 < kMwcM) {
    unsigned long long z = mwc_mulmod(z0, kMwcJumps<STEP>.v[lane]);
#pragma unroll
    for (int i = 0; i < STEP; ++i) {
      const unsigned v = rng_next(z);
      d.rst[k + STEP * lane + i] = z;
      d.rii[k + STEP * lane + i] = (int)(v % (unsigned)n);
    }
  }
  const int P = z0 < kMwcM ? k + STEP * 64 : k;
  if (lane == 0) d.rP = P;
  return P;
}

// By every lane of one wave: how many of i = first, first + stride, ... below n satisfy in(i).
template <class Pred>
__device__ __forceinline__ int wave_count_if(int first, int n, int stride, Pred in) {
  int c = 0;
  for (int i = first; i < n; i += stride) c += in(i) ? 1 : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
  return c;
}

// OpenCV's acceptance rule over hypotheses [h_begin, h_end) in iteration order, by one thread:
// goodCount > max(best, model_points - 1) makes hypothesis h the best (on_best(h) copies its
// model) and shortens niters; iterations at or past niters are not looked at.
template <class OnBest>
__device__ __forceinline__ void ransac_accept(RansacCtl& ctl, const int* counts, int h_begin,
                                              int h_end, int n, double confidence,
                                              int model_points, OnBest on_best) {
  int iter = ctl.iter, niters = ctl.niters, best = ctl.max_good;
  for (int h = h_begin; h < h_end && iter < niters; ++h, ++iter) {
    const int good = counts[h];
    if (good > max(best, model_points - 1)) {
      best = good;
      on_best(h);
      niters = update_num_iters(confidence, (double)(n - good) / n, model_points, niters);
    }
  }
  ctl.iter = iter;
  ctl.niters = niters;
  ctl.max_good = best;
  ctl.done = iter >= niters;
}

}  // namespace onepose
