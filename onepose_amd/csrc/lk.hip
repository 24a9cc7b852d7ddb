// Pyramidal Lucas-Kanade optical flow (the tracker's kpt_flow_track, src/tracker/ba_tracker.py
// :113-126, cv2.calcOpticalFlowPyrLK).  The arithmetic contract is stated in
// include/onepose_hip.h; tests/lk_oracle.py restates it in numpy and the GPU tests ask for
// bit-equality, so every float step below is a separate fp32 operation in the order written.
//
//   lk_pyr_head_kernel   level 0 (a copy of the image), its Scharr derivative, level 1
//   lk_pyr_tail_kernel   levels >= 1: derivative of level l and level l + 1, one workgroup per
//                        image, a workgroup barrier between levels
//   lk_pyr_level_kernel  the same one level at a time across the grid, above 1024 x 1024 pixels
//   lk_track_kernel      one wave per point, four points per workgroup; the window's I, Ix, Iy in
//                        registers for a whole level, the five sums as exact integers reduced with
//                        cross-lane shuffles.  No LDS, no atomics, nothing between workgroups.
#include <float.h>

#include "common.h"

#pragma STDC FP_CONTRACT OFF

namespace onepose {
namespace {

constexpr int kLkMaxLevels = 6;   // max_level <= 5
constexpr int kLkMinWin = 3, kLkMaxWin = 31, kLkMaxDim = 8192, kLkMaxCount = 100;
constexpr int kLkTailThreads = 1024;
// images of more pixels than this get one grid launch per level in place of the one-workgroup tail
constexpr int64_t kLkTailMaxPixels = 1024 * 1024;

struct LkLevel {
  int h, w;
  int64_t img, der;   // byte offsets in the blob
};
struct LkLayout {
  int levels;
  LkLevel lv[kLkMaxLevels];
  size_t bytes;
};

// false for an unsupported shape (the limits of the header)
bool lk_layout(int h, int w, int win, int max_level, LkLayout* L) {
  if (win < kLkMinWin || win > kLkMaxWin || (win & 1) == 0) return false;
  if (max_level < 0 || max_level >= kLkMaxLevels) return false;
  if (h <= win || w <= win || h > kLkMaxDim || w > kLkMaxDim) return false;
  size_t off = 0;
  int n = 0;
  for (;;) {
    LkLevel& v = L->lv[n++];
    v.h = h;
    v.w = w;
    v.img = (int64_t)off;
    off = align_up(off + (size_t)h * w, 256);
    v.der = (int64_t)off;
    off = align_up(off + (size_t)h * w * 4, 256);
    const int nh = (h + 1) / 2, nw = (w + 1) / 2;
    if (n > max_level || nh <= win || nw <= win) break;
    h = nh;
    w = nw;
  }
  L->levels = n;
  L->bytes = off;
  return true;
}

// BORDER_REFLECT_101 for an index at most n - 1 outside [0, n); the clamp changes nothing there
__device__ __forceinline__ int reflect101(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return min(max(i, 0), n - 1);
}

__device__ __forceinline__ uint8_t pyrdown_px(const uint8_t* s, int h, int w, int y, int x) {
  const int k[5] = {1, 4, 6, 4, 1};
  int xs[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) xs[j] = reflect101(2 * x + j - 2, w);
  int sum = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const uint8_t* r = s + (int64_t)reflect101(2 * y + i - 2, h) * w;
    int rs = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) rs += k[j] * (int)r[xs[j]];
    sum += k[i] * rs;
  }
  return (uint8_t)((sum + 128) >> 8);
}

__device__ __forceinline__ short2 scharr_px(const uint8_t* s, int h, int w, int y, int x) {
  const uint8_t* ru = s + (int64_t)reflect101(y - 1, h) * w;
  const uint8_t* rc = s + (int64_t)y * w;
  const uint8_t* rd = s + (int64_t)reflect101(y + 1, h) * w;
  const int xc[3] = {reflect101(x - 1, w), x, reflect101(x + 1, w)};
  int t0[3], t1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int u = ru[xc[j]], c = rc[xc[j]], d = rd[xc[j]];
    t0[j] = (u + d) * 3 + c * 10;
    t1[j] = d - u;
  }
  short2 r;
  r.x = (short)(t0[2] - t0[0]);
  r.y = (short)((t1[2] + t1[0]) * 3 + t1[1] * 10);
  return r;
}

__global__ __launch_bounds__(256) void lk_pyr_head_kernel(const uint8_t* image, int64_t image_bs,
                                                          uint8_t* pyr, LkLayout lay,
                                                          int with_deriv) {
  const int h = lay.lv[0].h, w = lay.lv[0].w;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= h * w) return;
  const uint8_t* src = image + (int64_t)blockIdx.y * image_bs;
  uint8_t* blob = pyr + (int64_t)blockIdx.y * (int64_t)lay.bytes;
  blob[lay.lv[0].img + i] = src[i];
  if (with_deriv)
    reinterpret_cast<short2*>(blob + lay.lv[0].der)[i] = scharr_px(src, h, w, i / w, i % w);
  if (lay.levels > 1) {
    const int h1 = lay.lv[1].h, w1 = lay.lv[1].w;
    if (i < h1 * w1) blob[lay.lv[1].img + i] = pyrdown_px(src, h, w, i / w1, i % w1);
  }
}

// Levels are produced and consumed by the same workgroup: the barrier between them orders the
// global writes of one level before the reads of the next.
__global__ __launch_bounds__(kLkTailThreads) void lk_pyr_tail_kernel(uint8_t* pyr, LkLayout lay,
                                                                     int with_deriv) {
  uint8_t* blob = pyr + (int64_t)blockIdx.x * (int64_t)lay.bytes;
  for (int l = 1; l < lay.levels; ++l) {
    const int h = lay.lv[l].h, w = lay.lv[l].w;
    const uint8_t* src = blob + lay.lv[l].img;
    if (with_deriv) {
      short2* der = reinterpret_cast<short2*>(blob + lay.lv[l].der);
      for (int i = threadIdx.x; i < h * w; i += kLkTailThreads)
        der[i] = scharr_px(src, h, w, i / w, i % w);
    }
    if (l + 1 < lay.levels) {
      const int h1 = lay.lv[l + 1].h, w1 = lay.lv[l + 1].w;
      uint8_t* dst = blob + lay.lv[l + 1].img;
      for (int i = threadIdx.x; i < h1 * w1; i += kLkTailThreads)
        dst[i] = pyrdown_px(src, h, w, i / w1, i % w1);
    }
    __threadfence_block();
    __syncthreads();
  }
}

// One level of the tail across the grid, for images too large for one workgroup: the derivative
// of level l and the image of level l + 1, one launch per level (the launch boundary orders them).
__global__ __launch_bounds__(256) void lk_pyr_level_kernel(uint8_t* pyr, LkLayout lay, int l,
                                                           int with_deriv) {
  uint8_t* blob = pyr + (int64_t)blockIdx.y * (int64_t)lay.bytes;
  const int h = lay.lv[l].h, w = lay.lv[l].w;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= h * w) return;
  const uint8_t* src = blob + lay.lv[l].img;
  if (with_deriv)
    reinterpret_cast<short2*>(blob + lay.lv[l].der)[i] = scharr_px(src, h, w, i / w, i % w);
  if (l + 1 < lay.levels) {
    const int h1 = lay.lv[l + 1].h, w1 = lay.lv[l + 1].w;
    if (i < h1 * w1) blob[lay.lv[l + 1].img + i] = pyrdown_px(src, h, w, i / w1, i % w1);
  }
}

struct LkTrackArgs {
  const uint8_t* prev;
  int64_t prev_bs;   // bytes, 0 = shared
  const uint8_t* next;
  const float* pts;
  int64_t pts_bs;   // floats, 0 = shared
  const int* counts;
  int max_points, win, max_count;
  float eps2, min_eig;
  float* out;
  uint8_t* status;
  LkLayout lay;
};

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct LkWeights {
  int w00, w01, w10, w11;
};
// a, b in [0, 1): the fractional parts; round-half-even
__device__ __forceinline__ LkWeights lk_weights(float a, float b) {
  const float W = 16384.f;
  LkWeights k;
  k.w00 = (int)rintf((1.f - a) * (1.f - b) * W);
  k.w01 = (int)rintf(a * (1.f - b) * W);
  k.w10 = (int)rintf((1.f - a) * b * W);
  k.w11 = 16384 - k.w00 - k.w01 - k.w10;
  return k;
}

// descale(4-tap image sum, 9) at (x, y), reflected-101 outside the level
__device__ __forceinline__ int lk_image_tap(const uint8_t* img, int rows, int cols, int x, int y,
                                            const LkWeights& k) {
  const int x0 = reflect101(x, cols), x1 = reflect101(x + 1, cols);
  const uint8_t* r0 = img + (int64_t)reflect101(y, rows) * cols;
  const uint8_t* r1 = img + (int64_t)reflect101(y + 1, rows) * cols;
  const int v = (int)r0[x0] * k.w00 + (int)r0[x1] * k.w01 + (int)r1[x0] * k.w10 +
                (int)r1[x1] * k.w11;
  return (v + 256) >> 9;
}

// the float-first bounds test of the contract: floor(p) in [-win, n) on both axes.  NaN and
// values no int holds fail it before any conversion.
__device__ __forceinline__ bool lk_inside(float fx, float fy, int win, int cols, int rows) {
  return fx >= (float)(-win) && fx < (float)cols && fy >= (float)(-win) && fy < (float)rows;
}

template <int NPL>   // window pixels per lane: ceil(win^2 / 64) <= NPL
__global__ __launch_bounds__(256) void lk_track_kernel(LkTrackArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.y, pt = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int cnt = min(max(a.counts[b], 0), a.max_points);
  if (pt >= cnt) return;   // the whole wave
  const float* pp = a.pts + (int64_t)b * a.pts_bs + 2 * (int64_t)pt;
  float* outp = a.out + ((int64_t)b * a.max_points + pt) * 2;
  uint8_t* stp = a.status + (int64_t)b * a.max_points + pt;
  const float px = pp[0], py = pp[1];
  if (!(fabsf(px) < 1073741824.f && fabsf(py) < 1073741824.f)) {   // NaN, inf, beyond 2^30
    if (lane == 0) {
      const uint32_t* raw = reinterpret_cast<const uint32_t*>(pp);
      reinterpret_cast<uint32_t*>(outp)[0] = raw[0];
      reinterpret_cast<uint32_t*>(outp)[1] = raw[1];
      *stp = 0;
    }
    return;
  }
  const int win = a.win, npx = win * win;
  const float half = (float)(win - 1) * 0.5f;
  int wx[NPL], wy[NPL];
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int idx = k * 64 + lane;
    wy[k] = idx < npx ? idx / win : 0;
    wx[k] = idx < npx ? idx - wy[k] * win : 0;
  }
  const uint8_t* pblob = a.prev + (int64_t)b * a.prev_bs;
  const uint8_t* nblob = a.next + (int64_t)b * (int64_t)a.lay.bytes;
  float ox = 0.f, oy = 0.f;
  int status = 1;
  for (int l = a.lay.levels - 1; l >= 0; --l) {
    const int rows = a.lay.lv[l].h, cols = a.lay.lv[l].w;
    const float sc = 1.f / (float)(1 << l);
    float qx = px * sc, qy = py * sc;
    if (l == a.lay.levels - 1) {
      ox = qx;
      oy = qy;
    } else {
      ox = ox * 2.f;
      oy = oy * 2.f;
    }
    qx = qx - half;
    qy = qy - half;
    float fx = floorf(qx), fy = floorf(qy);
    if (!lk_inside(fx, fy, win, cols, rows)) {
      if (l == 0) status = 0;
      continue;
    }
    int ix = (int)fx, iy = (int)fy;
    LkWeights k = lk_weights(qx - fx, qy - fy);
    const uint8_t* pimg = pblob + a.lay.lv[l].img;
    const short2* pder = reinterpret_cast<const short2*>(pblob + a.lay.lv[l].der);
    const uint8_t* nimg = nblob + a.lay.lv[l].img;
    int I[NPL], Ix[NPL], Iy[NPL];
    int s11 = 0, s12 = 0, s22 = 0;   // 16 terms of at most 4080^2 each: no overflow
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const bool on = i * 64 + lane < npx;
      const int x = ix + wx[i], y = iy + wy[i];
      I[i] = lk_image_tap(pimg, rows, cols, x, y, k);
      int vx = 0, vy = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int xx = x + (t & 1), yy = y + (t >> 1);
        const int wt = t == 0 ? k.w00 : t == 1 ? k.w01 : t == 2 ? k.w10 : k.w11;
        if (on && xx >= 0 && xx < cols && yy >= 0 && yy < rows) {   // zero outside the level
          const short2 d = pder[(int64_t)yy * cols + xx];
          vx += (int)d.x * wt;
          vy += (int)d.y * wt;
        }
      }
      Ix[i] = on ? (vx + 8192) >> 14 : 0;
      Iy[i] = on ? (vy + 8192) >> 14 : 0;
      s11 += Ix[i] * Ix[i];
      s12 += Ix[i] * Iy[i];
      s22 += Iy[i] * Iy[i];
    }
    const float A11 = (float)wave_sum_ll(s11) * 0x1p-20f;
    const float A12 = (float)wave_sum_ll(s12) * 0x1p-20f;
    const float A22 = (float)wave_sum_ll(s22) * 0x1p-20f;
    const float D = A11 * A22 - A12 * A12;
    const float dif = A11 - A22;
    // sqrtf and / are the correctly rounded ones here (hipcc's default
    // -fhip-fp32-correctly-rounded-divide-sqrt); __fsqrt_rn is not: it is the native 1-ulp one
    const float min_eig = (A22 + A11 - sqrtf(dif * dif + 4.f * A12 * A12)) / (float)(2 * npx);
    if (min_eig < a.min_eig || D < FLT_EPSILON) {
      if (l == 0) status = 0;
      continue;
    }
    const float Dinv = 1.f / D;
    float nx = ox - half, ny = oy - half;
    float pdx = 0.f, pdy = 0.f;
    for (int j = 0; j < a.max_count; ++j) {
      fx = floorf(nx);
      fy = floorf(ny);
      if (!lk_inside(fx, fy, win, cols, rows)) {
        if (l == 0) status = 0;
        break;
      }
      ix = (int)fx;
      iy = (int)fy;
      k = lk_weights(nx - fx, ny - fy);
      int t1 = 0, t2 = 0;   // 16 terms of at most 8160 * 4080 each: no overflow
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        const int diff = lk_image_tap(nimg, rows, cols, ix + wx[i], iy + wy[i], k) - I[i];
        t1 += diff * Ix[i];   // Ix, Iy are 0 off the window
        t2 += diff * Iy[i];
      }
      const float b1 = (float)wave_sum_ll(t1) * 0x1p-20f;
      const float b2 = (float)wave_sum_ll(t2) * 0x1p-20f;
      const float dx = (A12 * b2 - A22 * b1) * Dinv;
      const float dy = (A12 * b1 - A11 * b2) * Dinv;
      nx = nx + dx;
      ny = ny + dy;
      ox = nx + half;
      oy = ny + half;
      if (dx * dx + dy * dy <= a.eps2) break;
      if (j > 0 && fabsf(dx + pdx) < 0.01f && fabsf(dy + pdy) < 0.01f) {
        ox = ox - dx * 0.5f;
        oy = oy - dy * 0.5f;
        break;
      }
      pdx = dx;
      pdy = dy;
    }
  }
  if (lane == 0) {
    outp[0] = ox;
    outp[1] = oy;
    *stp = (uint8_t)status;
  }
}

}  // namespace
}  // namespace onepose

using namespace onepose;

extern "C" {

int onepose_lk_version(void) { return 1; }

int onepose_lk_levels(int h, int w, int win, int max_level) {
  LkLayout L;
  return lk_layout(h, w, win, max_level, &L) ? L.levels : 0;
}

size_t onepose_lk_pyramid_bytes(int h, int w, int win, int max_level) {
  LkLayout L;
  return lk_layout(h, w, win, max_level, &L) ? L.bytes : 0;
}

int onepose_lk_pyramid_layout(int h, int w, int win, int max_level, int level, int* lh, int* lw,
                              int64_t* image_offset, int64_t* deriv_offset) {
  clear_error();
  LkLayout L;
  OP_REQUIRE(lk_layout(h, w, win, max_level, &L),
             "lk_pyramid_layout: unsupported h=%d w=%d win=%d max_level=%d", h, w, win, max_level);
  OP_REQUIRE(level >= 0 && level < L.levels, "lk_pyramid_layout: level %d of %d", level, L.levels);
  OP_REQUIRE(lh && lw && image_offset && deriv_offset, "lk_pyramid_layout: null pointer");
  *lh = L.lv[level].h;
  *lw = L.lv[level].w;
  *image_offset = L.lv[level].img;
  *deriv_offset = L.lv[level].der;
  return ONEPOSE_OK;
}

int onepose_lk_build_pyramid(const uint8_t* image, int64_t image_bstride, int batch, int h, int w,
                             int win, int max_level, int with_deriv, void* pyramids,
                             void* stream) {
  clear_error();
  LkLayout L;
  OP_REQUIRE(lk_layout(h, w, win, max_level, &L),
             "lk_build_pyramid: unsupported h=%d w=%d win=%d max_level=%d", h, w, win, max_level);
  OP_REQUIRE(image && pyramids, "lk_build_pyramid: null pointer");
  OP_REQUIRE(batch >= 1 && batch <= 65535, "lk_build_pyramid: batch=%d", batch);
  OP_REQUIRE(batch == 1 || image_bstride >= (int64_t)h * w,
             "lk_build_pyramid: image_bstride %lld < h*w", (long long)image_bstride);
  OP_REQUIRE(with_deriv == 0 || with_deriv == 1, "lk_build_pyramid: with_deriv=%d", with_deriv);
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint8_t* pyr = static_cast<uint8_t*>(pyramids);
  hipLaunchKernelGGL(lk_pyr_head_kernel, dim3(ceil_div(h * w, 256), batch), dim3(256), 0, st,
                     image, image_bstride, pyr, L, with_deriv);
  OP_LAUNCHED();
  if (L.levels > 2 || (L.levels == 2 && with_deriv)) {
    if ((int64_t)h * w <= kLkTailMaxPixels) {
      hipLaunchKernelGGL(lk_pyr_tail_kernel, dim3(batch), dim3(kLkTailThreads), 0, st, pyr, L,
                         with_deriv);
      OP_LAUNCHED();
    } else {
      for (int l = 1; l < L.levels; ++l) {
        if (!with_deriv && l + 1 == L.levels) break;   // nothing to write at the top level
        hipLaunchKernelGGL(lk_pyr_level_kernel, dim3(ceil_div(L.lv[l].h * L.lv[l].w, 256), batch),
                           dim3(256), 0, st, pyr, L, l, with_deriv);
        OP_LAUNCHED();
      }
    }
  }
  return ONEPOSE_OK;
}

int onepose_lk_track(const void* prev_pyr, int64_t prev_pyr_bstride, const void* next_pyr,
                     const float* prev_pts, int64_t prev_pts_bstride, const int* counts, int batch,
                     int max_points, int h, int w, int win, int max_level, int max_count,
                     float epsilon, float min_eig_threshold, float* next_pts, uint8_t* status,
                     void* stream) {
  clear_error();
  LkTrackArgs a;
  OP_REQUIRE(lk_layout(h, w, win, max_level, &a.lay),
             "lk_track: unsupported h=%d w=%d win=%d max_level=%d", h, w, win, max_level);
  OP_REQUIRE(batch >= 1 && batch <= 65535, "lk_track: batch=%d", batch);
  OP_REQUIRE(max_points >= 0 && max_points <= (1 << 24), "lk_track: max_points=%d", max_points);
  OP_REQUIRE(epsilon == epsilon && min_eig_threshold == min_eig_threshold,
             "lk_track: NaN epsilon or min_eig_threshold");
  OP_REQUIRE(prev_pyr_bstride == 0 || prev_pyr_bstride >= (int64_t)a.lay.bytes,
             "lk_track: prev_pyr_bstride %lld is neither 0 nor >= %zu bytes",
             (long long)prev_pyr_bstride, a.lay.bytes);
  OP_REQUIRE(prev_pts_bstride == 0 || prev_pts_bstride >= 2 * (int64_t)max_points,
             "lk_track: prev_pts_bstride %lld is neither 0 nor >= 2*max_points",
             (long long)prev_pts_bstride);
  if (max_points == 0) return ONEPOSE_OK;
  OP_REQUIRE(prev_pyr && next_pyr && prev_pts && counts && next_pts && status,
             "lk_track: null pointer");
  a.prev = static_cast<const uint8_t*>(prev_pyr);
  a.prev_bs = prev_pyr_bstride;
  a.next = static_cast<const uint8_t*>(next_pyr);
  a.pts = prev_pts;
  a.pts_bs = prev_pts_bstride;
  a.counts = counts;
  a.max_points = max_points;
  a.win = win;
  a.max_count = max_count < 0 ? 0 : max_count > kLkMaxCount ? kLkMaxCount : max_count;
  const double e = epsilon < 0.f ? 0.0 : epsilon > 10.f ? 10.0 : (double)epsilon;
  a.eps2 = (float)(e * e);
  a.min_eig = min_eig_threshold;
  a.out = next_pts;
  a.status = status;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(ceil_div(max_points, 4), batch), block(256);
  const int npl = ceil_div(win * win, 64);
  if (npl <= 1)
    hipLaunchKernelGGL(lk_track_kernel<1>, grid, block, 0, st, a);
  else if (npl <= 4)
    hipLaunchKernelGGL(lk_track_kernel<4>, grid, block, 0, st, a);
  else if (npl <= 8)
    hipLaunchKernelGGL(lk_track_kernel<8>, grid, block, 0, st, a);
  else
    hipLaunchKernelGGL(lk_track_kernel<16>, grid, block, 0, st, a);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

}  // extern "C"
