// The 2D object detector's arithmetic on gfx950 (include/onepose_hip.h, "2D object detector"):
//   * cv2.estimateAffinePartial2D(method=RANSAC) as OpenCV 4.4 runs it, one workgroup per
//     reference view, with the view's correspondences in LDS (16 B each);
//   * the box of the warped view corners and the choice of view;
//   * crop_img_by_bbox as one integer bilinear warp.
//
// RANSAC, per round of 64 iterations of OpenCV's loop:
//   1. wave 0 generates the round's cv::RNG draws by jump-ahead (ransac.h), thread 0 deals the
//      64 two-point subsets from them in iteration order (a duplicate index is redrawn, so a
//      subset takes a varying number of draws; a chain that outruns the generated draws goes
//      on sequentially);
//   2. lane h of wave 0 solves minimal model h in double;
//   3. all 256 threads count the inliers of the 64 models (float32 error, as
//      AffinePartial2DEstimatorCallback::computeError);
//   4. thread 0 replays the acceptance rule in iteration order and stops where OpenCV would.
// Iterations evaluated beyond the stopping point are discarded, so the model, the mask and the
// iteration count are those of the sequential loop.  Wave 0 then refines the model over the
// inliers (Levenberg-Marquardt in the shape of LMSolverImpl::run).
#include "common.h"
#include "ransac.h"

namespace onepose {
namespace {

constexpr int kModelPoints = 2;
constexpr int kRound = 64;
constexpr int kThreads = 256;
constexpr int kDrawsPerLane = 4;   // generated per round: 8 + 4 * 64 draws
constexpr int kMinMatches = 6;     // local_feature_2D_detector.py:93

struct Shared {
  RansacDraws<kDrawsPerLane> draws;
  int subset[kRound][kModelPoints];
  double hyp[kRound][4];             // S0..S3 of each hypothesis
  int count[kRound];
  RansacCtl ctl;
  double best[4];
  int wave_cnt[4];
  double h[4];                       // refined [a, b, tx, ty]
};

// The minimal similarity through two correspondences (x, y) -> (X, Y), in double without
// contraction: M = [S0, -S1, S2; S1, S0, S3].  Coincident source points divide by zero and give a
// non-finite model (no inliers).
__device__ __forceinline__ void minimal_model(const float4 p1, const float4 p2, double* S) {
#pragma clang fp contract(off)
  const double x1 = p1.x, y1 = p1.y, X1 = p1.z, Y1 = p1.w;
  const double x2 = p2.x, y2 = p2.y, X2 = p2.z, Y2 = p2.w;
  const double dx = x1 - x2, dy = y1 - y2;
  const double d = 1.0 / (dx * dx + dy * dy);
  const double c = x1 * y2 - x2 * y1;
  S[0] = d * ((X1 - X2) * dx + (Y1 - Y2) * dy);
  S[1] = d * ((Y1 - Y2) * dx - (X1 - X2) * dy);
  S[2] = d * ((Y1 - Y2) * c - (X1 * y2 - X2 * y1) * dy - (X1 * x2 - X2 * x1) * dx);
  S[3] = d * (-(X1 - X2) * c - (Y1 * x2 - Y2 * x1) * dx - (Y1 * y2 - Y2 * y1) * dy);
}

// computeError: the model cast to float, the squared distance in float, no contraction
__device__ __forceinline__ float affine_err2(const float* F, const float4 p) {
#pragma clang fp contract(off)
  const float a = F[0] * p.x + F[1] * p.y + F[2] - p.z;
  const float b = F[3] * p.x + F[4] * p.y + F[5] - p.w;
  return a * a + b * b;
}

__device__ __forceinline__ void model_to_float(const double* S, float* F) {
  F[0] = (float)S[0];
  F[1] = (float)(-S[1]);
  F[2] = (float)S[2];
  F[3] = (float)S[1];
  F[4] = (float)S[0];
  F[5] = (float)S[3];
}

// Correspondence selection fused into the kernel (onepose_detect_stage): view b's valid matches
// (matches0 > -1, among its first counts0[b] keypoints) compacted in ascending index order
// straight into LDS.  matches0 null: the points are given (onepose_affine_partial_ransac).
struct DetSel {
  const int64_t* matches0;
  const int* counts0;
  const float* kp0;
  const float* kp1;
  int64_t kp1_bs;
  int n0, n1;
  const int* db_hw;
  int qh, qw;
  int* counts;
  int* bbox;
  float* mpts;
};

__global__ __launch_bounds__(kThreads)
void affine_ransac_kernel(const float* __restrict__ from, const float* __restrict__ to,
                          const int* __restrict__ counts, int max_points, double threshold,
                          int max_iters, double confidence, int refine_iters,
                          double* __restrict__ affine, uint8_t* __restrict__ mask_out,
                          int* __restrict__ n_inliers, int* __restrict__ status,
                          int* __restrict__ iters_run, DetSel sel) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
  Shared& sh = *reinterpret_cast<Shared*>(dyn);
  float4* pts = reinterpret_cast<float4*>(dyn + ((sizeof(Shared) + 15) / 16) * 16);
  const int b = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool stage = sel.matches0 != nullptr;
  int n;
  if (stage) {
    const int64_t* m = sel.matches0 + (int64_t)b * sel.n0;
    const float* k0 = sel.kp0 + (int64_t)b * sel.n0 * 2;
    const float* k1 = sel.kp1 + b * sel.kp1_bs;
    const int nk = sel.counts0 ? min(max(sel.counts0[b], 0), sel.n0) : sel.n0;
    float* mo = sel.mpts ? sel.mpts + (int64_t)b * max_points * 4 : nullptr;
    int base = 0;
    for (int start = 0; start < nk; start += kThreads) {
      const int i = start + t;
      const int64_t j = (i < nk) ? m[i] : -1;
      const bool valid = j > -1 && j < sel.n1;
      const int q = compact_step<4>(valid, sh.wave_cnt, base);
      if (valid) {
        const float4 p = make_float4(k0[(int64_t)i * 2], k0[(int64_t)i * 2 + 1], k1[j * 2],
                                     k1[j * 2 + 1]);
        pts[q] = p;
        if (mo) {   // four plain stores: mpts need not be 16-byte aligned
          mo[4 * q] = p.x;
          mo[4 * q + 1] = p.y;
          mo[4 * q + 2] = p.z;
          mo[4 * q + 3] = p.w;
        }
      }
    }
    n = base;
    if (t == 0) sel.counts[b] = n;
  } else {
    n = min(max(counts[b], 0), max_points);
  }
  uint8_t* mask = mask_out + (int64_t)b * max_points;
  double* A = affine + (int64_t)b * 6;
  for (int i = t; i < max_points; i += kThreads) mask[i] = 0;

  // no estimate: zero affine, no inliers, and (stage) the reference's fallback box
  auto none = [&](int st) {
    if (t < 6) A[t] = 0.0;
    if (t == 0) {
      n_inliers[b] = 0;
      status[b] = st;
      if (stage) {
        int* bb = sel.bbox + (int64_t)b * 4;
        bb[0] = 0;
        bb[1] = 0;
        bb[2] = sel.qh;   // query["size"] is (H, W): the reference's x1 is H
        bb[3] = sel.qw;
      }
    }
  };
  if (t == 0) iters_run[b] = 0;
  if (n < (stage ? kMinMatches : kModelPoints)) {
    none(1);
    return;
  }
  if (!stage) {
    for (int i = t; i < n; i += kThreads) {
      const int64_t g = ((int64_t)b * max_points + i) * 2;
      pts[i] = make_float4(from[g], from[g + 1], to[g], to[g + 1]);
    }
  }
  const float thr = (float)(threshold * threshold);
  if (t == 0) ransac_ctl_init(sh.ctl, max_iters, n == kModelPoints);
  __syncthreads();

  if (n == kModelPoints) {   // the kernel once on both points; all points are inliers
    if (t == 0) {
      double S[4];
      minimal_model(pts[0], pts[1], S);
      A[0] = S[0];
      A[1] = -S[1];
      A[2] = S[2];
      A[3] = S[1];
      A[4] = S[0];
      A[5] = S[3];
      n_inliers[b] = 2;
      status[b] = 0;
    }
    if (t < 2) mask[t] = 1;   // (thread t zeroed mask[t] above)
    return;   // (the stage never gets here: it needs 6 matches)
  }

  while (!sh.ctl.done) {
    if (wave == 0) {
      const int P = ransac_round_draws(sh.draws, sh.ctl, n);   // the round's draws, in parallel
      wave_lds_sync();
      if (lane == 0) {   // getSubset x 64 in iteration order
        unsigned long long st = sh.ctl.rng;
        int pos = 0;
        auto draw = [&]() {
          int v;
          if (pos < P) {
            st = sh.draws.rst[pos];
            v = sh.draws.rii[pos];
          } else {
            v = (int)(rng_next(st) % (unsigned)n);
          }
          ++pos;
          return v;
        };
        for (int h = 0; h < kRound; ++h) {
          const int i0 = draw();
          int i1 = draw();
          while (i1 == i0) i1 = draw();
          sh.subset[h][0] = i0;
          sh.subset[h][1] = i1;
        }
        sh.ctl.rng = st;
      }
      wave_lds_sync();
      double S[4];
      minimal_model(pts[sh.subset[lane][0]], pts[sh.subset[lane][1]], S);
#pragma unroll
      for (int i = 0; i < 4; ++i) sh.hyp[lane][i] = S[i];
    }
    __syncthreads();
    // inlier counts (wave w counts hypotheses w, w + 4, ...; lanes sweep the points)
    for (int h = wave; h < kRound; h += 4) {
      float F[6];
      model_to_float(sh.hyp[h], F);
      const int c =
          wave_count_if(lane, n, 64, [&](int i) { return affine_err2(F, pts[i]) <= thr; });
      if (lane == 0) sh.count[h] = c;
    }
    __syncthreads();
    if (t == 0) {   // the acceptance rule, in iteration order
      ransac_accept(sh.ctl, sh.count, 0, kRound, n, confidence, kModelPoints, [&](int h) {
        for (int i = 0; i < 4; ++i) sh.best[i] = sh.hyp[h][i];
      });
    }
    __syncthreads();
  }

  if (t == 0) iters_run[b] = sh.ctl.iter;
  if (sh.ctl.max_good <= 0) {
    none(2);
    return;
  }
  // the best model's mask
  float F[6];
  model_to_float(sh.best, F);
  const int c = wave_count_if(t, n, kThreads, [&](int i) {
    const bool in = affine_err2(F, pts[i]) <= thr;
    mask[i] = in ? 1 : 0;
    return in;
  });
  if (lane == 0) sh.wave_cnt[wave] = c;
  __syncthreads();
  const int nin = sh.wave_cnt[0] + sh.wave_cnt[1] + sh.wave_cnt[2] + sh.wave_cnt[3];
  if (wave != 0) return;

  // Levenberg-Marquardt over the inliers, wave 0: h = [a, b, tx, ty], residuals
  // (a x - b y + tx - X, b x + a y + ty - Y).  J^T J is constant (the problem is linear):
  //   [P 0 sx sy; 0 P -sy sx; sx -sy n 0; sy sx 0 n],  P = sum x^2 + y^2,
  // so with its diagonal scaled by 1 + lambda the 4 x 4 system splits into 2 x 2 blocks
  // p I, B = [sx sy; -sy sx], q I with B B^T = (sx^2 + sy^2) I and is solved in closed form.
  double h[4] = {sh.best[0], sh.best[1], sh.best[2], sh.best[3]};
  if (refine_iters > 0) {
    double P = 0.0, sx = 0.0, sy = 0.0;
    for (int i = lane; i < n; i += 64) {
      const float4 p = pts[i];
      if (affine_err2(F, p) <= thr) {
        const double x = p.x, y = p.y;
        P += x * x + y * y;
        sx += x;
        sy += y;
      }
    }
    P = wave_sum_d(P);
    sx = wave_sum_d(sx);
    sy = wave_sum_d(sy);
    // |r|^2, J^T r and |r|_inf at a parameter vector
    auto residual = [&](const double* hh, double* g, double& rinf) {
      double S = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0, rm = 0.0;
      for (int i = lane; i < n; i += 64) {
        const float4 p = pts[i];
        if (affine_err2(F, p) <= thr) {
          const double x = p.x, y = p.y;
          const double rx = hh[0] * x - hh[1] * y + hh[2] - (double)p.z;
          const double ry = hh[1] * x + hh[0] * y + hh[3] - (double)p.w;
          S += rx * rx + ry * ry;
          g0 += x * rx + y * ry;
          g1 += x * ry - y * rx;
          g2 += rx;
          g3 += ry;
          rm = fmax(rm, fmax(fabs(rx), fabs(ry)));
        }
      }
      g[0] = wave_sum_d(g0);
      g[1] = wave_sum_d(g1);
      g[2] = wave_sum_d(g2);
      g[3] = wave_sum_d(g3);
      rinf = wave_max_d(rm);
      return wave_sum_d(S);
    };
    double g[4], rinf;
    double S = residual(h, g, rinf);
    int log_lambda = -3;
    for (int it = 0; it < refine_iters; ++it) {
      const double f = 1.0 + pow(10.0, (double)log_lambda);
      const double p = P * f, q = (double)nin * f;
      const double det = p * q - (sx * sx + sy * sy);
      double d[4];
      d[0] = (q * g[0] - (sx * g[2] + sy * g[3])) / det;
      d[1] = (q * g[1] - (sx * g[3] - sy * g[2])) / det;
      d[2] = (p * g[2] - (sx * g[0] - sy * g[1])) / det;
      d[3] = (p * g[3] - (sy * g[0] + sx * g[1])) / det;
      const double hn[4] = {h[0] - d[0], h[1] - d[1], h[2] - d[2], h[3] - d[3]};
      double gn[4], rn;
      const double Sn = residual(hn, gn, rn);
      if (Sn < S) {
        S = Sn;
        rinf = rn;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          h[i] = hn[i];
          g[i] = gn[i];
        }
        log_lambda = max(log_lambda - 1, -16);
      } else {
        log_lambda = min(log_lambda + 1, 16);
      }
      const double dinf = fmax(fmax(fabs(d[0]), fabs(d[1])), fmax(fabs(d[2]), fabs(d[3])));
      if (dinf < 1.1920928955078125e-07 || rinf < 1.1920928955078125e-07) break;
    }
  }
  if (lane == 0) {
    A[0] = h[0];
    A[1] = -h[1];
    A[2] = h[2];
    A[3] = h[1];
    A[4] = h[0];
    A[5] = h[3];
    n_inliers[b] = nin;
    status[b] = 0;
    if (stage) {   // the view's corners through the affine, truncated toward zero
      const int vh = sel.db_hw[2 * b], vw = sel.db_hw[2 * b + 1];
      int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
      for (int k = 0; k < 4; ++k) {
        const double cx = (k & 1) ? (double)vw : 0.0, cy = (k & 2) ? (double)vh : 0.0;
        const int px = (int)(h[0] * cx - h[1] * cy + h[2]);
        const int py = (int)(h[1] * cx + h[0] * cy + h[3]);
        x0 = k ? min(x0, px) : px;
        x1 = k ? max(x1, px) : px;
        y0 = k ? min(y0, py) : py;
        y1 = k ? max(y1, py) : py;
      }
      int* bb = sel.bbox + (int64_t)b * 4;
      bb[0] = x0;
      bb[1] = y0;
      bb[2] = x1;
      bb[3] = y1;
    }
  }
}

// detect_by_matching's choice of view: the first view, in input order, with the largest rank
// value.  rank_mode 0: the number of matched points (the reference sorts by the N x 1 mask's
// row count); 1: the number of inliers.  A view without an estimate ranks as 0.
__global__ void rank_views_kernel(const int* __restrict__ counts, const int* __restrict__ n_inliers,
                                  const int* __restrict__ status, const int* __restrict__ bbox,
                                  int batch, int rank_mode, int* __restrict__ best_view,
                                  int* __restrict__ best_bbox) {
  const int lane = threadIdx.x;
  int bv = 0x7fffffff, bval = -1;
  for (int b = lane; b < batch; b += 64) {
    const int v = status[b] == 0 ? (rank_mode == 0 ? counts[b] : n_inliers[b]) : 0;
    if (v > bval) {   // ascending b within a lane: the first of equals stays
      bval = v;
      bv = b;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int ov = __shfl_xor(bval, o, 64), ob = __shfl_xor(bv, o, 64);
    if (ov > bval || (ov == bval && ob < bv)) {
      bval = ov;
      bv = ob;
    }
  }
  if (lane == 0) best_view[0] = bv;
  if (lane < 4) best_bbox[lane] = bbox[(int64_t)bv * 4 + lane];
}

// crop_img_by_bbox: the two warpAffine calls as one bilinear warp of the zero-padded window
// [x0, x1) x [y0, y1) of the image, in warpAffine's fixed-point arithmetic (AB_BITS 10,
// INTER_BITS 5, weights summing to 2^15), and K_crop = T2 T1 K.
__global__ __launch_bounds__(256)
void crop_resize_kernel(const uint8_t* __restrict__ image, int h, int w,
                        const int* __restrict__ bbox, const double* __restrict__ K, int crop,
                        uint8_t* __restrict__ out_u8, float* __restrict__ out_f32,
                        double* __restrict__ K_crop, int* __restrict__ crop_status) {
#pragma clang fp contract(off)
  const int x0 = bbox[0], y0 = bbox[1], x1 = bbox[2], y1 = bbox[3];
  const int64_t bw = (int64_t)x1 - x0, bh = (int64_t)y1 - y0;
  // status 1: an empty box; 2: a coordinate outside warpAffine's short maps (the integer walk
  // below would leave int range).  Either way a zero image and K_crop = K.
  auto big = [](int v) { return v >= 32768 || v <= -32768; };
  const int box_status = (bw <= 0 || bh <= 0) ? 1 : (big(x0) || big(y0) || big(x1) || big(y1)) ? 2 : 0;
  const bool bad = box_status != 0;
  const int ox = blockIdx.x * 64 + (threadIdx.x & 63);
  const int oy = blockIdx.y * 4 + (threadIdx.x >> 6);
  // T2 = [s 0 tx; 0 s ty]: uniform scale by the window's width (data_utils.py:34)
  const double s = bad ? 1.0 : (double)crop / (double)bw;
  const double tx = (double)crop * 0.5 - s * (double)bw * 0.5;
  const double ty = (double)crop * 0.5 - s * (double)bh * 0.5;
  if (blockIdx.x == 0 && blockIdx.y == 0) {
    if (threadIdx.x == 0) crop_status[0] = box_status;
    if (K != nullptr && threadIdx.x < 9) {
      const int r = threadIdx.x / 3, c = threadIdx.x % 3;
      double v = K[threadIdx.x];
      if (!bad && r < 2) {
        const double k1 = K[r * 3 + c] - (double)(r == 0 ? x0 : y0) * K[6 + c];   // T1 K
        v = s * k1 + (r == 0 ? tx : ty) * K[6 + c];                                // T2 (T1 K)
      }
      K_crop[threadIdx.x] = v;
    }
  }
  if (ox >= crop || oy >= crop) return;
  int val = 0;
  if (!bad) {
    // warpAffine inverts the matrix, then walks it in 1/1024 steps
    double D = s * s;
    D = D != 0.0 ? 1.0 / D : 0.0;
    const double A11 = s * D, A22 = s * D;
    const double b1 = -A11 * tx, b2 = -A22 * ty;
    const int adelta = __double2int_rn(A11 * (double)ox * 1024.0);
    const int X0 = __double2int_rn(b1 * 1024.0) + 16;
    const int Y0 = __double2int_rn((A22 * (double)oy + b2) * 1024.0) + 16;
    const int X = (X0 + adelta) >> 5, Y = Y0 >> 5;
    const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
    auto tap = [&](int ix, int iy) -> int {
      if (ix < 0 || iy < 0 || ix >= bw || iy >= bh) return 0;
      const int64_t gx = (int64_t)x0 + ix, gy = (int64_t)y0 + iy;
      if (gx < 0 || gy < 0 || gx >= w || gy >= h) return 0;
      return image[gy * w + gx];
    };
    const int acc = (32 - fx) * (32 - fy) * 32 * tap(sx, sy) + fx * (32 - fy) * 32 * tap(sx + 1, sy) +
                    (32 - fx) * fy * 32 * tap(sx, sy + 1) + fx * fy * 32 * tap(sx + 1, sy + 1);
    val = (acc + 16384) >> 15;
    val = min(val, 255);
  }
  const int64_t o = (int64_t)oy * crop + ox;
  out_u8[o] = (uint8_t)val;
  if (out_f32 != nullptr) out_f32[o] = (float)val / 255.0f;
}

}  // namespace
}  // namespace onepose

using namespace onepose;

extern "C" {

constexpr size_t kDetLdsBudget = 160 * 1024;
constexpr size_t kDetSharedBytes = ((sizeof(Shared) + 15) / 16) * 16;
constexpr size_t kDetPointBytes = 16;
static_assert(kDetSharedBytes < kDetLdsBudget, "Shared leaves no room for points");

int onepose_detector_version(void) { return 1; }

int onepose_affine_partial_max_points(void) {
  return (int)((kDetLdsBudget - kDetSharedBytes) / kDetPointBytes);
}

size_t onepose_affine_partial_workspace_bytes(int batch, int max_points) {
  if (batch <= 0 || max_points <= 0) return 0;
  return align_up((size_t)batch * sizeof(int), 256);
}

static int launch_ransac(const char* who, const float* from, const float* to, const int* counts,
                         int max_points, int batch, double threshold, int max_iters,
                         double confidence, int refine_iters, double* affine,
                         uint8_t* inlier_mask, int* n_inliers, int* status, void* workspace,
                         size_t workspace_bytes, const DetSel& sel, hipStream_t st) {
  OP_REQUIRE(batch >= 1 && max_points >= 1, "%s: batch=%d max_points=%d", who, batch, max_points);
  OP_REQUIRE(max_points <= onepose_affine_partial_max_points(),
             "%s: max_points=%d above onepose_affine_partial_max_points() = %d (LDS)", who,
             max_points, onepose_affine_partial_max_points());
  OP_REQUIRE(threshold >= 0.0, "%s: threshold %f negative", who, threshold);
  OP_REQUIRE(confidence > 0 && confidence < 1, "%s: confidence %f not in (0,1)", who, confidence);
  OP_REQUIRE(refine_iters >= 0, "%s: refine_iters %d negative", who, refine_iters);
  const size_t need = onepose_affine_partial_workspace_bytes(batch, max_points);
  if (!workspace || workspace_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    return ONEPOSE_ERR_WORKSPACE;
  }
  static bool attr_set = false;
  if (!attr_set) {
    OP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(affine_ransac_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDetLdsBudget));
    attr_set = true;
  }
  const size_t lds = kDetSharedBytes + (size_t)max_points * kDetPointBytes;
  // (no profile kind: the kind list is closed by the SuperGlue family's four)
  hipLaunchKernelGGL(affine_ransac_kernel, dim3(batch), dim3(kThreads), lds, st, from, to, counts,
                     max_points, threshold, max_iters, confidence, refine_iters, affine,
                     inlier_mask, n_inliers, status, static_cast<int*>(workspace), sel);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

int onepose_affine_partial_ransac(const float* from, const float* to, const int* counts,
                                  int max_points, int batch, double threshold, int max_iters,
                                  double confidence, int refine_iters, double* affine,
                                  uint8_t* inlier_mask, int* n_inliers, int* status,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  OP_REQUIRE(from && to && counts, "affine_partial: null input");
  OP_REQUIRE(affine && inlier_mask && n_inliers && status, "affine_partial: null output");
  const DetSel none{};
  return launch_ransac("affine_partial", from, to, counts, max_points, batch, threshold,
                       max_iters, confidence, refine_iters, affine, inlier_mask, n_inliers, status,
                       workspace, workspace_bytes, none, static_cast<hipStream_t>(stream));
}

int onepose_detect_stage(const int64_t* matches0, const int* counts0, const float* kpts0,
                         const float* kpts1, int64_t kpts1_bstride, const int* db_hw, int batch,
                         int n0, int n1, int query_h, int query_w, double threshold,
                         int max_iters, double confidence, int refine_iters, int rank_mode,
                         int* counts, float* mpts, double* affine, uint8_t* inlier_mask,
                         int* n_inliers, int* status, int* bbox, int* best_view, int* best_bbox,
                         void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  OP_REQUIRE(matches0 && kpts0 && kpts1 && db_hw, "detect_stage: null input");
  OP_REQUIRE(counts && affine && inlier_mask && n_inliers && status && bbox && best_view &&
                 best_bbox,
             "detect_stage: null output");
  OP_REQUIRE(n1 >= 1, "detect_stage: n1=%d", n1);
  OP_REQUIRE(rank_mode == 0 || rank_mode == 1, "detect_stage: rank_mode %d not 0 or 1", rank_mode);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const DetSel sel{matches0, counts0, kpts0, kpts1, kpts1_bstride, n0, n1, db_hw,
                   query_h, query_w, counts, bbox, mpts};
  const int rc = launch_ransac("detect_stage", nullptr, nullptr, nullptr, n0, batch, threshold,
                               max_iters, confidence, refine_iters, affine, inlier_mask, n_inliers,
                               status, workspace, workspace_bytes, sel, st);
  if (rc != ONEPOSE_OK) return rc;
  hipLaunchKernelGGL(rank_views_kernel, dim3(1), dim3(64), 0, st, counts, n_inliers, status, bbox,
                     batch, rank_mode, best_view, best_bbox);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

int onepose_crop_resize(const uint8_t* image, int h, int w, const int* bbox, const double* K,
                        int crop_size, uint8_t* crop_u8, float* crop_f32, double* K_crop,
                        int* crop_status, void* stream) {
  clear_error();
  OP_REQUIRE(image && bbox, "crop_resize: null input");
  OP_REQUIRE(crop_u8 && crop_status, "crop_resize: null output");
  OP_REQUIRE(!K == !K_crop, "crop_resize: K and K_crop go together");
  OP_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w < (1ll << 31), "crop_resize: image %d x %d", h, w);
  OP_REQUIRE(crop_size >= 1 && crop_size <= 8192, "crop_resize: crop_size %d not in [1, 8192]",
             crop_size);
  hipLaunchKernelGGL(crop_resize_kernel, dim3(ceil_div(crop_size, 64), ceil_div(crop_size, 4)),
                     dim3(256), 0, static_cast<hipStream_t>(stream), image, h, w, bbox, K,
                     crop_size, crop_u8, crop_f32, K_crop, crop_status);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

}  // extern "C"
