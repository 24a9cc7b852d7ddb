// Tracker back end: bundle adjustment (src/tracker/ba_tracker.py:358-441, apply_ba, which hands
// the problem to DeepLM's Solve with SnavelyReprojectionErrorV2, tracking_utils.py:91-169) and
// two-view triangulation with track_ba's filters (ba_tracker.py:267-273, :546-571).  All fp64.
//
// What the reference pins is the cost function only: residual = f (R(aa) X + t).xy / (.).z +
// (cx, cy) - (u, v), with the reference's two rotation branches (theta^2 > 0: Rodrigues; else the
// first-order pt + aa x pt).  The solver on top is this project's (DeepLM's source is not part of
// the reference tree): a Ceres-style Levenberg-Marquardt with a Schur complement onto the cameras,
// stated in include/onepose_hip.h and restated in numpy float64 by tests/ba_oracle.py.
//
// Launches (every kernel returns at once when the state block says the solve is over, so the
// sequence is fixed and graph-capturable; accept / reject and the radius live on the device):
//   init, validate, gather, eval(initial), decide(initial), then per iteration
//   linearize -> reduce (U, V = L L^T, g, damping) -> whiten (Y = L^-1 W^T) -> schur ->
//   cholesky + solves -> update (dp and the candidate) -> eval (candidate residuals, model
//   decrease terms) -> decide.
// No floating-point atomics; every sum has a fixed order (per-camera sums: lane-strided over the
// camera's by-camera CSR range, then a 64-lane butterfly; per-point sums and the Schur products:
// one thread per output element walking CSR ranges in order; cost sums: 256 strided partial sums
// and a halving tree), so results are bit-identical from run to run and on any stream.
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"

namespace onepose {
namespace {

constexpr int kBaVersion = 1;
constexpr int kBaMaxActive = 24;          // active cameras: S is (6 * 24)^2, its packed lower
                                          // triangle 83.5 KB of the 160 KB of LDS
constexpr int64_t kBaMaxObs = 1 << 20;
constexpr int kBaMaxVars = 1 << 20;       // cameras, points
constexpr int kBaMaxIters = 16;
constexpr int kBaInfoHead = 8, kBaInfoRow = 6;
constexpr int kBaInfoDoubles = kBaInfoHead + kBaMaxIters * kBaInfoRow;
constexpr int kBaMagic = 0x42413031;      // "BA01"
constexpr int kBaHeader = 8;              // int32 words: magic, N, C, P, A, Pa, 0, 0
constexpr int kBaCholThreads = 256;
constexpr int kBaSchurThreads = 128;
constexpr double kBaSeriesTh2 = 1e-4;     // theta^2 below which the Jacobian's b, ca, ab are series
enum { BA_OK = 0, BA_FAILED = 1, BA_BAD_INDEX = 2 };

struct BaState {
  double radius, factor, cost;
  int done, iter, succ, chol_fail, need_lin, bad, pad0, pad1;
};

// The index as onepose_ba_build_index lays it out, located from (N, C, P) alone
struct BaIndex {
  const int *head, *act_cams, *act_pts, *cam_start, *pt_start, *cam_order, *pt_order;
  size_t bytes;
};
BaIndex ba_index_layout(const void* base, int64_t N, int C, int P) {
  const int* p = static_cast<const int*>(base);
  BaIndex ix;
  size_t off = 0;
  auto take = [&](size_t n) {
    const int* q = p ? p + off : nullptr;
    off += n;
    return q;
  };
  ix.head = take(kBaHeader);
  ix.act_cams = take(C);
  ix.act_pts = take(P);
  ix.cam_start = take((size_t)C + 1);
  ix.pt_start = take((size_t)P + 1);
  ix.cam_order = take(N);
  ix.pt_order = take(N);
  ix.bytes = align_up(off * sizeof(int), 256);
  return ix;
}

struct BaArgs {
  double *points, *cam_pose;
  const double* features;
  const int64_t *ptIdx, *camIdx;
  BaIndex ix;
  int N, C, P, A, Pa;
  int max_iters, max_success;
  double radius0;
  double* info;
  BaState* st;
  double *r, *Jc, *Jp, *W, *Y, *tcost, *tmd;   // per observation
  int *oacam, *oapt;                       // observation -> active camera / point slot
  double *U, *gc, *Lv, *gp, *S, *rhs, *dc, *dp, *camw, *ptw, *camn, *ptn;
};

void ba_carve(BaArgs& a, void* ws, size_t* bytes) {
  Carve cv(ws);
  const size_t N = a.N, A = a.A, Pa = a.Pa;
  a.st = cv.take<BaState>(1);
  a.r = cv.take<double>(2 * N);
  a.Jc = cv.take<double>(12 * N);
  a.Jp = cv.take<double>(6 * N);
  a.W = cv.take<double>(18 * N);
  a.Y = cv.take<double>(18 * N);
  a.tcost = cv.take<double>(N);
  a.tmd = cv.take<double>(N);
  a.oacam = cv.take<int>(N);
  a.oapt = cv.take<int>(N);
  a.U = cv.take<double>(36 * A);
  a.gc = cv.take<double>(6 * A);
  a.Lv = cv.take<double>(6 * Pa);
  a.gp = cv.take<double>(3 * Pa);
  a.S = cv.take<double>(36 * A * A);
  a.rhs = cv.take<double>(6 * A);
  a.dc = cv.take<double>(6 * A);
  a.dp = cv.take<double>(3 * Pa);
  a.camw = cv.take<double>(6 * A);
  a.ptw = cv.take<double>(3 * Pa);
  a.camn = cv.take<double>(6 * A);
  a.ptn = cv.take<double>(3 * Pa);
  *bytes = align_up(cv.off, 256);
}

// ---- the cost function ------------------------------------------------------------------
// SnavelyReprojectionErrorV2 for one observation: cam = (angle-axis, t), X, ft = (u, v, f, cx,
// cy).  Jc (2 x 6, row-major) and Jp (2 x 3) may be null.  The rotation follows
// AngleAxisRotatePoint operation by operation; the Jacobian is the derivative of that same
// expression, R X = c X + a (w x X) + b w (w . X) with a = sin / theta, b = (1 - cos) / theta^2
// (its coefficients by series below theta^2 = 1e-4; the residual path is untouched),
// and at theta^2 == 0 the derivative of the first-order branch X + w x X, i.e. -[X]x and I + [w]x.
__device__ __forceinline__ void ba_observe(const double* cam, const double* X, const double* ft,
                                           double* r, double* Jc, double* Jp) {
  const double w0 = cam[0], w1 = cam[1], w2 = cam[2];
  const double x0 = X[0], x1 = X[1], x2 = X[2];
  const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
  const double wx0 = w1 * x2 - w2 * x1, wx1 = w2 * x0 - w0 * x2, wx2 = w0 * x1 - w1 * x0;
  const double wd = w0 * x0 + w1 * x1 + w2 * x2;
  double p0, p1, p2, c = 1.0, a = 1.0, th = 0.0;
  if (th2 > 0.0) {
    th = sqrt(th2);
    c = cos(th);
    const double s = sin(th), inv = 1.0 / th;
    const double k0 = w0 * inv, k1 = w1 * inv, k2 = w2 * inv;
    const double tmp = (k0 * x0 + k1 * x1 + k2 * x2) * (1.0 - c);
    p0 = x0 * c + (k1 * x2 - k2 * x1) * s + k0 * tmp;
    p1 = x1 * c + (k2 * x0 - k0 * x2) * s + k1 * tmp;
    p2 = x2 * c + (k0 * x1 - k1 * x0) * s + k2 * tmp;
    a = s / th;
  } else {
    p0 = x0 + wx0;
    p1 = x1 + wx1;
    p2 = x2 + wx2;
  }
  p0 += cam[3];
  p1 += cam[4];
  p2 += cam[5];
  const double f = ft[2];
  const double xp = p0 / p2, yp = p1 / p2;
  r[0] = (f * xp + ft[3]) - ft[0];
  r[1] = (f * yp + ft[4]) - ft[1];
  if (Jc == nullptr) return;
  const double iz = 1.0 / p2;
  // D = d r / d p
  const double D00 = f * iz, D02 = -f * xp * iz, D11 = f * iz, D12 = -f * yp * iz;
  const double w[3] = {w0, w1, w2}, x[3] = {x0, x1, x2}, wx[3] = {wx0, wx1, wx2};
  double R[3][3], M[3][3];
  const double Xx[3][3] = {{0.0, -x2, x1}, {x2, 0.0, -x0}, {-x1, x0, 0.0}};
  const double Wx[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
  if (th2 > 0.0) {
    // b = (1 - cos) / theta^2, ca = (cos - a) / theta^2, ab = (a - 2 b) / theta^2: below
    // kBaSeriesTh2 from their series (error < 1e-16 there).  The closed forms cancel to nothing
    // under theta = 1e-8, and a subnormal theta^2 overflows the quotient into a NaN Jacobian.
    double b, ca, ab;
    if (th2 >= kBaSeriesTh2) {
      b = (1.0 - c) / th2;
      ca = (c - a) / th2;
      ab = (a - 2.0 * b) / th2;
    } else {
      b = 0.5 + th2 * (-1.0 / 24.0 + th2 * (1.0 / 720.0));
      ca = -1.0 / 3.0 + th2 * (1.0 / 30.0 + th2 * (-1.0 / 840.0));
      ab = -1.0 / 12.0 + th2 * (1.0 / 180.0 + th2 * (-1.0 / 6720.0));
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        R[i][j] = (i == j ? c : 0.0) + a * Wx[i][j] + b * w[i] * w[j];
        M[i][j] = -a * x[i] * w[j] + ca * wx[i] * w[j] - a * Xx[i][j] +
                  b * (w[i] * x[j] + (i == j ? wd : 0.0)) + ab * wd * w[i] * w[j];
      }
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        R[i][j] = (i == j ? 1.0 : 0.0) + Wx[i][j];
        M[i][j] = -Xx[i][j];
      }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    Jc[j] = D00 * M[0][j] + D02 * M[2][j];
    Jc[6 + j] = D11 * M[1][j] + D12 * M[2][j];
    Jp[j] = D00 * R[0][j] + D02 * R[2][j];
    Jp[3 + j] = D11 * R[1][j] + D12 * R[2][j];
  }
  Jc[3] = D00;
  Jc[4] = 0.0;
  Jc[5] = D02;
  Jc[9] = 0.0;
  Jc[10] = D11;
  Jc[11] = D12;
}

// Fixed-order sum of v[0 .. n) by one workgroup of 256: thread t adds v[t], v[t + 256], ... in
// order, then a halving tree over the 256 partial sums.  Every thread returns the total.
__device__ __forceinline__ double block_sum_256(const double* v, int n, double* lds) {
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int i = t; i < n; i += 256) acc += v[i];
  __syncthreads();   // lds may still be read from an earlier sum
  lds[t] = acc;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (t < h) lds[t] += lds[t + h];
    __syncthreads();
  }
  return lds[0];
}

// ---- stand-alone linearisation (onepose_ba_linearize) -------------------------------------
__global__ __launch_bounds__(256) void ba_linearize_plain_kernel(
    const double* points, const double* cam_pose, const double* features, const int64_t* ptIdx,
    const int64_t* camIdx, int N, int C, int P, double* r, double* Jc, double* Jp) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= N) return;
  const int64_t pi = ptIdx[o], ci = camIdx[o];
  double rr[2], jc[12], jp[6];
  if (pi < 0 || pi >= P || ci < 0 || ci >= C) {   // never dereferenced: the row is NaN
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    rr[0] = rr[1] = nan;
    for (int i = 0; i < 12; ++i) jc[i] = nan;
    for (int i = 0; i < 6; ++i) jp[i] = nan;
  } else {
    ba_observe(cam_pose + 6 * ci, points + 3 * pi, features + 5 * (int64_t)o, rr, jc, jp);
  }
  r[2 * (int64_t)o] = rr[0];
  r[2 * (int64_t)o + 1] = rr[1];
  for (int i = 0; i < 12; ++i) Jc[12 * (int64_t)o + i] = jc[i];
  for (int i = 0; i < 6; ++i) Jp[6 * (int64_t)o + i] = jp[i];
}

// cost = 1/2 sum r^2 over the 2 N residual entries, in block_sum_256's order on r^2
__global__ __launch_bounds__(256) void ba_cost_kernel(const double* r, int n2, double* cost) {
  __shared__ double lds[256];
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int i = t; i < n2; i += 256) acc += r[i] * r[i];
  lds[t] = acc;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (t < h) lds[t] += lds[t + h];
    __syncthreads();
  }
  if (t == 0) *cost = 0.5 * lds[0];
}

// ---- the solve ------------------------------------------------------------------------------
__global__ void ba_init_kernel(BaArgs P) {
  const int t = threadIdx.x;
  if (t < kBaInfoDoubles) P.info[t] = 0.0;
  if (t == 0) {
    BaState s;
    s.radius = P.radius0;
    s.factor = 2.0;
    s.cost = 0.0;
    s.done = s.iter = s.succ = s.chol_fail = s.bad = s.pad0 = s.pad1 = 0;
    s.need_lin = 1;
    *P.st = s;
  }
}

// largest a in [0, n) with start[a] <= k, whatever start holds (reads stay inside start[0 .. n))
__device__ __forceinline__ int ba_range_of(const int* start, int n, int k) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= k) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// One side (cameras or points) of the check for slot k of its CSR order: the range that claims
// k really holds it, the observation there is in [0, N), carries the range's key, and follows
// its predecessor in observation order (stable, and hence a permutation).  Returns the active
// slot or -1.
__device__ __forceinline__ int ba_check_slot(const int* start, const int* order, const int* act,
                                             int n_act, const int64_t* key, int N, int k,
                                             int* obs) {
  const int a = ba_range_of(start, n_act, k);
  if (!(start[a] <= k && k < start[a + 1])) return -1;
  const int o = order[k];
  if (o < 0 || o >= N) return -1;
  if (key[o] != (int64_t)act[a]) return -1;
  if (k > 0 && k > start[a] && !(order[k - 1] < o)) return -1;
  *obs = o;
  return a;
}

__global__ __launch_bounds__(256) void ba_validate_kernel(BaArgs P) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const BaIndex& ix = P.ix;
  bool ok = true;
  if (k == 0) {
    ok = ix.head[0] == kBaMagic && ix.head[1] == P.N && ix.head[2] == P.C && ix.head[3] == P.P &&
         ix.head[4] == P.A && ix.head[5] == P.Pa;
    ok = ok && ix.cam_start[0] == 0 && ix.cam_start[P.A] == P.N;
    ok = ok && ix.pt_start[0] == 0 && ix.pt_start[P.Pa] == P.N;
  }
  if (k < P.A) {
    ok = ok && ix.cam_start[k] < ix.cam_start[k + 1];
    ok = ok && ix.act_cams[k] >= 0 && ix.act_cams[k] < P.C;
    ok = ok && (k == 0 || ix.act_cams[k - 1] < ix.act_cams[k]);
  }
  if (k < P.Pa) {
    ok = ok && ix.pt_start[k] < ix.pt_start[k + 1];
    ok = ok && ix.act_pts[k] >= 0 && ix.act_pts[k] < P.P;
    ok = ok && (k == 0 || ix.act_pts[k - 1] < ix.act_pts[k]);
  }
  if (k < P.N) {
    const int64_t pi = P.ptIdx[k], ci = P.camIdx[k];
    ok = ok && pi >= 0 && pi < P.P && ci >= 0 && ci < P.C;
    int o = 0;
    const int a = ba_check_slot(ix.cam_start, ix.cam_order, ix.act_cams, P.A, P.camIdx, P.N, k, &o);
    if (a >= 0) P.oacam[o] = a; else ok = false;
    const int q = ba_check_slot(ix.pt_start, ix.pt_order, ix.act_pts, P.Pa, P.ptIdx, P.N, k, &o);
    if (q >= 0) P.oapt[o] = q; else ok = false;
  }
  if (!ok) atomicOr(&P.st->bad, 1);
}

// Working copies of the active variables; a bad index ends the solve here
__global__ __launch_bounds__(256) void ba_gather_kernel(BaArgs P) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (P.st->bad) {
    if (e == 0) {
      P.st->done = 1;
      P.info[0] = (double)BA_BAD_INDEX;
    }
    return;
  }
  if (e < 6 * P.A) {
    P.camw[e] = P.cam_pose[6 * (int64_t)P.ix.act_cams[e / 6] + e % 6];
  } else if (e < 6 * P.A + 3 * P.Pa) {
    const int j = e - 6 * P.A;
    P.ptw[j] = P.points[3 * (int64_t)P.ix.act_pts[j / 3] + j % 3];
  }
}

__global__ __launch_bounds__(256) void ba_linearize_kernel(BaArgs P) {
  if (P.st->done || !P.st->need_lin) return;
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= P.N) return;
  double rr[2], jc[12], jp[6];
  ba_observe(P.camw + 6 * P.oacam[o], P.ptw + 3 * P.oapt[o], P.features + 5 * (int64_t)o, rr, jc,
             jp);
  P.r[2 * (int64_t)o] = rr[0];
  P.r[2 * (int64_t)o + 1] = rr[1];
  for (int i = 0; i < 12; ++i) P.Jc[12 * (int64_t)o + i] = jc[i];
  for (int i = 0; i < 6; ++i) P.Jp[6 * (int64_t)o + i] = jp[i];
  // W = Jc^T Jp, 6 x 3
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 3; ++j)
      P.W[18 * (int64_t)o + 3 * i + j] = jc[i] * jp[j] + jc[6 + i] * jp[3 + j];
}

__device__ __forceinline__ double ba_damp(double d, double mu) {
  return mu * fmin(fmax(d, 1e-6), 1e32);
}

// Blocks [0, A): one wave per active camera, U = sum Jc^T Jc (+ damping) and g_c = sum Jc^T r.
// Blocks from A: one thread per active point, V, g_p, damping, the Cholesky factor of the
// symmetric 3 x 3 and z = L^-1 g_p.
__global__ __launch_bounds__(64) void ba_reduce_kernel(BaArgs P) {
  if (P.st->done) return;
  const double mu = 1.0 / P.st->radius;
  const int lane = threadIdx.x;
  if ((int)blockIdx.x < P.A) {
    const int a = blockIdx.x;
    double u[21], g[6];
    for (int i = 0; i < 21; ++i) u[i] = 0.0;
    for (int i = 0; i < 6; ++i) g[i] = 0.0;
    for (int k = P.ix.cam_start[a] + lane; k < P.ix.cam_start[a + 1]; k += 64) {
      const int o = P.ix.cam_order[k];
      const double* jc = P.Jc + 12 * (int64_t)o;
      const double r0 = P.r[2 * (int64_t)o], r1 = P.r[2 * (int64_t)o + 1];
      int e = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        g[i] += jc[i] * r0 + jc[6 + i] * r1;
#pragma unroll
        for (int j = i; j < 6; ++j) u[e++] += jc[i] * jc[j] + jc[6 + i] * jc[6 + j];
      }
    }
#pragma unroll
    for (int i = 0; i < 21; ++i) u[i] = wave_sum_d(u[i]);
#pragma unroll
    for (int i = 0; i < 6; ++i) g[i] = wave_sum_d(g[i]);
    if (lane == 0) {
      int e = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        P.gc[6 * a + i] = g[i];
#pragma unroll
        for (int j = i; j < 6; ++j) {
          const double v = (i == j) ? u[e] + ba_damp(u[e], mu) : u[e];
          P.U[36 * a + 6 * i + j] = v;
          P.U[36 * a + 6 * j + i] = v;
          ++e;
        }
      }
    }
    return;
  }
  const int q = ((int)blockIdx.x - P.A) * 64 + lane;
  if (q >= P.Pa) return;
  double v00 = 0, v01 = 0, v02 = 0, v11 = 0, v12 = 0, v22 = 0, g0 = 0, g1 = 0, g2 = 0;
  for (int k = P.ix.pt_start[q]; k < P.ix.pt_start[q + 1]; ++k) {
    const int o = P.ix.pt_order[k];
    const double* jp = P.Jp + 6 * (int64_t)o;
    const double r0 = P.r[2 * (int64_t)o], r1 = P.r[2 * (int64_t)o + 1];
    v00 += jp[0] * jp[0] + jp[3] * jp[3];
    v01 += jp[0] * jp[1] + jp[3] * jp[4];
    v02 += jp[0] * jp[2] + jp[3] * jp[5];
    v11 += jp[1] * jp[1] + jp[4] * jp[4];
    v12 += jp[1] * jp[2] + jp[4] * jp[5];
    v22 += jp[2] * jp[2] + jp[5] * jp[5];
    g0 += jp[0] * r0 + jp[3] * r1;
    g1 += jp[1] * r0 + jp[4] * r1;
    g2 += jp[2] * r0 + jp[5] * r1;
  }
  v00 += ba_damp(v00, mu);
  v11 += ba_damp(v11, mu);
  v22 += ba_damp(v22, mu);
  // V = L L^T, column by column; z = L^-1 g_p.  V^-1 is never formed: a point seen by few
  // cameras has 1 / damping in every entry of its inverse, and products with it would lose that
  // factor in S.  The damped diagonal keeps every pivot positive.
  const double l00 = sqrt(v00), l10 = v01 / l00, l20 = v02 / l00;
  const double l11 = sqrt(v11 - l10 * l10), l21 = (v12 - l20 * l10) / l11;
  const double l22 = sqrt(v22 - l20 * l20 - l21 * l21);
  double* lv = P.Lv + 6 * (int64_t)q;
  lv[0] = l00;
  lv[1] = l10;
  lv[2] = l11;
  lv[3] = l20;
  lv[4] = l21;
  lv[5] = l22;
  const double z0 = g0 / l00, z1 = (g1 - l10 * z0) / l11;
  P.gp[3 * q] = z0;
  P.gp[3 * q + 1] = z1;
  P.gp[3 * q + 2] = (g2 - l20 * z0 - l21 * z1) / l22;
}

// Y_n = L^-1 W_n^T for the factor of n's point, stored as six 3-vectors (one per row of W_n):
// W V^-1 W^T = Y^T Y and W V^-1 g_p = Y^T z
__global__ __launch_bounds__(256) void ba_whiten_kernel(BaArgs P) {
  if (P.st->done) return;
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= P.N) return;
  const double* lv = P.Lv + 6 * (int64_t)P.oapt[o];
  const double l00 = lv[0], l10 = lv[1], l11 = lv[2], l20 = lv[3], l21 = lv[4], l22 = lv[5];
  for (int i = 0; i < 6; ++i) {
    const double* w = P.W + 18 * (int64_t)o + 3 * i;
    double* y = P.Y + 18 * (int64_t)o + 3 * i;
    const double y0 = w[0] / l00, y1 = (w[1] - l10 * y0) / l11;
    y[0] = y0;
    y[1] = y1;
    y[2] = (w[2] - l20 * y0 - l21 * y1) / l22;
  }
}

// Block row i of S = U - sum_p W V_p^-1 W^T (lower triangle: column blocks a <= i) and of
// rhs = -g_c + sum W V^-1 g_p.  One thread per output element, which it keeps in a register: it
// walks camera i's observations n in index order and, for each, the observation list of n's
// point in order, subtracting Y_n[r] . Y_m[c] (Y = L^-1 W^T, V = L L^T) where m lies in its column block.  Two
// observations of one (camera, point) pair meet in the same thread, one after the other.
__global__ __launch_bounds__(kBaSchurThreads) void ba_schur_kernel(BaArgs P) {
  if (P.st->done) return;
  const int i = blockIdx.x, e = blockIdx.y * kBaSchurThreads + threadIdx.x;
  const int n6 = 6 * P.A;
  if (e >= 36 * P.A + 6) return;
  const bool is_rhs = e >= 36 * P.A;
  const int a = is_rhs ? -1 : e / 36;
  const int r = is_rhs ? e - 36 * P.A : (e % 36) / 6, c = e % 6;
  if (!is_rhs && a > i) return;
  double acc = is_rhs ? -P.gc[6 * i + r] : (a == i ? P.U[36 * i + 6 * r + c] : 0.0);
  for (int k = P.ix.cam_start[i]; k < P.ix.cam_start[i + 1]; ++k) {
    const int n = P.ix.cam_order[k], q = P.oapt[n];
    const double* yn = P.Y + 18 * (int64_t)n + 3 * r;
    const double t0 = yn[0], t1 = yn[1], t2 = yn[2];
    if (is_rhs) {
      acc += t0 * P.gp[3 * q] + t1 * P.gp[3 * q + 1] + t2 * P.gp[3 * q + 2];
    } else {
      for (int kk = P.ix.pt_start[q]; kk < P.ix.pt_start[q + 1]; ++kk) {
        const int m = P.ix.pt_order[kk];
        if (P.oacam[m] != a) continue;
        const double* ym = P.Y + 18 * (int64_t)m + 3 * c;
        acc -= t0 * ym[0] + t1 * ym[1] + t2 * ym[2];
      }
    }
  }
  if (is_rhs) P.rhs[6 * i + r] = acc;
  else P.S[(int64_t)(6 * i + r) * n6 + 6 * a + c] = acc;
}

// Cholesky of S (n = 6 A <= 144) on its packed lower triangle in LDS, left-looking: thread r owns
// row r and computes L[r][k] from the columns before k, two barriers per column.  Then
// L y = rhs and L^T dc = y, column by column.  A pivot that is not > 0 (NaN included) sets
// chol_fail and leaves dc alone.
__global__ __launch_bounds__(kBaCholThreads) void ba_cholesky_kernel(BaArgs P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
  if (P.st->done) return;
  const int n = 6 * P.A, t = threadIdx.x;
  double* L = reinterpret_cast<double*>(dyn);   // n (n + 1) / 2
  double* y = L + n * (n + 1) / 2;              // n
  double* piv = y + n;                          // 1
  for (int idx = t; idx < n * n; idx += kBaCholThreads) {
    const int rr = idx / n, cc = idx % n;
    if (cc <= rr) L[rr * (rr + 1) / 2 + cc] = P.S[idx];
  }
  if (t < n) y[t] = P.rhs[t];
  __syncthreads();
  double* row = L + (t < n ? t * (t + 1) / 2 : 0);   // used by t < n only
  bool fail = false;
  for (int k = 0; k < n; ++k) {
    double v = 0.0;
    if (t >= k && t < n) {
      v = row[k];
      const double* rk = L + k * (k + 1) / 2;
      for (int j = 0; j < k; ++j) v -= row[j] * rk[j];
      if (t == k) *piv = v;
    }
    __syncthreads();
    const double d = *piv;
    if (!(d > 0.0)) {
      fail = true;
      break;   // uniform: every thread read the same pivot
    }
    const double sd = sqrt(d);
    if (t >= k && t < n) row[k] = (t == k) ? sd : v / sd;
    __syncthreads();
  }
  if (fail) {
    if (t == 0) P.st->chol_fail = 1;
    return;
  }
  for (int k = 0; k < n; ++k) {   // forward: y[k] final once columns < k are applied
    if (t == k) y[k] = y[k] / row[k];
    __syncthreads();
    if (t > k && t < n) y[t] -= row[k] * y[k];
    __syncthreads();
  }
  for (int k = n - 1; k >= 0; --k) {   // backward with row k of L as column k of L^T
    const double* rk = L + k * (k + 1) / 2;
    if (t == k) y[k] = y[k] / rk[k];
    __syncthreads();
    if (t < k) y[t] -= rk[t] * y[k];
    __syncthreads();
  }
  if (t < n) P.dc[t] = y[t];
  if (t == 0) P.st->chol_fail = 0;
}

// dp = V^-1 (-g_p - W^T dc) = L^-T (-z - sum Y dc) per active point, and the candidate variables
__global__ __launch_bounds__(256) void ba_update_kernel(BaArgs P) {
  if (P.st->done || P.st->chol_fail) return;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < P.Pa) {
    const int q = e;
    double b0 = -P.gp[3 * q], b1 = -P.gp[3 * q + 1], b2 = -P.gp[3 * q + 2];   // -z
    for (int kk = P.ix.pt_start[q]; kk < P.ix.pt_start[q + 1]; ++kk) {
      const int m = P.ix.pt_order[kk];
      const double* ym = P.Y + 18 * (int64_t)m;
      const double* d = P.dc + 6 * P.oacam[m];
      double s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) {
        s0 += ym[3 * rr] * d[rr];
        s1 += ym[3 * rr + 1] * d[rr];
        s2 += ym[3 * rr + 2] * d[rr];
      }
      b0 -= s0;
      b1 -= s1;
      b2 -= s2;
    }
    const double* lv = P.Lv + 6 * (int64_t)q;   // dp = L^-T b
    const double d2 = b2 / lv[5], d1 = (b1 - lv[4] * d2) / lv[2];
    const double dd[3] = {(b0 - lv[1] * d1 - lv[3] * d2) / lv[0], d1, d2};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      P.dp[3 * q + j] = dd[j];
      P.ptn[3 * q + j] = P.ptw[3 * q + j] + dd[j];
    }
  } else if (e < P.Pa + 6 * P.A) {
    const int j = e - P.Pa;
    P.camn[j] = P.camw[j] + P.dc[j];
  }
}

// Per observation: the candidate's cost term 1/2 |r'|^2 and the model decrease term
// -(J d) . (r + J d / 2).  initial: the cost term of the working copies alone.
__global__ __launch_bounds__(256) void ba_eval_kernel(BaArgs P, int initial) {
  if (P.st->done || (!initial && P.st->chol_fail)) return;
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= P.N) return;
  const int a = P.oacam[o], q = P.oapt[o];
  double rr[2];
  ba_observe((initial ? P.camw : P.camn) + 6 * a, (initial ? P.ptw : P.ptn) + 3 * q,
             P.features + 5 * (int64_t)o, rr, nullptr, nullptr);
  P.tcost[o] = 0.5 * (rr[0] * rr[0] + rr[1] * rr[1]);
  if (initial) return;
  const double* jc = P.Jc + 12 * (int64_t)o;
  const double* jp = P.Jp + 6 * (int64_t)o;
  const double* d = P.dc + 6 * a;
  const double* dq = P.dp + 3 * q;
  double j0 = 0, j1 = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    j0 += jc[i] * d[i];
    j1 += jc[6 + i] * d[i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    j0 += jp[i] * dq[i];
    j1 += jp[3 + i] * dq[i];
  }
  const double r0 = P.r[2 * (int64_t)o], r1 = P.r[2 * (int64_t)o + 1];
  P.tmd[o] = -(j0 * (r0 + 0.5 * j0) + j1 * (r1 + 0.5 * j1));
}

// One workgroup: the sums, the decision, the trust region, the info block, and on acceptance
// the candidate becomes the iterate (working copies and the caller's arrays).
__global__ __launch_bounds__(256) void ba_decide_kernel(BaArgs P, int initial) {
  __shared__ double lds[256];
  __shared__ int accept_s;
  BaState* st = P.st;
  const int t = threadIdx.x;
  const bool done = st->done, chol_fail = !initial && st->chol_fail;
  __syncthreads();   // every wave has read the state before thread 0 rewrites it below
  if (done) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double cand = nan, md = nan;
  if (!chol_fail) {
    cand = block_sum_256(P.tcost, P.N, lds);
    if (!initial) md = block_sum_256(P.tmd, P.N, lds);
  }
  if (initial) {
    if (t == 0) {
      P.info[3] = cand;
      P.info[4] = cand;
      P.info[5] = st->radius;
      if (isfinite(cand)) {
        st->cost = cand;
      } else {
        st->done = 1;
        P.info[0] = (double)BA_FAILED;
      }
    }
    return;
  }
  if (t == 0) {
    const double cost = st->cost, radius = st->radius;
    const double rho = chol_fail ? nan : (cost - cand) / md;
    const bool accept = !chol_fail && isfinite(cand) && md > 0.0 && rho > 1e-3;
    double* row = P.info + kBaInfoHead + kBaInfoRow * st->iter;
    row[0] = cost;
    row[1] = cand;
    row[2] = md;
    row[3] = rho;
    row[4] = radius;
    row[5] = accept ? 1.0 : 0.0;
    if (accept) {
      const double q = 2.0 * rho - 1.0;
      st->radius = fmin(radius / fmax(1.0 / 3.0, 1.0 - q * q * q), 1e16);
      st->factor = 2.0;
      st->cost = cand;
      st->succ += 1;
      st->need_lin = 1;
    } else {
      st->radius = radius / st->factor;
      st->factor *= 2.0;
      st->need_lin = 0;
    }
    st->iter += 1;
    st->chol_fail = 0;
    if (st->iter >= P.max_iters || st->succ >= P.max_success) st->done = 1;
    P.info[1] = (double)st->iter;
    P.info[2] = (double)st->succ;
    P.info[4] = st->cost;
    P.info[5] = st->radius;
    accept_s = accept ? 1 : 0;
  }
  __syncthreads();
  if (!accept_s) return;
  for (int e = t; e < 6 * P.A; e += 256) {
    const double v = P.camn[e];
    P.camw[e] = v;
    P.cam_pose[6 * (int64_t)P.ix.act_cams[e / 6] + e % 6] = v;
  }
  for (int e = t; e < 3 * P.Pa; e += 256) {
    const double v = P.ptn[e];
    P.ptw[e] = v;
    P.points[3 * (int64_t)P.ix.act_pts[e / 3] + e % 3] = v;
  }
}

// ---- triangulation -----------------------------------------------------------------------
// cv2.triangulatePoints as apply_triangulation uses it (ba_tracker.py:267-273), one thread per
// pair: the 4 x 4 DLT matrix A, the eigenvector of A^T A's smallest eigenvalue by cyclic Jacobi
// (as the reference's own _triangulatePy takes it from A^T A, :255-263), dehomogenised; then
// track_ba's filters (:556-571).
__device__ __forceinline__ void tri_reproject(const double* Pm, const double* X, double u, double v,
                                              double* err) {
  const double x = Pm[0] * X[0] + Pm[1] * X[1] + Pm[2] * X[2] + Pm[3];
  const double y = Pm[4] * X[0] + Pm[5] * X[1] + Pm[6] * X[2] + Pm[7];
  const double z = Pm[8] * X[0] + Pm[9] * X[1] + Pm[10] * X[2] + Pm[11];
  const double du = x / z - u, dv = y / z - v;
  *err = sqrt(du * du + dv * dv);
}

__global__ __launch_bounds__(64) void triangulate_kernel(const double* P1, const double* P2,
                                                         const double* pts1, const double* pts2,
                                                         int n, double rep_thr, double z_max,
                                                         double* X, double* err1, double* err2,
                                                         double* zo, uint8_t* keep) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const double u1 = pts1[2 * (int64_t)i], v1 = pts1[2 * (int64_t)i + 1];
  const double u2 = pts2[2 * (int64_t)i], v2 = pts2[2 * (int64_t)i + 1];
  double A[4][4], M[4][4], V[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    A[0][j] = u1 * P1[8 + j] - P1[j];
    A[1][j] = v1 * P1[8 + j] - P1[4 + j];
    A[2][j] = u2 * P2[8 + j] - P2[j];
    A[3][j] = v2 * P2[8 + j] - P2[4 + j];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      M[r][c] = A[0][r] * A[0][c] + A[1][r] * A[1][c] + A[2][r] * A[2][c] + A[3][r] * A[3][c];
      V[r][c] = r == c ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 24; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = M[p][q];
        if (fabs(apq) <= 1e-20 * sqrt(fabs(M[p][p] * M[q][q])) || apq == 0.0) {
          M[p][q] = M[q][p] = 0.0;
          continue;
        }
        rotated = true;
        const double theta = (M[q][q] - M[p][p]) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // M <- M G
          const double mkp = M[k][p], mkq = M[k][q];
          M[k][p] = cs * mkp - sn * mkq;
          M[k][q] = sn * mkp + cs * mkq;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // M <- G^T M
          const double mpk = M[p][k], mqk = M[q][k];
          M[p][k] = cs * mpk - sn * mqk;
          M[q][k] = sn * mpk + cs * mqk;
        }
        M[p][q] = M[q][p] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = cs * vkp - sn * vkq;
          V[k][q] = sn * vkp + cs * vkq;
        }
      }
    if (!rotated) break;
  }
  double best = M[0][0], h0 = V[0][0], h1 = V[1][0], h2 = V[2][0], h3 = V[3][0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (M[j][j] < best) {
      best = M[j][j];
      h0 = V[0][j];
      h1 = V[1][j];
      h2 = V[2][j];
      h3 = V[3][j];
    }
  const double Xw[3] = {h0 / h3, h1 / h3, h2 / h3};
  double e1, e2;
  tri_reproject(P1, Xw, u1, v1, &e1);
  tri_reproject(P2, Xw, u2, v2, &e2);
  const bool fin = h3 != 0.0 && isfinite(Xw[0]) && isfinite(Xw[1]) && isfinite(Xw[2]) &&
                   isfinite(e1) && isfinite(e2);
  X[3 * (int64_t)i] = Xw[0];
  X[3 * (int64_t)i + 1] = Xw[1];
  X[3 * (int64_t)i + 2] = Xw[2];
  err1[i] = e1;
  err2[i] = e2;
  zo[i] = Xw[2];
  keep[i] = (fin && e1 <= rep_thr && e2 <= rep_thr && Xw[2] <= z_max) ? 1 : 0;
}

bool ba_dims_ok(int64_t N, int C, int P) {
  return N >= 1 && N <= kBaMaxObs && C >= 1 && C <= kBaMaxVars && P >= 1 && P <= kBaMaxVars;
}

}  // namespace
}  // namespace onepose

using namespace onepose;

extern "C" {

int onepose_ba_version(void) { return kBaVersion; }
int onepose_ba_max_active_cameras(void) { return kBaMaxActive; }

size_t onepose_ba_index_bytes(int64_t n_obs, int n_cams, int n_points) {
  if (!ba_dims_ok(n_obs, n_cams, n_points)) return 0;
  return ba_index_layout(nullptr, n_obs, n_cams, n_points).bytes;
}

int onepose_ba_build_index(const int64_t* ptIdx, const int64_t* camIdx, int64_t n_obs, int n_cams,
                           int n_points, void* index, size_t index_bytes, int* n_active_cams,
                           int* n_active_points) {
  clear_error();
  OP_REQUIRE(ptIdx && camIdx && index && n_active_cams && n_active_points,
             "ba_build_index: null pointer");
  OP_REQUIRE(ba_dims_ok(n_obs, n_cams, n_points),
             "ba_build_index: n_obs = %lld, n_cams = %d, n_points = %d, need 1..%lld, 1..%d, 1..%d",
             (long long)n_obs, n_cams, n_points, (long long)kBaMaxObs, kBaMaxVars, kBaMaxVars);
  const BaIndex ix = ba_index_layout(index, n_obs, n_cams, n_points);
  if (index_bytes < ix.bytes) {
    set_error("ba_build_index: index buffer of %zu bytes, %zu needed", index_bytes, ix.bytes);
    return ONEPOSE_ERR_WORKSPACE;
  }
  const int N = (int)n_obs;
  for (int o = 0; o < N; ++o)
    OP_REQUIRE(ptIdx[o] >= 0 && ptIdx[o] < n_points && camIdx[o] >= 0 && camIdx[o] < n_cams,
               "ba_build_index: observation %d names point %lld, camera %lld (of %d, %d)", o,
               (long long)ptIdx[o], (long long)camIdx[o], n_points, n_cams);
  std::memset(index, 0, ix.bytes);
  // one stable counting sort per side; slot[] maps an id to its active slot
  auto side = [N](const int64_t* key, int n_ids, int* act, int* start, int* order) {
    std::vector<int> count(n_ids, 0), slot(n_ids, -1);
    for (int o = 0; o < N; ++o) ++count[key[o]];
    int n_act = 0;
    start[0] = 0;
    for (int id = 0; id < n_ids; ++id)
      if (count[id] > 0) {
        slot[id] = n_act;
        act[n_act] = id;
        start[n_act + 1] = start[n_act] + count[id];
        ++n_act;
      }
    std::vector<int> fill(start, start + n_act);
    for (int o = 0; o < N; ++o) order[fill[slot[key[o]]]++] = o;
    return n_act;
  };
  const int A = side(camIdx, n_cams, const_cast<int*>(ix.act_cams),
                     const_cast<int*>(ix.cam_start), const_cast<int*>(ix.cam_order));
  const int Pa = side(ptIdx, n_points, const_cast<int*>(ix.act_pts),
                      const_cast<int*>(ix.pt_start), const_cast<int*>(ix.pt_order));
  int* head = const_cast<int*>(ix.head);
  head[0] = kBaMagic;
  head[1] = N;
  head[2] = n_cams;
  head[3] = n_points;
  head[4] = A;
  head[5] = Pa;
  *n_active_cams = A;
  *n_active_points = Pa;
  return ONEPOSE_OK;
}

size_t onepose_ba_workspace_bytes(int64_t n_obs, int n_active_cams, int n_active_points) {
  if (n_obs < 1 || n_obs > kBaMaxObs || n_active_cams < 1 || n_active_cams > kBaMaxActive ||
      n_active_points < 1 || n_active_points > kBaMaxVars)
    return 0;
  BaArgs a{};
  a.N = (int)n_obs;
  a.A = n_active_cams;
  a.Pa = n_active_points;
  size_t bytes = 0;
  ba_carve(a, nullptr, &bytes);
  return bytes;
}

int onepose_ba_solve(double* points, double* cam_pose, const double* features,
                     const int64_t* ptIdx, const int64_t* camIdx, const void* index,
                     int64_t n_obs, int n_cams, int n_points, int n_active_cams,
                     int n_active_points, int max_iters, int max_success, double initial_radius,
                     double* info, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  OP_REQUIRE(points && cam_pose && features && ptIdx && camIdx && index && info && workspace,
             "ba_solve: null pointer (variables, features, indices, index, info and workspace "
             "are all required)");
  OP_REQUIRE(ba_dims_ok(n_obs, n_cams, n_points) && n_active_cams >= 1 &&
                 n_active_cams <= n_cams && n_active_points >= 1 && n_active_points <= n_points &&
                 (int64_t)n_active_cams <= n_obs && (int64_t)n_active_points <= n_obs,
             "ba_solve: shape n_obs = %lld, n_cams = %d, n_points = %d, active %d / %d",
             (long long)n_obs, n_cams, n_points, n_active_cams, n_active_points);
  OP_REQUIRE(n_active_cams <= kBaMaxActive, "ba_solve: %d active cameras, at most %d",
             n_active_cams, kBaMaxActive);
  OP_REQUIRE(max_iters >= 1 && max_iters <= kBaMaxIters, "ba_solve: max_iters = %d, need 1..%d",
             max_iters, kBaMaxIters);
  OP_REQUIRE(max_success >= 1, "ba_solve: max_success = %d, need >= 1", max_success);
  OP_REQUIRE(initial_radius > 0.0 && std::isfinite(initial_radius),
             "ba_solve: initial_radius %g is not a positive finite number", initial_radius);
  BaArgs a{};
  a.points = points;
  a.cam_pose = cam_pose;
  a.features = features;
  a.ptIdx = ptIdx;
  a.camIdx = camIdx;
  a.ix = ba_index_layout(index, n_obs, n_cams, n_points);
  a.N = (int)n_obs;
  a.C = n_cams;
  a.P = n_points;
  a.A = n_active_cams;
  a.Pa = n_active_points;
  a.max_iters = max_iters;
  a.max_success = max_success;
  a.radius0 = initial_radius;
  a.info = info;
  size_t need = 0;
  ba_carve(a, workspace, &need);
  if (workspace_bytes < need) {
    set_error("ba_solve: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    return ONEPOSE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int n6 = 6 * a.A;
  const size_t chol_lds = ((size_t)n6 * (n6 + 1) / 2 + n6 + 2) * sizeof(double);
  static bool attr_set = false;
  if (!attr_set) {
    OP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ba_cholesky_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(((size_t)6 * kBaMaxActive * (6 * kBaMaxActive + 1) / 2 +
                                      6 * kBaMaxActive + 2) * sizeof(double))));
    attr_set = true;
  }
  const int obs_blocks = ceil_div(a.N, 256);
  const int most = a.N > a.Pa ? a.N : a.Pa;
  hipLaunchKernelGGL(ba_init_kernel, dim3(1), dim3(128), 0, st, a);
  OP_LAUNCHED();
  hipLaunchKernelGGL(ba_validate_kernel, dim3(ceil_div(most + 1, 256)), dim3(256), 0, st, a);
  OP_LAUNCHED();
  hipLaunchKernelGGL(ba_gather_kernel, dim3(ceil_div(6 * a.A + 3 * a.Pa, 256)), dim3(256), 0, st,
                     a);
  OP_LAUNCHED();
  hipLaunchKernelGGL(ba_eval_kernel, dim3(obs_blocks), dim3(256), 0, st, a, 1);
  OP_LAUNCHED();
  hipLaunchKernelGGL(ba_decide_kernel, dim3(1), dim3(256), 0, st, a, 1);
  OP_LAUNCHED();
  for (int it = 0; it < max_iters; ++it) {
    hipLaunchKernelGGL(ba_linearize_kernel, dim3(obs_blocks), dim3(256), 0, st, a);
    OP_LAUNCHED();
    hipLaunchKernelGGL(ba_reduce_kernel, dim3(a.A + ceil_div(a.Pa, 64)), dim3(64), 0, st, a);
    OP_LAUNCHED();
    hipLaunchKernelGGL(ba_whiten_kernel, dim3(obs_blocks), dim3(256), 0, st, a);
    OP_LAUNCHED();
    hipLaunchKernelGGL(ba_schur_kernel, dim3(a.A, ceil_div(36 * a.A + 6, kBaSchurThreads)),
                       dim3(kBaSchurThreads), 0, st, a);
    OP_LAUNCHED();
    hipLaunchKernelGGL(ba_cholesky_kernel, dim3(1), dim3(kBaCholThreads), chol_lds, st, a);
    OP_LAUNCHED();
    hipLaunchKernelGGL(ba_update_kernel, dim3(ceil_div(a.Pa + 6 * a.A, 256)), dim3(256), 0, st, a);
    OP_LAUNCHED();
    hipLaunchKernelGGL(ba_eval_kernel, dim3(obs_blocks), dim3(256), 0, st, a, 0);
    OP_LAUNCHED();
    hipLaunchKernelGGL(ba_decide_kernel, dim3(1), dim3(256), 0, st, a, 0);
    OP_LAUNCHED();
  }
  return ONEPOSE_OK;
}

int onepose_ba_linearize(const double* points, const double* cam_pose, const double* features,
                         const int64_t* ptIdx, const int64_t* camIdx, int64_t n_obs, int n_cams,
                         int n_points, double* residuals, double* Jc, double* Jp, double* cost,
                         void* stream) {
  clear_error();
  OP_REQUIRE(points && cam_pose && features && ptIdx && camIdx && residuals && Jc && Jp && cost,
             "ba_linearize: null pointer");
  OP_REQUIRE(ba_dims_ok(n_obs, n_cams, n_points),
             "ba_linearize: shape n_obs = %lld, n_cams = %d, n_points = %d", (long long)n_obs,
             n_cams, n_points);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int N = (int)n_obs;
  hipLaunchKernelGGL(ba_linearize_plain_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, st, points,
                     cam_pose, features, ptIdx, camIdx, N, n_cams, n_points, residuals, Jc, Jp);
  OP_LAUNCHED();
  hipLaunchKernelGGL(ba_cost_kernel, dim3(1), dim3(256), 0, st, residuals, 2 * N, cost);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

int onepose_triangulate(const double* P1, const double* P2, const double* pts1,
                        const double* pts2, int n, double rep_thr, double z_max, double* X,
                        double* err1, double* err2, double* z, uint8_t* keep, void* stream) {
  clear_error();
  OP_REQUIRE(P1 && P2 && pts1 && pts2 && X && err1 && err2 && z && keep,
             "triangulate: null pointer");
  OP_REQUIRE(n >= 1 && n <= (1 << 24), "triangulate: n = %d, need 1..%d", n, 1 << 24);
  OP_REQUIRE(rep_thr == rep_thr && z_max == z_max, "triangulate: NaN threshold");
  hipLaunchKernelGGL(triangulate_kernel, dim3(ceil_div(n, 64)), dim3(64), 0,
                     static_cast<hipStream_t>(stream), P1, P2, pts1, pts2, n, rep_thr, z_max, X,
                     err1, err2, z, keep);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

}  // extern "C"
