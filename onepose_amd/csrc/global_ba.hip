// Global bundle adjustment of an SfM model on gfx950 (include/onepose_global_ba.h): Ceres-style
// Levenberg-Marquardt whose camera step comes from preconditioned CG on the implicit Schur
// complement, all fp64.  The cost function is the tracker family's (ba.hip, ba_observe) with a
// focal length per axis, restated here so that ba.hip stays as it is; the index is that of
// onepose_ba_build_index and its device-side validation is restated too.
//
// Launches (every kernel returns at once unless the workspace holds a live state of these shapes,
// so the sequence is fixed and graph-capturable; every decision lives on the device):
//   begin: init, validate, gather, eval(initial), decide(initial)
//   step, per outer iteration: linearize -> point (V = L L^T, g_p, z_p) -> camera (U, g_c, the
//   preconditioner block and its factor, rhs, CG start) -> cg_start (rz_0) ->
//   pcg_max_iters x [cg_point (y_p) -> cg_camera (S p, p . S p per camera) -> cg_update] ->
//   update (dp and the candidate) -> eval -> decide.
// No floating-point atomics; the order of every sum is stated in the header.
#include <cmath>

#include "common.h"

namespace onepose {
namespace {

constexpr int kGbaVersion = 1;
constexpr int kGbaMaxCams = 4096;           // active cameras
constexpr int64_t kGbaMaxObs = 1 << 20;
constexpr int kGbaMaxVars = 1 << 20;        // cameras, points
constexpr int kGbaMaxSteps = 1024, kGbaMaxPcg = 500, kGbaMaxInfoRows = 65536;
constexpr int kGbaInfoHead = 8, kGbaInfoRow = 8;
constexpr int kGbaIndexMagic = 0x42413031;  // onepose_ba_build_index's "BA01"
constexpr int kGbaIndexHeader = 8;
constexpr int kGbaStateMagic = 0x47424131;  // "GBA1"
constexpr double kGbaSeriesTh2 = 1e-4;
constexpr double kGbaMinRadius = 1e-32;
enum { GBA_OK = 0, GBA_FAILED = 1, GBA_BAD_INDEX = 2, GBA_CONVERGED = 3, GBA_MIN_RADIUS = 4 };
enum { CG_TOL = 1, CG_CAP = 2, CG_INDEFINITE = 3, CG_NONFINITE = 4, CG_ZERO_RHS = 5 };

struct GbaState {
  double radius, factor, cost, rz, rz0, cg_total;
  int magic, n, a, pa;
  int done, status, iter, succ, need_lin, bad, lin_fail, cg_done, cg_iters, cg_reason, pad0, pad1;
};

// The index as onepose_ba_build_index lays it out, located from (N, C, P) alone
struct GbaIndex {
  const int *head, *act_cams, *act_pts, *cam_start, *pt_start, *cam_order, *pt_order;
};
GbaIndex gba_index_layout(const void* base, int64_t N, int C, int P) {
  const int* p = static_cast<const int*>(base);
  GbaIndex ix;
  size_t off = 0;
  auto take = [&](size_t n) {
    const int* q = p + off;
    off += n;
    return q;
  };
  ix.head = take(kGbaIndexHeader);
  ix.act_cams = take(C);
  ix.act_pts = take(P);
  ix.cam_start = take((size_t)C + 1);
  ix.pt_start = take((size_t)P + 1);
  ix.cam_order = take(N);
  ix.pt_order = take(N);
  return ix;
}

struct GbaArgs {
  double *points, *cam_pose;
  const double *K4, *xy;
  const int64_t *ptIdx, *camIdx;
  const uint8_t* fixed;
  GbaIndex ix;
  int N, C, P, A, Pa;
  int info_rows, pcg_max;
  double radius0, pcg_tol, ftol;
  double* info;
  GbaState* st;
  double *r, *Jc, *Jp, *tcost, *tmd;        // per observation
  int *oacam, *oapt, *fixa;                 // observation -> active slot; active camera -> mask
  double *U, *Mc, *gc, *rhs, *x, *res, *z, *p, *Sp, *camdot;   // per active camera
  double *Lv, *gp, *zp, *yp, *dp;           // per active point
  double *camw, *ptw, *camn, *ptn;
};

void gba_carve(GbaArgs& a, void* ws, size_t* bytes) {
  Carve cv(ws);
  const size_t N = a.N, A = a.A, Pa = a.Pa;
  a.st = cv.take<GbaState>(1);
  a.r = cv.take<double>(2 * N);
  a.Jc = cv.take<double>(12 * N);
  a.Jp = cv.take<double>(6 * N);
  a.tcost = cv.take<double>(N);
  a.tmd = cv.take<double>(N);
  a.oacam = cv.take<int>(N);
  a.oapt = cv.take<int>(N);
  a.fixa = cv.take<int>(A);
  a.U = cv.take<double>(36 * A);
  a.Mc = cv.take<double>(21 * A);
  a.gc = cv.take<double>(6 * A);
  a.rhs = cv.take<double>(6 * A);
  a.x = cv.take<double>(6 * A);
  a.res = cv.take<double>(6 * A);
  a.z = cv.take<double>(6 * A);
  a.p = cv.take<double>(6 * A);
  a.Sp = cv.take<double>(6 * A);
  a.camdot = cv.take<double>(A);
  a.Lv = cv.take<double>(6 * Pa);
  a.gp = cv.take<double>(3 * Pa);
  a.zp = cv.take<double>(3 * Pa);
  a.yp = cv.take<double>(3 * Pa);
  a.dp = cv.take<double>(3 * Pa);
  a.camw = cv.take<double>(6 * A);
  a.ptw = cv.take<double>(3 * Pa);
  a.camn = cv.take<double>(6 * A);
  a.ptn = cv.take<double>(3 * Pa);
  *bytes = align_up(cv.off, 256);
}

// A live state of these shapes: written by this call sequence's init kernel and not yet stopped
__device__ __forceinline__ bool gba_live(const GbaArgs& P) {
  const GbaState* s = P.st;
  return s->magic == kGbaStateMagic && s->n == P.N && s->a == P.A && s->pa == P.Pa && !s->done;
}

// ---- the cost function ------------------------------------------------------------------
// One observation: cam = (angle-axis, t), X, k4 = (fx, fy, cx, cy), uv.  Jc (2 x 6, row-major)
// and Jp (2 x 3) may be null.  The tracker family's ba_observe operation by operation, with fx
// in row 0 and fy in row 1 of D = d r / d p.
__device__ __forceinline__ void gba_observe(const double* cam, const double* X, const double* k4,
                                            const double* uv, double* r, double* Jc, double* Jp) {
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
  const double fx = k4[0], fy = k4[1];
  const double xp = p0 / p2, yp = p1 / p2;
  r[0] = (fx * xp + k4[2]) - uv[0];
  r[1] = (fy * yp + k4[3]) - uv[1];
  if (Jc == nullptr) return;
  const double iz = 1.0 / p2;
  const double D00 = fx * iz, D02 = -fx * xp * iz, D11 = fy * iz, D12 = -fy * yp * iz;
  const double w[3] = {w0, w1, w2}, x[3] = {x0, x1, x2}, wx[3] = {wx0, wx1, wx2};
  double R[3][3], M[3][3];
  const double Xx[3][3] = {{0.0, -x2, x1}, {x2, 0.0, -x0}, {-x1, x0, 0.0}};
  const double Wx[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
  if (th2 > 0.0) {
    double b, ca, ab;
    if (th2 >= kGbaSeriesTh2) {
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

__device__ __forceinline__ void gba_zero_fixed(double* jc, int mask) {
#pragma unroll
  for (int j = 0; j < 6; ++j)
    if (mask >> j & 1) {
      jc[j] = 0.0;
      jc[6 + j] = 0.0;
    }
}

// Fixed-order sum of v[0 .. n) by one workgroup of 256: thread t adds v[t], v[t + 256], ... in
// order, then a halving tree over the 256 partial sums.  Every thread returns the total.
__device__ __forceinline__ double gba_block_sum(const double* v, int n, double* lds) {
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
  const double total = lds[0];
  __syncthreads();
  return total;
}

__device__ __forceinline__ double gba_damp(double d, double mu) {
  return mu * fmin(fmax(d, 1e-6), 1e32);
}

// x = (C C^T)^-1 b for the packed lower factor C (row i at i (i + 1) / 2)
__device__ __forceinline__ void gba_solve6(const double* C, const double* b, double* x) {
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= C[i * (i + 1) / 2 + k] * y[k];
    y[i] = v / C[i * (i + 1) / 2 + i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) v -= C[k * (k + 1) / 2 + i] * x[k];
    x[i] = v / C[i * (i + 1) / 2 + i];
  }
}

// L^-1 b and L^-T b for the packed 3 x 3 factor (l00, l10, l11, l20, l21, l22)
__device__ __forceinline__ void gba_fwd3(const double* lv, const double* b, double* y) {
  y[0] = b[0] / lv[0];
  y[1] = (b[1] - lv[1] * y[0]) / lv[2];
  y[2] = (b[2] - lv[3] * y[0] - lv[4] * y[1]) / lv[5];
}
__device__ __forceinline__ void gba_bwd3(const double* lv, const double* y, double* x) {
  x[2] = y[2] / lv[5];
  x[1] = (y[1] - lv[4] * x[2]) / lv[2];
  x[0] = (y[0] - lv[1] * x[1] - lv[3] * x[2]) / lv[0];
}

// ---- stand-alone linearisation ------------------------------------------------------------
__global__ __launch_bounds__(256) void gba_linearize_plain_kernel(
    const double* points, const double* cam_pose, const double* K4, const double* xy,
    const int64_t* ptIdx, const int64_t* camIdx, const uint8_t* fixed, int N, int C, int P,
    double* r, double* Jc, double* Jp) {
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
    gba_observe(cam_pose + 6 * ci, points + 3 * pi, K4 + 4 * ci, xy + 2 * (int64_t)o, rr, jc, jp);
    if (fixed != nullptr) gba_zero_fixed(jc, fixed[ci] & 63);
  }
  r[2 * (int64_t)o] = rr[0];
  r[2 * (int64_t)o + 1] = rr[1];
  for (int i = 0; i < 12; ++i) Jc[12 * (int64_t)o + i] = jc[i];
  for (int i = 0; i < 6; ++i) Jp[6 * (int64_t)o + i] = jp[i];
}

// cost = 1/2 sum r^2 over the 2 N residual entries, in gba_block_sum's order on r^2
__global__ __launch_bounds__(256) void gba_cost_kernel(const double* r, int n2, double* cost) {
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

// ---- begin ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gba_init_kernel(GbaArgs P) {
  const int t = threadIdx.x;
  const int n = kGbaInfoHead + kGbaInfoRow * P.info_rows;
  for (int i = t; i < n; i += 256) P.info[i] = 0.0;
  if (t == 0) {
    GbaState s;
    s.radius = P.radius0;
    s.factor = 2.0;
    s.cost = s.rz = s.rz0 = s.cg_total = 0.0;
    s.magic = kGbaStateMagic;
    s.n = P.N;
    s.a = P.A;
    s.pa = P.Pa;
    s.done = s.status = s.iter = s.succ = s.bad = s.lin_fail = s.cg_iters = s.cg_reason = 0;
    s.pad0 = s.pad1 = 0;
    s.need_lin = 1;
    s.cg_done = 1;
    *P.st = s;
  }
}

// largest a in [0, n) with start[a] <= k, whatever start holds (reads stay inside start[0 .. n))
__device__ __forceinline__ int gba_range_of(const int* start, int n, int k) {
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
__device__ __forceinline__ int gba_check_slot(const int* start, const int* order, const int* act,
                                              int n_act, const int64_t* key, int N, int k,
                                              int* obs) {
  const int a = gba_range_of(start, n_act, k);
  if (!(start[a] <= k && k < start[a + 1])) return -1;
  const int o = order[k];
  if (o < 0 || o >= N) return -1;
  if (key[o] != (int64_t)act[a]) return -1;
  if (k > 0 && k > start[a] && !(order[k - 1] < o)) return -1;
  *obs = o;
  return a;
}

__global__ __launch_bounds__(256) void gba_validate_kernel(GbaArgs P) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const GbaIndex& ix = P.ix;
  bool ok = true;
  if (k == 0) {
    ok = ix.head[0] == kGbaIndexMagic && ix.head[1] == P.N && ix.head[2] == P.C &&
         ix.head[3] == P.P && ix.head[4] == P.A && ix.head[5] == P.Pa;
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
    const int a = gba_check_slot(ix.cam_start, ix.cam_order, ix.act_cams, P.A, P.camIdx, P.N, k, &o);
    if (a >= 0) P.oacam[o] = a; else ok = false;
    const int q = gba_check_slot(ix.pt_start, ix.pt_order, ix.act_pts, P.Pa, P.ptIdx, P.N, k, &o);
    if (q >= 0) P.oapt[o] = q; else ok = false;
  }
  if (!ok) atomicOr(&P.st->bad, 1);
}

// Working copies of the active variables and masks; a bad index ends the solve here
__global__ __launch_bounds__(256) void gba_gather_kernel(GbaArgs P) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (P.st->bad) {
    if (e == 0) {
      P.st->done = 1;
      P.st->status = GBA_BAD_INDEX;
      P.info[0] = (double)GBA_BAD_INDEX;
    }
    return;
  }
  if (e < 6 * P.A) {
    const int id = P.ix.act_cams[e / 6];
    P.camw[e] = P.cam_pose[6 * (int64_t)id + e % 6];
    if (e % 6 == 0) P.fixa[e / 6] = P.fixed ? (P.fixed[id] & 63) : 0;
  } else if (e < 6 * P.A + 3 * P.Pa) {
    const int j = e - 6 * P.A;
    P.ptw[j] = P.points[3 * (int64_t)P.ix.act_pts[j / 3] + j % 3];
  }
}

// ---- one outer iteration --------------------------------------------------------------------
__global__ __launch_bounds__(256) void gba_linearize_kernel(GbaArgs P) {
  if (!gba_live(P) || !P.st->need_lin) return;
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= P.N) return;
  const int a = P.oacam[o];
  double rr[2], jc[12], jp[6];
  gba_observe(P.camw + 6 * a, P.ptw + 3 * P.oapt[o], P.K4 + 4 * (int64_t)P.ix.act_cams[a],
              P.xy + 2 * (int64_t)o, rr, jc, jp);
  gba_zero_fixed(jc, P.fixa[a]);
  P.r[2 * (int64_t)o] = rr[0];
  P.r[2 * (int64_t)o + 1] = rr[1];
  for (int i = 0; i < 12; ++i) P.Jc[12 * (int64_t)o + i] = jc[i];
  for (int i = 0; i < 6; ++i) P.Jp[6 * (int64_t)o + i] = jp[i];
}

// One thread per active point: V, g_p, damping, V = L L^T, z = L^-1 g_p
__global__ __launch_bounds__(64) void gba_point_kernel(GbaArgs P) {
  if (!gba_live(P)) return;
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= P.Pa) return;
  const double mu = 1.0 / P.st->radius;
  double v00 = 0, v01 = 0, v02 = 0, v11 = 0, v12 = 0, v22 = 0, g[3] = {0, 0, 0};
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
    g[0] += jp[0] * r0 + jp[3] * r1;
    g[1] += jp[1] * r0 + jp[4] * r1;
    g[2] += jp[2] * r0 + jp[5] * r1;
  }
  v00 += gba_damp(v00, mu);
  v11 += gba_damp(v11, mu);
  v22 += gba_damp(v22, mu);
  double lv[6], z[3];
  const double d1 = v00;
  lv[0] = sqrt(d1);
  lv[1] = v01 / lv[0];
  lv[3] = v02 / lv[0];
  const double d2 = v11 - lv[1] * lv[1];
  lv[2] = sqrt(d2);
  lv[4] = (v12 - lv[3] * lv[1]) / lv[2];
  const double d3 = v22 - lv[3] * lv[3] - lv[4] * lv[4];
  lv[5] = sqrt(d3);
  if (!(d1 > 0.0) || !(d2 > 0.0) || !(d3 > 0.0)) atomicOr(&P.st->lin_fail, 1);
  gba_fwd3(lv, g, z);
#pragma unroll
  for (int i = 0; i < 6; ++i) P.Lv[6 * (int64_t)q + i] = lv[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    P.gp[3 * q + i] = g[i];
    P.zp[3 * q + i] = z[i];
  }
}

// One wave per active camera: U, g_c, M_c = U_c - sum Y^T Y and its factor, rhs, and the start
// of CG (x = 0, res = rhs, z = M^-1 res, p = z, this camera's res . z)
__global__ __launch_bounds__(64) void gba_camera_kernel(GbaArgs P) {
  if (!gba_live(P) || P.st->lin_fail) return;
  const double mu = 1.0 / P.st->radius;
  const int lane = threadIdx.x, a = blockIdx.x;
  double u[21], m[21], g[6], h[6];
#pragma unroll
  for (int i = 0; i < 21; ++i) u[i] = m[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) g[i] = h[i] = 0.0;
  for (int k = P.ix.cam_start[a] + lane; k < P.ix.cam_start[a + 1]; k += 64) {
    const int o = P.ix.cam_order[k], q = P.oapt[o];
    const double* jc = P.Jc + 12 * (int64_t)o;
    const double* jp = P.Jp + 6 * (int64_t)o;
    const double* lv = P.Lv + 6 * (int64_t)q;
    const double* zq = P.zp + 3 * (int64_t)q;
    const double r0 = P.r[2 * (int64_t)o], r1 = P.r[2 * (int64_t)o + 1];
    double y[6][3];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double w[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) w[j] = jc[i] * jp[j] + jc[6 + i] * jp[3 + j];
      gba_fwd3(lv, w, y[i]);
    }
    int e = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      g[i] += jc[i] * r0 + jc[6 + i] * r1;
      h[i] += y[i][0] * zq[0] + y[i][1] * zq[1] + y[i][2] * zq[2];
#pragma unroll
      for (int j = i; j < 6; ++j) {
        u[e] += jc[i] * jc[j] + jc[6 + i] * jc[6 + j];
        m[e] += y[i][0] * y[j][0] + y[i][1] * y[j][1] + y[i][2] * y[j][2];
        ++e;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 21; ++i) {
    u[i] = wave_sum_d(u[i]);
    m[i] = wave_sum_d(m[i]);
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    g[i] = wave_sum_d(g[i]);
    h[i] = wave_sum_d(h[i]);
  }
  if (lane != 0) return;
  const int mask = P.fixa[a];
  double M[6][6], C[21], b[6], z[6];
  int e = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) {
      double v = u[e];
      if (i == j) {
        v += gba_damp(v, mu);
        if (mask >> i & 1) v = 1.0;
      }
      P.U[36 * a + 6 * i + j] = v;
      P.U[36 * a + 6 * j + i] = v;
      M[i][j] = M[j][i] = v - m[e];
      ++e;
    }
  bool fail = false;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = M[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= C[j * (j + 1) / 2 + k] * C[j * (j + 1) / 2 + k];
    if (!(d > 0.0)) fail = true;
    const double sd = sqrt(d);
    C[j * (j + 1) / 2 + j] = sd;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = M[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= C[i * (i + 1) / 2 + k] * C[j * (j + 1) / 2 + k];
      C[i * (i + 1) / 2 + j] = v / sd;
    }
  }
  if (fail) {
    atomicOr(&P.st->lin_fail, 1);
    return;
  }
#pragma unroll
  for (int i = 0; i < 21; ++i) P.Mc[21 * a + i] = C[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) b[i] = -g[i] + h[i];
  gba_solve6(C, b, z);
  double dot = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    P.gc[6 * a + i] = g[i];
    P.rhs[6 * a + i] = b[i];
    P.x[6 * a + i] = 0.0;
    P.res[6 * a + i] = b[i];
    P.z[6 * a + i] = z[i];
    P.p[6 * a + i] = z[i];
    dot += b[i] * z[i];
  }
  P.camdot[a] = dot;
}

// rz_0 and the CG state of this iteration
__global__ __launch_bounds__(256) void gba_cg_start_kernel(GbaArgs P) {
  __shared__ double lds[256];
  if (!gba_live(P) || P.st->lin_fail) return;
  const double rz0 = gba_block_sum(P.camdot, P.A, lds);
  if (threadIdx.x == 0) {
    GbaState* st = P.st;
    st->rz = st->rz0 = rz0;
    st->cg_iters = 0;
    st->cg_done = 0;
    st->cg_reason = 0;
    if (!isfinite(rz0)) {
      st->cg_done = 1;
      st->cg_reason = CG_NONFINITE;
    } else if (rz0 == 0.0) {
      st->cg_done = 1;
      st->cg_reason = CG_ZERO_RHS;
    }
  }
}

// s_q = sum_n Jp_n^T (Jc_n v_cam(n)) over point q's observations in index order
__device__ __forceinline__ void gba_point_gather(const GbaArgs& P, int q, const double* v,
                                                 double* s) {
  s[0] = s[1] = s[2] = 0.0;
  for (int k = P.ix.pt_start[q]; k < P.ix.pt_start[q + 1]; ++k) {
    const int o = P.ix.pt_order[k];
    const double* jc = P.Jc + 12 * (int64_t)o;
    const double* jp = P.Jp + 6 * (int64_t)o;
    const double* d = v + 6 * P.oacam[o];
    double t0 = 0.0, t1 = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      t0 += jc[i] * d[i];
      t1 += jc[6 + i] * d[i];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) s[j] += jp[j] * t0 + jp[3 + j] * t1;
  }
}

__global__ __launch_bounds__(64) void gba_cg_point_kernel(GbaArgs P) {
  if (!gba_live(P) || P.st->lin_fail || P.st->cg_done) return;
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= P.Pa) return;
  double s[3], y[3], v[3];
  gba_point_gather(P, q, P.p, s);
  const double* lv = P.Lv + 6 * (int64_t)q;
  gba_fwd3(lv, s, y);
  gba_bwd3(lv, y, v);
#pragma unroll
  for (int j = 0; j < 3; ++j) P.yp[3 * q + j] = v[j];
}

__global__ __launch_bounds__(64) void gba_cg_camera_kernel(GbaArgs P) {
  if (!gba_live(P) || P.st->lin_fail || P.st->cg_done) return;
  const int lane = threadIdx.x, a = blockIdx.x;
  double acc[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[i] = 0.0;
  for (int k = P.ix.cam_start[a] + lane; k < P.ix.cam_start[a + 1]; k += 64) {
    const int o = P.ix.cam_order[k];
    const double* jc = P.Jc + 12 * (int64_t)o;
    const double* jp = P.Jp + 6 * (int64_t)o;
    const double* y = P.yp + 3 * (int64_t)P.oapt[o];
    const double t0 = jp[0] * y[0] + jp[1] * y[1] + jp[2] * y[2];
    const double t1 = jp[3] * y[0] + jp[4] * y[1] + jp[5] * y[2];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] += jc[i] * t0 + jc[6 + i] * t1;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[i] = wave_sum_d(acc[i]);
  if (lane != 0) return;
  const double* pc = P.p + 6 * a;
  double dot = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) v += P.U[36 * a + 6 * i + j] * pc[j];
    v -= acc[i];
    P.Sp[6 * a + i] = v;
    dot += pc[i] * v;
  }
  P.camdot[a] = dot;
}

// One workgroup: p . S p, the step along p, the preconditioned residual, the new direction and
// the stop tests of the header
__global__ __launch_bounds__(256) void gba_cg_update_kernel(GbaArgs P) {
  __shared__ double lds[256];
  if (!gba_live(P) || P.st->lin_fail || P.st->cg_done) return;   // uniform: read before any write
  GbaState* st = P.st;
  const int t = threadIdx.x;
  const double rz = st->rz, rz0 = st->rz0;
  const int k = st->cg_iters + 1;
  const double pSp = gba_block_sum(P.camdot, P.A, lds);   // its barriers order the reads above
  if (!isfinite(pSp) || pSp <= 0.0) {
    if (t == 0) {
      st->cg_done = 1;
      st->cg_reason = isfinite(pSp) ? CG_INDEFINITE : CG_NONFINITE;
    }
    return;
  }
  const double alpha = rz / pSp;
  for (int a = t; a < P.A; a += 256) {
    double res[6], z[6], dot = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      P.x[6 * a + i] += alpha * P.p[6 * a + i];
      res[i] = P.res[6 * a + i] - alpha * P.Sp[6 * a + i];
      P.res[6 * a + i] = res[i];
    }
    gba_solve6(P.Mc + 21 * a, res, z);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      P.z[6 * a + i] = z[i];
      dot += res[i] * z[i];
    }
    P.camdot[a] = dot;
  }
  const double rzn = gba_block_sum(P.camdot, P.A, lds);
  const double beta = rzn / rz;
  for (int a = t; a < P.A; a += 256)
#pragma unroll
    for (int i = 0; i < 6; ++i) P.p[6 * a + i] = P.z[6 * a + i] + beta * P.p[6 * a + i];
  if (t == 0) {
    st->rz = rzn;
    st->cg_iters = k;
    st->cg_total += 1.0;
    int reason = 0;
    if (!isfinite(alpha) || !isfinite(rzn) || !isfinite(beta)) reason = CG_NONFINITE;
    else if (sqrt(rzn / rz0) <= P.pcg_tol) reason = CG_TOL;
    else if (k >= P.pcg_max) reason = CG_CAP;
    if (reason) {
      st->cg_done = 1;
      st->cg_reason = reason;
    }
  }
}

// dp = L^-T L^-1 (-g_p - sum Jp^T (Jc dc)) per active point, and the candidate variables
__global__ __launch_bounds__(256) void gba_update_kernel(GbaArgs P) {
  if (!gba_live(P) || P.st->lin_fail) return;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < P.Pa) {
    const int q = e;
    double s[3], b[3], y[3], d[3];
    gba_point_gather(P, q, P.x, s);
#pragma unroll
    for (int j = 0; j < 3; ++j) b[j] = -P.gp[3 * q + j] - s[j];
    const double* lv = P.Lv + 6 * (int64_t)q;
    gba_fwd3(lv, b, y);
    gba_bwd3(lv, y, d);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      P.dp[3 * q + j] = d[j];
      P.ptn[3 * q + j] = P.ptw[3 * q + j] + d[j];
    }
  } else if (e < P.Pa + 6 * P.A) {
    const int j = e - P.Pa;
    const bool fixed = P.fixa[j / 6] >> (j % 6) & 1;
    P.camn[j] = fixed ? P.camw[j] : P.camw[j] + P.x[j];
  }
}

// Per observation: the candidate's cost term 1/2 |r'|^2 and the model decrease term
// -(J d) . (r + J d / 2).  initial: the cost term of the working copies alone.
__global__ __launch_bounds__(256) void gba_eval_kernel(GbaArgs P, int initial) {
  if (!gba_live(P) || (!initial && P.st->lin_fail)) return;
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= P.N) return;
  const int a = P.oacam[o], q = P.oapt[o];
  double rr[2];
  gba_observe((initial ? P.camw : P.camn) + 6 * a, (initial ? P.ptw : P.ptn) + 3 * q,
              P.K4 + 4 * (int64_t)P.ix.act_cams[a], P.xy + 2 * (int64_t)o, rr, nullptr, nullptr);
  P.tcost[o] = 0.5 * (rr[0] * rr[0] + rr[1] * rr[1]);
  if (initial) return;
  const double* jc = P.Jc + 12 * (int64_t)o;
  const double* jp = P.Jp + 6 * (int64_t)o;
  const double* d = P.x + 6 * a;
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

// One workgroup: the sums, the decision, the trust region, the stop rules, the info block, and
// on acceptance the candidate becomes the iterate (working copies and the caller's arrays).
__global__ __launch_bounds__(256) void gba_decide_kernel(GbaArgs P, int initial) {
  __shared__ double lds[256];
  __shared__ int accept_s;
  if (!gba_live(P)) return;   // uniform: read before any write
  GbaState* st = P.st;
  const int t = threadIdx.x;
  const bool lin_fail = !initial && st->lin_fail;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double cand = nan, md = nan;
  __syncthreads();
  if (!lin_fail) {
    cand = gba_block_sum(P.tcost, P.N, lds);
    if (!initial) md = gba_block_sum(P.tmd, P.N, lds);
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
        st->status = GBA_FAILED;
        P.info[0] = (double)GBA_FAILED;
      }
    }
    return;
  }
  if (t == 0) {
    const double cost = st->cost, radius = st->radius;
    const double rho = lin_fail ? nan : (cost - cand) / md;
    const bool accept = !lin_fail && isfinite(cand) && md > 0.0 && rho > 1e-3;
    if (st->iter < P.info_rows) {
      double* row = P.info + kGbaInfoHead + kGbaInfoRow * (int64_t)st->iter;
      row[0] = cost;
      row[1] = cand;
      row[2] = md;
      row[3] = rho;
      row[4] = radius;
      row[5] = accept ? 1.0 : 0.0;
      row[6] = lin_fail ? 0.0 : (double)st->cg_iters;
      row[7] = lin_fail ? 0.0 : (double)st->cg_reason;
    }
    int status = GBA_OK;
    if (accept) {
      const double q = 2.0 * rho - 1.0;
      st->radius = fmin(radius / fmax(1.0 / 3.0, 1.0 - q * q * q), 1e16);
      st->factor = 2.0;
      st->cost = cand;
      st->succ += 1;
      st->need_lin = 1;
      if (P.ftol > 0.0 && fabs(cost - cand) / cost <= P.ftol) status = GBA_CONVERGED;
    } else {
      st->radius = radius / st->factor;
      st->factor *= 2.0;
      st->need_lin = 0;
    }
    if (status == GBA_OK && st->radius < kGbaMinRadius) status = GBA_MIN_RADIUS;
    st->iter += 1;
    st->lin_fail = 0;
    st->cg_done = 1;
    st->cg_iters = 0;
    st->cg_reason = 0;
    if (status != GBA_OK) {
      st->status = status;
      st->done = 1;
    }
    P.info[0] = (double)status;
    P.info[1] = (double)st->iter;
    P.info[2] = (double)st->succ;
    P.info[4] = st->cost;
    P.info[5] = st->radius;
    P.info[6] = st->cg_total;
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

bool gba_dims_ok(int64_t N, int C, int P) {
  return N >= 1 && N <= kGbaMaxObs && C >= 1 && C <= kGbaMaxVars && P >= 1 && P <= kGbaMaxVars;
}

bool gba_active_ok(int64_t N, int A, int Pa) {
  return N >= 1 && N <= kGbaMaxObs && A >= 1 && A <= kGbaMaxCams && Pa >= 1 &&
         Pa <= kGbaMaxVars && A <= N && Pa <= N;
}

// The checks that begin and step share (everything before their own scalars), and the carve
int gba_common(const char* who, GbaArgs& a, double* points, double* cam_pose, const double* K4,
               const double* xy, const int64_t* ptIdx, const int64_t* camIdx,
               const uint8_t* fixed, const void* index, int64_t n_obs, int n_cams, int n_points,
               int A, int Pa, double* info, int info_rows, void* workspace) {
  OP_REQUIRE(points && cam_pose && K4 && xy && ptIdx && camIdx && index && info && workspace,
             "%s: null pointer (variables, intrinsics, observations, indices, index, info and "
             "workspace are all required)", who);
  OP_REQUIRE(gba_dims_ok(n_obs, n_cams, n_points) && A >= 1 && A <= n_cams && Pa >= 1 &&
                 Pa <= n_points && (int64_t)A <= n_obs && (int64_t)Pa <= n_obs,
             "%s: shape n_obs = %lld, n_cams = %d, n_points = %d, active %d / %d", who,
             (long long)n_obs, n_cams, n_points, A, Pa);
  OP_REQUIRE(A <= kGbaMaxCams, "%s: %d active cameras, at most %d", who, A, kGbaMaxCams);
  OP_REQUIRE(info_rows >= 0 && info_rows <= kGbaMaxInfoRows, "%s: info_rows = %d, need 0..%d",
             who, info_rows, kGbaMaxInfoRows);
  a.points = points;
  a.cam_pose = cam_pose;
  a.K4 = K4;
  a.xy = xy;
  a.ptIdx = ptIdx;
  a.camIdx = camIdx;
  a.fixed = fixed;
  a.ix = gba_index_layout(index, n_obs, n_cams, n_points);
  a.N = (int)n_obs;
  a.C = n_cams;
  a.P = n_points;
  a.A = A;
  a.Pa = Pa;
  a.info = info;
  a.info_rows = info_rows;
  return ONEPOSE_OK;
}

int gba_check_workspace(const char* who, GbaArgs& a, void* workspace, size_t workspace_bytes) {
  size_t need = 0;
  gba_carve(a, workspace, &need);
  if (workspace_bytes < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    return ONEPOSE_ERR_WORKSPACE;
  }
  return ONEPOSE_OK;
}

}  // namespace
}  // namespace onepose

using namespace onepose;

extern "C" {

int onepose_gba_version(void) { return kGbaVersion; }
int onepose_gba_max_cameras(void) { return kGbaMaxCams; }

size_t onepose_gba_workspace_bytes(int64_t n_obs, int n_active_cams, int n_active_points) {
  if (!gba_active_ok(n_obs, n_active_cams, n_active_points)) return 0;
  GbaArgs a{};
  a.N = (int)n_obs;
  a.A = n_active_cams;
  a.Pa = n_active_points;
  size_t bytes = 0;
  gba_carve(a, nullptr, &bytes);
  return bytes;
}

int onepose_gba_linearize(const double* points, const double* cam_pose, const double* cam_K4,
                          const double* obs_xy, const int64_t* ptIdx, const int64_t* camIdx,
                          const uint8_t* cam_fixed, int64_t n_obs, int n_cams, int n_points,
                          double* residuals, double* Jc, double* Jp, double* cost, void* stream) {
  clear_error();
  OP_REQUIRE(points && cam_pose && cam_K4 && obs_xy && ptIdx && camIdx && residuals && Jc && Jp &&
                 cost, "gba_linearize: null pointer");
  OP_REQUIRE(gba_dims_ok(n_obs, n_cams, n_points),
             "gba_linearize: shape n_obs = %lld, n_cams = %d, n_points = %d", (long long)n_obs,
             n_cams, n_points);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int N = (int)n_obs;
  hipLaunchKernelGGL(gba_linearize_plain_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, st, points,
                     cam_pose, cam_K4, obs_xy, ptIdx, camIdx, cam_fixed, N, n_cams, n_points,
                     residuals, Jc, Jp);
  OP_LAUNCHED();
  hipLaunchKernelGGL(gba_cost_kernel, dim3(1), dim3(256), 0, st, residuals, 2 * N, cost);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

int onepose_gba_begin(double* points, double* cam_pose, const double* cam_K4,
                      const double* obs_xy, const int64_t* ptIdx, const int64_t* camIdx,
                      const uint8_t* cam_fixed, const void* index, int64_t n_obs, int n_cams,
                      int n_points, int n_active_cams, int n_active_points,
                      double initial_radius, double* info, int info_rows, void* workspace,
                      size_t workspace_bytes, void* stream) {
  clear_error();
  GbaArgs a{};
  int rc = gba_common("gba_begin", a, points, cam_pose, cam_K4, obs_xy, ptIdx, camIdx, cam_fixed,
                      index, n_obs, n_cams, n_points, n_active_cams, n_active_points, info,
                      info_rows, workspace);
  if (rc != ONEPOSE_OK) return rc;
  OP_REQUIRE(initial_radius > 0.0 && std::isfinite(initial_radius),
             "gba_begin: initial_radius %g is not a positive finite number", initial_radius);
  a.radius0 = initial_radius;
  rc = gba_check_workspace("gba_begin", a, workspace, workspace_bytes);
  if (rc != ONEPOSE_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int most = a.N > a.Pa ? a.N : a.Pa;
  hipLaunchKernelGGL(gba_init_kernel, dim3(1), dim3(256), 0, st, a);
  OP_LAUNCHED();
  hipLaunchKernelGGL(gba_validate_kernel, dim3(ceil_div(most + 1, 256)), dim3(256), 0, st, a);
  OP_LAUNCHED();
  hipLaunchKernelGGL(gba_gather_kernel, dim3(ceil_div(6 * a.A + 3 * a.Pa, 256)), dim3(256), 0, st,
                     a);
  OP_LAUNCHED();
  hipLaunchKernelGGL(gba_eval_kernel, dim3(ceil_div(a.N, 256)), dim3(256), 0, st, a, 1);
  OP_LAUNCHED();
  hipLaunchKernelGGL(gba_decide_kernel, dim3(1), dim3(256), 0, st, a, 1);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

int onepose_gba_step(double* points, double* cam_pose, const double* cam_K4,
                     const double* obs_xy, const int64_t* ptIdx, const int64_t* camIdx,
                     const uint8_t* cam_fixed, const void* index, int64_t n_obs, int n_cams,
                     int n_points, int n_active_cams, int n_active_points, int n_steps,
                     int pcg_max_iters, double pcg_tol, double function_tolerance, double* info,
                     int info_rows, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  GbaArgs a{};
  int rc = gba_common("gba_step", a, points, cam_pose, cam_K4, obs_xy, ptIdx, camIdx, cam_fixed,
                      index, n_obs, n_cams, n_points, n_active_cams, n_active_points, info,
                      info_rows, workspace);
  if (rc != ONEPOSE_OK) return rc;
  OP_REQUIRE(n_steps >= 1 && n_steps <= kGbaMaxSteps, "gba_step: n_steps = %d, need 1..%d",
             n_steps, kGbaMaxSteps);
  OP_REQUIRE(pcg_max_iters >= 1 && pcg_max_iters <= kGbaMaxPcg,
             "gba_step: pcg_max_iters = %d, need 1..%d", pcg_max_iters, kGbaMaxPcg);
  OP_REQUIRE(std::isfinite(pcg_tol) && pcg_tol >= 0.0,
             "gba_step: pcg_tol %g is not finite and >= 0", pcg_tol);
  OP_REQUIRE(std::isfinite(function_tolerance) && function_tolerance >= 0.0,
             "gba_step: function_tolerance %g is not finite and >= 0", function_tolerance);
  a.pcg_max = pcg_max_iters;
  a.pcg_tol = pcg_tol;
  a.ftol = function_tolerance;
  rc = gba_check_workspace("gba_step", a, workspace, workspace_bytes);
  if (rc != ONEPOSE_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int obs_blocks = ceil_div(a.N, 256), pt_blocks = ceil_div(a.Pa, 64);
  for (int it = 0; it < n_steps; ++it) {
    hipLaunchKernelGGL(gba_linearize_kernel, dim3(obs_blocks), dim3(256), 0, st, a);
    OP_LAUNCHED();
    hipLaunchKernelGGL(gba_point_kernel, dim3(pt_blocks), dim3(64), 0, st, a);
    OP_LAUNCHED();
    hipLaunchKernelGGL(gba_camera_kernel, dim3(a.A), dim3(64), 0, st, a);
    OP_LAUNCHED();
    hipLaunchKernelGGL(gba_cg_start_kernel, dim3(1), dim3(256), 0, st, a);
    OP_LAUNCHED();
    for (int k = 0; k < pcg_max_iters; ++k) {
      hipLaunchKernelGGL(gba_cg_point_kernel, dim3(pt_blocks), dim3(64), 0, st, a);
      OP_LAUNCHED();
      hipLaunchKernelGGL(gba_cg_camera_kernel, dim3(a.A), dim3(64), 0, st, a);
      OP_LAUNCHED();
      hipLaunchKernelGGL(gba_cg_update_kernel, dim3(1), dim3(256), 0, st, a);
      OP_LAUNCHED();
    }
    hipLaunchKernelGGL(gba_update_kernel, dim3(ceil_div(a.Pa + 6 * a.A, 256)), dim3(256), 0, st, a);
    OP_LAUNCHED();
    hipLaunchKernelGGL(gba_eval_kernel, dim3(obs_blocks), dim3(256), 0, st, a, 0);
    OP_LAUNCHED();
    hipLaunchKernelGGL(gba_decide_kernel, dim3(1), dim3(256), 0, st, a, 0);
    OP_LAUNCHED();
  }
  return ONEPOSE_OK;
}

}  // extern "C"
