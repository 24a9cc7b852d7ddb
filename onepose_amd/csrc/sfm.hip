// Sparse reconstruction (the reference's sfm_core, run.py:140-193, after matching): feature tracks
// as connected components of the match graph, and this project's own multi-view triangulation in
// place of COLMAP's point_triangulator.  The contract is stated in include/onepose_hip.h;
// tests/sfm_oracle.py restates it in plain loops.  Contraction is off for this file, so every
// floating-point step is the operation written.
//
//   sfm_cc_init_kernel      parent[i] = i (a first call) and the status words
//   sfm_cc_compress_kernel  every node walks to its root and stores it
//   sfm_cc_hook_kernel      per edge with roots ru != rv: atomicMin(&parent[max], min)
//   sfm_cc_check_kernel     edges whose ends still differ, edges out of range
//   sfm_tri_check_kernel    the CSR checked before anything is read through it, one workgroup
//   sfm_tri_kernel          one wave per track: DLT with the drop-worst loop, the duplicate
//                           rule, Gauss-Newton, the final check; per-observation state in LDS
// Integer atomicMin only (its result does not depend on the order), no floating-point atomics,
// every sum over a track in ascending position; nothing between workgroups, no spin wait.
#include <limits.h>
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace onepose {
namespace {

constexpr int kSfmMaxTrack = 256;
constexpr int kSfmMaxRounds = 64;
constexpr int kSfmMaxNodes = 1 << 30;
constexpr int kSfmMaxTracks = 1 << 24;
constexpr int kSfmMaxObs = 1 << 28;
constexpr int kSfmCheckThreads = 1024;

// ---- connected components ----------------------------------------------------------------
// parent[x] <= x always, parent[r] == r at a root, and a parent only ever decreases: whatever a
// concurrent reader sees is a node of the same component that is not above x.  A value outside
// [0, x] (a caller's parent array that no first call wrote) ends the walk: nothing is read
// through it.
__device__ __forceinline__ int sfm_root(const int* parent, int x) {
  int r = x;
  for (;;) {
    const int p = parent[r];
    if (p < 0 || p >= r) break;
    r = p;
  }
  return r;
}

__global__ __launch_bounds__(256) void sfm_cc_init_kernel(int* parent, int n_nodes, int init,
                                                          int* status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 4) status[i] = 0;
  if (init && i < n_nodes) parent[i] = i;
}

__global__ __launch_bounds__(256) void sfm_cc_compress_kernel(int* parent, int n_nodes) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_nodes) return;
  const int r = sfm_root(parent, i);
  if (r != i) parent[i] = r;   // a root is never written here, so every walk ends at a true root
}

// status[3]: 1 + the last round in which an edge joined two trees.  Those rounds are 0, 1, ...
// without a gap (a round that joins nothing leaves every edge inside one tree for good), so
// round r has work only if status[3] >= r; the word only grows, so the test cannot race.
__global__ __launch_bounds__(256) void sfm_cc_hook_kernel(const int* edges, int n_edges,
                                                          int n_nodes, int round, int* parent,
                                                          int* status) {
  if (round > 0 && status[3] < round) return;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_edges) return;
  const int u = edges[2 * (int64_t)e], v = edges[2 * (int64_t)e + 1];
  if (u < 0 || u >= n_nodes || v < 0 || v >= n_nodes) return;
  const int ru = sfm_root(parent, u), rv = sfm_root(parent, v);
  if (ru == rv) return;
  atomicMin(&parent[ru > rv ? ru : rv], ru > rv ? rv : ru);
  atomicMax(&status[3], round + 1);
}

__global__ __launch_bounds__(256) void sfm_cc_check_kernel(const int* edges, int n_edges,
                                                           int n_nodes, const int* parent,
                                                           int* status) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e == 0) status[1] = status[3];
  if (e >= n_edges) return;
  const int u = edges[2 * (int64_t)e], v = edges[2 * (int64_t)e + 1];
  const bool outside = u < 0 || u >= n_nodes || v < 0 || v >= n_nodes;
  bool open = false;
  if (!outside) open = parent[u] != parent[v];
  // one add whose word is chosen per lane: two adds in two branches were merged by the compiler
  // into one whose address was wrong for an edge with only its second end outside
  if (outside || open) atomicAdd(status + (outside ? 2 : 0), 1);
}

// ---- triangulation -----------------------------------------------------------------------
struct SfmTri {
  const double* Rt;
  const double* K4;
  int n_images;
  const int* track_start;
  const int* obs_image;
  const double* obs_xy;
  int n_tracks, n_obs;
  double max_reproj, min_angle_deg;
  double* xyz;
  double* err;
  int* reason;
  int* n_kept;
  uint8_t* obs_keep;
  int* status;
};

// status[0]: 0, 1 track_start is not 0 = s[0] <= s[1] <= ... <= s[n_tracks] = n_obs, 2 an image id
// outside [0, n_images); status[1]: the smallest offending index.
__global__ __launch_bounds__(kSfmCheckThreads) void sfm_tri_check_kernel(SfmTri a) {
  __shared__ int bad_start, bad_image;
  if (threadIdx.x == 0) {
    bad_start = INT_MAX;
    bad_image = INT_MAX;
  }
  __syncthreads();
  for (int t = threadIdx.x; t <= a.n_tracks; t += kSfmCheckThreads) {
    const int s = a.track_start[t];
    bool bad = s < 0 || s > a.n_obs || (t == 0 && s != 0) || (t == a.n_tracks && s != a.n_obs);
    if (t > 0) bad = bad || s < a.track_start[t - 1];
    if (bad) atomicMin(&bad_start, t);
  }
  for (int o = threadIdx.x; o < a.n_obs; o += kSfmCheckThreads) {
    const int im = a.obs_image[o];
    if (im < 0 || im >= a.n_images) atomicMin(&bad_image, o);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.status[0] = bad_start != INT_MAX ? 1 : bad_image != INT_MAX ? 2 : 0;
    a.status[1] = bad_start != INT_MAX ? bad_start : bad_image != INT_MAX ? bad_image : 0;
  }
}

// The eigenvector of the smallest eigenvalue of the symmetric 4 x 4 M by cyclic Jacobi, as
// onepose_triangulate takes it (ba.hip).
__device__ __forceinline__ void sfm_smallest_eigvec4(double M[4][4], double h[4]) {
  double V[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
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
        for (int k = 0; k < 4; ++k) {
          const double mkp = M[k][p], mkq = M[k][q];
          M[k][p] = cs * mkp - sn * mkq;
          M[k][q] = sn * mkp + cs * mkq;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
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
  double best = M[0][0];
  h[0] = V[0][0], h[1] = V[1][0], h[2] = V[2][0], h[3] = V[3][0];
#pragma unroll
  for (int j = 1; j < 4; ++j)
    if (M[j][j] < best) {
      best = M[j][j];
      h[0] = V[0][j], h[1] = V[1][j], h[2] = V[2][j], h[3] = V[3][j];
    }
}

struct SfmCam {
  double r[12];   // Rt, row-major [3, 4]
  double fx, fy, cx, cy;
};

__device__ __forceinline__ SfmCam sfm_cam(const SfmTri& a, int im) {
  SfmCam c;
  const double* R = a.Rt + 12 * (int64_t)im;
#pragma unroll
  for (int k = 0; k < 12; ++k) c.r[k] = R[k];
  const double* K = a.K4 + 4 * (int64_t)im;
  c.fx = K[0], c.fy = K[1], c.cx = K[2], c.cy = K[3];
  return c;
}

// Camera coordinates of X, and the pixel residual (projection - observation).
__device__ __forceinline__ void sfm_residual(const SfmCam& c, const double* X, double u, double v,
                                             double* pc, double* ru, double* rv) {
  pc[0] = ((c.r[0] * X[0] + c.r[1] * X[1]) + c.r[2] * X[2]) + c.r[3];
  pc[1] = ((c.r[4] * X[0] + c.r[5] * X[1]) + c.r[6] * X[2]) + c.r[7];
  pc[2] = ((c.r[8] * X[0] + c.r[9] * X[1]) + c.r[10] * X[2]) + c.r[11];
  *ru = (c.fx * (pc[0] / pc[2]) + c.cx) - u;
  *rv = (c.fy * (pc[1] / pc[2]) + c.cy) - v;
}

// e = sqrt(ru^2 + rv^2), +inf where the depth is not positive; NaN stays NaN.
__device__ __forceinline__ double sfm_error(const SfmCam& c, const double* X, double u, double v) {
  double pc[3], ru, rv;
  sfm_residual(c, X, u, v, pc, &ru, &rv);
  const double e = sqrt(ru * ru + rv * rv);
  if (e != e || pc[2] != pc[2]) return NAN;
  return pc[2] > 0.0 ? e : INFINITY;
}

struct SfmLds {
  double row[8][kSfmMaxTrack];   // DLT rows, then the Jacobian rows and residuals, then the rays
  double e[kSfmMaxTrack];
  double bc[10];                 // the ten sums, read by every lane
  int img[kSfmMaxTrack];
  uint8_t in_s[kSfmMaxTrack];
  uint8_t drop[kSfmMaxTrack];
};

// sum over the positions of S, ascending, of row[a1] row[b1] + row[a2] row[b2]
__device__ __forceinline__ double sfm_serial_sum(const SfmLds& s, int len, int a1, int b1, int a2,
                                                 int b2) {
  double m = 0.0;
  for (int p = 0; p < len; ++p)
    if (s.in_s[p]) m = m + (s.row[a1][p] * s.row[b1][p] + s.row[a2][p] * s.row[b2][p]);
  return m;
}

__device__ __forceinline__ int sfm_count(const SfmLds& s, int len, int lane) {
  int n = 0;
  for (int p = lane; p < len; p += 64) n += s.in_s[p];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  return n;
}

__device__ __forceinline__ void sfm_fail(const SfmTri& a, int t, int start, int len, int lane,
                                         int why, bool clear_obs) {
  if (lane == 0) {
    a.reason[t] = why;
    a.n_kept[t] = 0;
    a.err[t] = NAN;
    a.xyz[3 * (int64_t)t] = a.xyz[3 * (int64_t)t + 1] = a.xyz[3 * (int64_t)t + 2] = NAN;
  }
  if (clear_obs)
    for (int p = lane; p < len; p += 64) a.obs_keep[start + p] = 0;
}

__global__ __launch_bounds__(64) void sfm_tri_kernel(SfmTri a) {
  __shared__ SfmLds s;
  if (a.status[0] != 0) return;   // the CSR check failed: nothing moves
  const int t = blockIdx.x, lane = threadIdx.x;
  const int start = a.track_start[t], len = a.track_start[t + 1] - start;
  if (len < 2 || len > kSfmMaxTrack) {
    // an over-long track's observations are cleared too: start .. start + len lies in the CSR
    sfm_fail(a, t, start, len, lane, 3, true);
    return;
  }
  const double* xy = a.obs_xy + 2 * (int64_t)start;
  for (int p = lane; p < len; p += 64) {
    const int im = a.obs_image[start + p];
    const SfmCam c = sfm_cam(a, im);
    const double xn = (xy[2 * p] - c.cx) / c.fx, yn = (xy[2 * p + 1] - c.cy) / c.fy;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s.row[j][p] = xn * c.r[8 + j] - c.r[j];
      s.row[4 + j][p] = yn * c.r[8 + j] - c.r[4 + j];
    }
    s.img[p] = im;
    s.in_s[p] = 1;
  }
  __syncthreads();
  // lane k < 10 owns entry (mi, mj) of the upper triangle of A^T A
  int mi = 0, mj = lane;
  while (mi < 3 && mj >= 4 - mi) {
    mj -= 4 - mi;
    ++mi;
  }
  mj += mi;
  double X[3];
  int count = len;
  // 1, 2: DLT on S; drop the worst observation while one fails
  for (;;) {
    if (lane < 10) s.bc[lane] = sfm_serial_sum(s, len, mi, mj, 4 + mi, 4 + mj);
    __syncthreads();
    double M[4][4], h[4];
    {
      int k = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) {
          M[i][j] = M[j][i] = s.bc[k];
          ++k;
        }
    }
    sfm_smallest_eigvec4(M, h);
    X[0] = h[0] / h[3], X[1] = h[1] / h[3], X[2] = h[2] / h[3];
    if (!(isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]))) {
      sfm_fail(a, t, start, len, lane, 4, true);
      return;
    }
    double we = -1.0;
    int wp = INT_MAX;
    bool nan = false;
    for (int p = lane; p < len; p += 64) {
      if (!s.in_s[p]) continue;
      const double e = sfm_error(sfm_cam(a, s.img[p]), X, xy[2 * p], xy[2 * p + 1]);
      s.e[p] = e;
      nan = nan || e != e;
      if (e > we) {   // ascending p: the lowest position wins a tie
        we = e;
        wp = p;
      }
    }
    if (__any(nan)) {
      sfm_fail(a, t, start, len, lane, 4, true);
      return;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double oe = __shfl_xor(we, o, 64);
      const int op = __shfl_xor(wp, o, 64);
      if (oe > we || (oe == we && op < wp)) {
        we = oe;
        wp = op;
      }
    }
    __syncthreads();
    if (!(we > a.max_reproj)) break;
    if (--count < 2) {
      sfm_fail(a, t, start, len, lane, 1, true);
      return;
    }
    if (lane == 0 && wp < len) s.in_s[wp] = 0;
    __syncthreads();
  }
  // 3: of several observations in one image the one with the smallest error stays
  for (int p = lane; p < len; p += 64) {
    bool drop = false;
    if (s.in_s[p]) {
      const int im = s.img[p];
      const double e = s.e[p];
      for (int q = 0; q < len; ++q)
        if (q != p && s.in_s[q] && s.img[q] == im && (s.e[q] < e || (s.e[q] == e && q < p)))
          drop = true;
    }
    s.drop[p] = drop;
  }
  __syncthreads();
  for (int p = lane; p < len; p += 64)
    if (s.drop[p]) s.in_s[p] = 0;
  __syncthreads();
  count = sfm_count(s, len, lane);
  if (count < 2) {
    sfm_fail(a, t, start, len, lane, 1, true);
    return;
  }
  // 4: Gauss-Newton on the squared pixel errors over S.  Lanes 0..5 sum H (00 01 02 11 12 22),
  // 6..8 g = J^T r, 9 the cost; rows 0..2 = du/dX, 3..5 = dv/dX, 6 = ru, 7 = rv.
  int a1 = 6, b1 = 6, a2 = 7, b2 = 7;
  if (lane < 6) {
    a1 = lane < 3 ? 0 : lane < 5 ? 1 : 2;
    b1 = lane < 3 ? lane : lane < 5 ? lane - 2 : 2;
    a2 = a1 + 3, b2 = b1 + 3;
  } else if (lane < 9) {
    a1 = lane - 6, b1 = 6, a2 = lane - 3, b2 = 7;
  }
  for (int step = 0; step < 5; ++step) {
    for (int p = lane; p < len; p += 64) {
      if (!s.in_s[p]) continue;
      const SfmCam c = sfm_cam(a, s.img[p]);
      double pc[3], ru, rv;
      sfm_residual(c, X, xy[2 * p], xy[2 * p + 1], pc, &ru, &rv);
      const double iz = 1.0 / pc[2], xz = pc[0] * iz, yz = pc[1] * iz;
      const double fu = c.fx * iz, fv = c.fy * iz;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        s.row[k][p] = fu * (c.r[k] - xz * c.r[8 + k]);
        s.row[3 + k][p] = fv * (c.r[4 + k] - yz * c.r[8 + k]);
      }
      s.row[6][p] = ru;
      s.row[7][p] = rv;
    }
    __syncthreads();
    if (lane < 10) s.bc[lane] = sfm_serial_sum(s, len, a1, b1, a2, b2);
    __syncthreads();
    const double h00 = s.bc[0], h01 = s.bc[1], h02 = s.bc[2], h11 = s.bc[3], h12 = s.bc[4],
                 h22 = s.bc[5], g0 = s.bc[6], g1 = s.bc[7], g2 = s.bc[8], cost = s.bc[9];
    // H = L L^T, H d = -g
    if (!(h00 > 0.0)) break;
    const double l00 = sqrt(h00), l10 = h01 / l00, l20 = h02 / l00;
    const double d11 = h11 - l10 * l10;
    if (!(d11 > 0.0)) break;
    const double l11 = sqrt(d11), l21 = (h12 - l20 * l10) / l11;
    const double d22 = (h22 - l20 * l20) - l21 * l21;
    if (!(d22 > 0.0)) break;
    const double l22 = sqrt(d22);
    const double y0 = -g0 / l00, y1 = (-g1 - l10 * y0) / l11, y2 = ((-g2 - l20 * y0) - l21 * y1) / l22;
    const double d2 = y2 / l22, d1 = (y1 - l21 * d2) / l11, d0 = ((y0 - l10 * d1) - l20 * d2) / l00;
    const double Xn[3] = {X[0] + d0, X[1] + d1, X[2] + d2};
    for (int p = lane; p < len; p += 64) {
      if (!s.in_s[p]) continue;
      double pc[3], ru, rv;
      sfm_residual(sfm_cam(a, s.img[p]), Xn, xy[2 * p], xy[2 * p + 1], pc, &ru, &rv);
      s.row[6][p] = ru;
      s.row[7][p] = rv;
    }
    __syncthreads();
    if (lane == 9) s.bc[9] = sfm_serial_sum(s, len, 6, 6, 7, 7);
    __syncthreads();
    const double cand = s.bc[9];
    __syncthreads();   // bc and the rows are rewritten by the next step
    if (!(cand < cost)) break;
    X[0] = Xn[0], X[1] = Xn[1], X[2] = Xn[2];
  }
  __syncthreads();
  // 5: the errors at the refined point; the observations that fail leave S
  bool nan = false;
  for (int p = lane; p < len; p += 64) {
    if (!s.in_s[p]) continue;
    const SfmCam c = sfm_cam(a, s.img[p]);
    const double e = sfm_error(c, X, xy[2 * p], xy[2 * p + 1]);
    nan = nan || e != e;
    s.e[p] = e;
    if (!(e <= a.max_reproj)) s.in_s[p] = 0;
    // the unit ray from X to the camera centre -R^T t
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      d[k] = -((c.r[k] * c.r[3] + c.r[4 + k] * c.r[7]) + c.r[8 + k] * c.r[11]) - X[k];
    const double nrm = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) s.row[k][p] = d[k] / nrm;
  }
  if (__any(nan)) {
    sfm_fail(a, t, start, len, lane, 4, true);
    return;
  }
  __syncthreads();
  count = sfm_count(s, len, lane);
  if (count < 2) {
    sfm_fail(a, t, start, len, lane, 1, true);
    return;
  }
  double cmin = 2.0;   // the largest angle is the smallest cosine; min is exact in any order
  for (int p = lane; p < len; p += 64) {
    if (!s.in_s[p]) continue;
    for (int q = p + 1; q < len; ++q)
      if (s.in_s[q]) {
        const double c = (s.row[0][p] * s.row[0][q] + s.row[1][p] * s.row[1][q]) +
                         s.row[2][p] * s.row[2][q];
        cmin = c < cmin ? c : cmin;
        nan = nan || c != c;
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double oc = __shfl_xor(cmin, o, 64);
    cmin = oc < cmin ? oc : cmin;
  }
  if (__any(nan)) {
    sfm_fail(a, t, start, len, lane, 4, true);
    return;
  }
  const double angle = acos(fmin(fmax(cmin, -1.0), 1.0)) * (180.0 / 3.14159265358979323846);
  if (angle < a.min_angle_deg) {
    sfm_fail(a, t, start, len, lane, 2, true);
    return;
  }
  if (lane == 0) {
    double sum = 0.0;
    for (int p = 0; p < len; ++p)
      if (s.in_s[p]) sum = sum + s.e[p];
    a.reason[t] = 0;
    a.n_kept[t] = count;
    a.err[t] = sum / (double)count;
    a.xyz[3 * (int64_t)t] = X[0];
    a.xyz[3 * (int64_t)t + 1] = X[1];
    a.xyz[3 * (int64_t)t + 2] = X[2];
  }
  for (int p = lane; p < len; p += 64) a.obs_keep[start + p] = s.in_s[p];
}

}  // namespace
}  // namespace onepose

using namespace onepose;

extern "C" {

int onepose_sfm_version(void) { return 1; }

int onepose_sfm_max_track(void) { return kSfmMaxTrack; }

int onepose_track_components(const int* edges, int n_edges, int n_nodes, int rounds, int init,
                             int* parent, int* status, void* stream) {
  clear_error();
  OP_REQUIRE(n_nodes >= 1 && n_nodes <= kSfmMaxNodes, "track_components: n_nodes=%d outside 1..2^30",
             n_nodes);
  OP_REQUIRE(n_edges >= 0 && n_edges <= kSfmMaxNodes, "track_components: n_edges=%d outside 0..2^30",
             n_edges);
  OP_REQUIRE(rounds >= 0 && rounds <= kSfmMaxRounds, "track_components: rounds=%d outside 0..%d",
             rounds, kSfmMaxRounds);
  OP_REQUIRE(parent && status && (edges || n_edges == 0), "track_components: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 block(256), nodes(ceil_div(n_nodes, 256)), edge_grid(n_edges ? ceil_div(n_edges, 256) : 1);
  hipLaunchKernelGGL(sfm_cc_init_kernel, nodes, block, 0, st, parent, n_nodes, init, status);
  OP_LAUNCHED();
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(sfm_cc_compress_kernel, nodes, block, 0, st, parent, n_nodes);
    OP_LAUNCHED();
    hipLaunchKernelGGL(sfm_cc_hook_kernel, edge_grid, block, 0, st, edges, n_edges, n_nodes, r,
                       parent, status);
    OP_LAUNCHED();
  }
  hipLaunchKernelGGL(sfm_cc_compress_kernel, nodes, block, 0, st, parent, n_nodes);
  OP_LAUNCHED();
  hipLaunchKernelGGL(sfm_cc_check_kernel, edge_grid, block, 0, st, edges, n_edges, n_nodes, parent,
                     status);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

int onepose_tracks_triangulate(const double* Rt, const double* K4, int n_images,
                               const int* track_start, const int* obs_image, const double* obs_xy,
                               int n_tracks, int n_obs, double max_reproj, double min_angle_deg,
                               double* xyz, double* err, int* reason, int* n_kept,
                               uint8_t* obs_keep, int* status, void* stream) {
  clear_error();
  OP_REQUIRE(n_images >= 1 && n_images <= (1 << 24), "tracks_triangulate: n_images=%d", n_images);
  OP_REQUIRE(n_tracks >= 1 && n_tracks <= kSfmMaxTracks,
             "tracks_triangulate: n_tracks=%d outside 1..2^24", n_tracks);
  OP_REQUIRE(n_obs >= 1 && n_obs <= kSfmMaxObs, "tracks_triangulate: n_obs=%d outside 1..2^28",
             n_obs);
  OP_REQUIRE(max_reproj == max_reproj && min_angle_deg == min_angle_deg,
             "tracks_triangulate: NaN threshold");
  OP_REQUIRE(Rt && K4 && track_start && obs_image && obs_xy && xyz && err && reason && n_kept &&
                 obs_keep && status,
             "tracks_triangulate: null pointer");
  SfmTri a{Rt, K4, n_images, track_start, obs_image, obs_xy, n_tracks, n_obs, max_reproj,
           min_angle_deg, xyz, err, reason, n_kept, obs_keep, status};
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sfm_tri_check_kernel, dim3(1), dim3(kSfmCheckThreads), 0, st, a);
  OP_LAUNCHED();
  hipLaunchKernelGGL(sfm_tri_kernel, dim3(n_tracks), dim3(64), 0, st, a);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

}  // extern "C"
