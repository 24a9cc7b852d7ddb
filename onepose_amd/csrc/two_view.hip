// Two-view geometric verification on gfx950 (include/onepose_two_view.h): a fundamental matrix per
// image pair by RANSAC over the normalised 8-point algorithm, squared Sampson error, refits over
// the inliers -- or the same test against a given F.  One workgroup of 256 threads per pair, the
// pair's matches (16 B each) and their inlier flags in LDS.  The contract, operation order
// included, is the header's; tests/two_view_oracle.py restates it in plain loops.  Contraction
// is off for this file, so every floating-point step is the operation written.
//
// Per round of 64 iterations of the loop (the scaffold -- draws, inlier count, acceptance -- is
// ransac.h's):
//   1. wave 0 generates the round's cv::RNG draws by jump-ahead, thread 0 deals the 64 subsets
//      of 8 distinct indices from them in iteration order (a chain that outruns the generated
//      draws goes on sequentially);
//   2. lane h of wave 0 solves hypothesis h: Hartley normalisation, the 45 sums of A^T A and the
//      9 x 9 cyclic Jacobi with its matrix and eigenvectors in LDS at [entry][lane] (no
//      per-thread array is indexed at run time: 0 bytes of scratch), rank 2, denormalisation;
//   3. wave w counts the inliers of hypotheses w, w + 4, ... over the pair's matches;
//   4. thread 0 replays the acceptance rule in iteration order and stops where the sequential
//      loop would.
// A refit: 4, 2 and then 45 lanes of wave 0 each take one serial sum over the inliers in
// ascending order, lane 0 runs the same Jacobi, all threads score the candidate.
#include <math.h>

#include "common.h"
#include "ransac.h"

#pragma clang fp contract(off)

namespace onepose {
namespace {

constexpr int kTvModel = 8;
constexpr int kTvRound = 64;
constexpr int kTvThreads = 256;
constexpr int kTvDrawsPerLane = 10;   // generated per round: 8 + 10 * 64 draws
constexpr int kTvSweeps = 24;
constexpr int kTvSym = 45;            // unique entries of the symmetric 9 x 9
constexpr double kTvSqrt2 = 1.4142135623730951;

struct TvShared {
  double jm[kTvSym][kTvRound];   // A^T A, upper triangle by rows, [entry][lane]
  double jv[81][kTvRound];       // the Jacobi's V, [row * 9 + column][lane]
  double hyp[kTvRound][9];
  RansacDraws<kTvDrawsPerLane> draws;
  int subset[kTvRound][kTvModel];
  int count[kTvRound];
  RansacCtl ctl;
  double best[9], cand[9];
  double red[8];                 // a refit's cx0, cy0, cx1, cy1, s0, s1
  int wave_cnt[4];
};

// index of (i, j), i <= j, in the upper triangle stored by rows
__device__ __forceinline__ int tv_sym(int i, int j) { return i * 9 - (i * (i - 1)) / 2 + (j - i); }

// the row a of one match under a normalisation (cx0, cy0, cx1, cy1, s0, s1)
__device__ __forceinline__ void tv_row(const float4 p, const double (&nm)[6], double (&a)[9]) {
  const double u0 = ((double)p.x - nm[0]) * nm[4], v0 = ((double)p.y - nm[1]) * nm[4];
  const double u1 = ((double)p.z - nm[2]) * nm[5], v1 = ((double)p.w - nm[3]) * nm[5];
  a[0] = u1 * u0;
  a[1] = u1 * v0;
  a[2] = u1;
  a[3] = v1 * u0;
  a[4] = v1 * v0;
  a[5] = v1;
  a[6] = u0;
  a[7] = v0;
  a[8] = 1.0;
}

// J(9) on this lane's column of jm / jv (element e at [e * kTvRound]); returns the column of jv
// that holds the eigenvector of the smallest eigenvalue
__device__ __forceinline__ int tv_jacobi9(double* jm, double* jv) {
  constexpr int S = kTvRound;
  for (int e = 0; e < 81; ++e) jv[e * S] = (e / 9 == e % 9) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kTvSweeps; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 8; ++p)
      for (int q = p + 1; q < 9; ++q) {
        const int ipp = tv_sym(p, p), iqq = tv_sym(q, q), ipq = tv_sym(p, q);
        const double apq = jm[ipq * S], app = jm[ipp * S], aqq = jm[iqq * S];
        if (fabs(apq) <= 1e-20 * sqrt(fabs(app * aqq)) || apq == 0.0) {
          jm[ipq * S] = 0.0;
          continue;
        }
        rotated = true;
        const double theta = (aqq - app) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
        for (int r = 0; r < 9; ++r) {
          if (r == p || r == q) continue;
          const int irp = r < p ? tv_sym(r, p) : tv_sym(p, r);
          const int irq = r < q ? tv_sym(r, q) : tv_sym(q, r);
          const double arp = jm[irp * S], arq = jm[irq * S];
          jm[irp * S] = cs * arp - sn * arq;
          jm[irq * S] = sn * arp + cs * arq;
        }
        const double bpp = cs * app - sn * apq, bpq = sn * app + cs * apq;
        const double bqp = cs * apq - sn * aqq, bqq = sn * apq + cs * aqq;
        jm[ipp * S] = cs * bpp - sn * bqp;
        jm[iqq * S] = sn * bpq + cs * bqq;
        jm[ipq * S] = 0.0;
        for (int r = 0; r < 9; ++r) {
          const double vrp = jv[(r * 9 + p) * S], vrq = jv[(r * 9 + q) * S];
          jv[(r * 9 + p) * S] = cs * vrp - sn * vrq;
          jv[(r * 9 + q) * S] = sn * vrp + cs * vrq;
        }
      }
    if (!rotated) break;
  }
  int bj = 0;
  double best = jm[0];
  for (int j = 1; j < 9; ++j) {
    const double d = jm[tv_sym(j, j) * S];
    if (d < best) {
      best = d;
      bj = j;
    }
  }
  return bj;
}

// J(3) in registers (static indices only): the eigenvector of the smallest eigenvalue of G
__device__ __forceinline__ void tv_jacobi3(double (&M)[3][3], double (&v)[3]) {
  double V[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kTvSweeps; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        const double apq = M[p][q], app = M[p][p], aqq = M[q][q];
        if (fabs(apq) <= 1e-20 * sqrt(fabs(app * aqq)) || apq == 0.0) {
          M[p][q] = M[q][p] = 0.0;
          continue;
        }
        rotated = true;
        const double theta = (aqq - app) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          if (r == p || r == q) continue;
          const double arp = M[r][p], arq = M[r][q];
          M[r][p] = M[p][r] = cs * arp - sn * arq;
          M[r][q] = M[q][r] = sn * arp + cs * arq;
        }
        const double bpp = cs * app - sn * apq, bpq = sn * app + cs * apq;
        const double bqp = cs * apq - sn * aqq, bqq = sn * apq + cs * aqq;
        M[p][p] = cs * bpp - sn * bqp;
        M[q][q] = sn * bpq + cs * bqq;
        M[p][q] = M[q][p] = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double vrp = V[r][p], vrq = V[r][q];
          V[r][p] = cs * vrp - sn * vrq;
          V[r][q] = sn * vrp + cs * vrq;
        }
      }
    if (!rotated) break;
  }
  double best = M[0][0];
  v[0] = V[0][0], v[1] = V[1][0], v[2] = V[2][0];
#pragma unroll
  for (int j = 1; j < 3; ++j)
    if (M[j][j] < best) {
      best = M[j][j];
      v[0] = V[0][j], v[1] = V[1][j], v[2] = V[2][j];
    }
}

// Steps 3-5 of the solver on this lane's sums: Jacobi, rank 2, denormalisation.
__device__ __forceinline__ void tv_finish(double* jm, double* jv, const double (&nm)[6],
                                          double* Fout) {
  const int bj = tv_jacobi9(jm, jv);
  double f[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) f[r] = jv[(r * 9 + bj) * kTvRound];
  double N[3][3] = {{f[0], f[1], f[2]}, {f[3], f[4], f[5]}, {f[6], f[7], f[8]}};
  double G[3][3], v[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) G[i][j] = (N[0][i] * N[0][j] + N[1][i] * N[1][j]) + N[2][i] * N[2][j];
  tv_jacobi3(G, v);
  double A[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double w = (N[i][0] * v[0] + N[i][1] * v[1]) + N[i][2] * v[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) N[i][j] = N[i][j] - w * v[j];
    A[i][0] = N[i][0] * nm[4];
    A[i][1] = N[i][1] * nm[4];
    A[i][2] = (N[i][2] - A[i][0] * nm[0]) - A[i][1] * nm[1];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double f0 = nm[5] * A[0][j], f1 = nm[5] * A[1][j];
    Fout[j] = f0;
    Fout[3 + j] = f1;
    Fout[6 + j] = (A[2][j] - nm[2] * f0) - nm[3] * f1;
  }
}

// S(subset) by one lane: the hypothesis of the 8 matches sub[0..7], in that order
__device__ __forceinline__ void tv_solve_minimal(const float4* pts, const int* sub, double* jm, double* jv,
                                 double* Fout) {
  constexpr int S = kTvRound;
  double nm[6];
  double sx0 = 0.0, sy0 = 0.0, sx1 = 0.0, sy1 = 0.0;
  for (int k = 0; k < kTvModel; ++k) {
    const float4 p = pts[sub[k]];
    sx0 = sx0 + (double)p.x;
    sy0 = sy0 + (double)p.y;
    sx1 = sx1 + (double)p.z;
    sy1 = sy1 + (double)p.w;
  }
  const double m = (double)kTvModel;
  nm[0] = sx0 / m;
  nm[1] = sy0 / m;
  nm[2] = sx1 / m;
  nm[3] = sy1 / m;
  double d0 = 0.0, d1 = 0.0;
  for (int k = 0; k < kTvModel; ++k) {
    const float4 p = pts[sub[k]];
    const double dx0 = (double)p.x - nm[0], dy0 = (double)p.y - nm[1];
    const double dx1 = (double)p.z - nm[2], dy1 = (double)p.w - nm[3];
    d0 = d0 + sqrt(dx0 * dx0 + dy0 * dy0);
    d1 = d1 + sqrt(dx1 * dx1 + dy1 * dy1);
  }
  nm[4] = kTvSqrt2 / (d0 / m);
  nm[5] = kTvSqrt2 / (d1 / m);
  for (int e = 0; e < kTvSym; ++e) jm[e * S] = 0.0;
  for (int k = 0; k < kTvModel; ++k) {
    double a[9];
    tv_row(pts[sub[k]], nm, a);
    int e = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
      for (int j = i; j < 9; ++j, ++e) jm[e * S] = jm[e * S] + a[i] * a[j];
  }
  tv_finish(jm, jv, nm, Fout);
}

__device__ __forceinline__ bool tv_finite9(const double* F) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) ok = ok && isfinite(F[i]);
  return ok;
}

// squared Sampson distance of one match
__device__ __forceinline__ double tv_sampson(const double (&F)[9], const float4 p) {
  const double x0 = p.x, y0 = p.y, x1 = p.z, y1 = p.w;
  const double a0 = (F[0] * x0 + F[1] * y0) + F[2];
  const double a1 = (F[3] * x0 + F[4] * y0) + F[5];
  const double a2 = (F[6] * x0 + F[7] * y0) + F[8];
  const double b0 = (F[0] * x1 + F[3] * y1) + F[6];
  const double b1 = (F[1] * x1 + F[4] * y1) + F[7];
  const double e = (x1 * a0 + y1 * a1) + a2;
  return (e * e) / (((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1);
}

struct TvArgs {
  const float* pts0;
  const float* pts1;
  const int* counts;
  int max_points;
  const double* F_in;
  double max_error, confidence;
  int max_trials, min_num_inliers;
  double min_inlier_ratio;
  int refine_iters;
  double* F;
  uint8_t* inlier_mask;
  int* n_inliers;
  int* iters;
  int* status;
};

__global__ __launch_bounds__(kTvThreads) void two_view_kernel(TvArgs a) {
  __shared__ TvShared sh;
  extern __shared__ __attribute__((aligned(16))) unsigned char tv_dyn[];
  float4* pts = reinterpret_cast<float4*>(tv_dyn);
  uint8_t* lmask = tv_dyn + (size_t)a.max_points * 16;
  const int b = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = min(max(a.counts[b], 0), a.max_points);
  uint8_t* mask = a.inlier_mask + (int64_t)b * a.max_points;
  double* Fo = a.F + (int64_t)b * 9;
  const bool given = a.F_in != nullptr;
  const double thr = a.max_error * a.max_error;

  // all threads: the mask of F over the pair's matches into LDS (when store), its count
  auto score = [&](const double* Fp, bool store) {
    double F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = Fp[i];
    const bool ok = tv_finite9(F);
    const int c = wave_count_if(t, n, kTvThreads, [&](int i) {
      const bool in = ok && tv_sampson(F, pts[i]) <= thr;
      if (store) lmask[i] = in ? 1 : 0;
      return in;
    });
    __syncthreads();   // (the previous reader of wave_cnt is done)
    if (lane == 0) sh.wave_cnt[wave] = c;
    __syncthreads();
    return sh.wave_cnt[0] + sh.wave_cnt[1] + sh.wave_cnt[2] + sh.wave_cnt[3];
  };
  // no model, or nothing run: a zero mask, F zeros (the given F's copy)
  auto none = [&](int st, int it) {
    for (int i = t; i < a.max_points; i += kTvThreads) mask[i] = 0;
    if (t < 9) Fo[t] = given ? a.F_in[(int64_t)b * 9 + t] : 0.0;
    if (t == 0) {
      a.n_inliers[b] = 0;
      a.iters[b] = it;
      a.status[b] = st;
    }
  };
  auto report = [&](const double* Fp, int nin, int it) {
    for (int i = t; i < a.max_points; i += kTvThreads) mask[i] = i < n ? lmask[i] : 0;
    if (t < 9) Fo[t] = Fp[t];
    if (t == 0) {
      a.n_inliers[b] = nin;
      a.iters[b] = it;
      a.status[b] =
          (nin < a.min_num_inliers || (double)nin < a.min_inlier_ratio * (double)n) ? 3 : 0;
    }
  };

  if (n < a.min_num_inliers) {
    none(1, 0);
    return;
  }
  for (int i = t; i < n; i += kTvThreads) {
    const int64_t g = ((int64_t)b * a.max_points + i) * 2;
    pts[i] = make_float4(a.pts0[g], a.pts0[g + 1], a.pts1[g], a.pts1[g + 1]);
  }
  if (given) {
    if (t < 9) sh.best[t] = a.F_in[(int64_t)b * 9 + t];
    __syncthreads();
    const int nin = score(sh.best, true);
    report(sh.best, nin, 0);
    return;
  }
  if (t == 0) ransac_ctl_init(sh.ctl, a.max_trials, false);
  __syncthreads();

  while (!sh.ctl.done) {
    if (wave == 0) {
      const int P = ransac_round_draws(sh.draws, sh.ctl, n);
      wave_lds_sync();
      if (lane == 0) {   // 64 subsets of 8 distinct indices, in iteration order
        unsigned long long st = sh.ctl.rng;
        int pos = 0;
        for (int h = 0; h < kTvRound; ++h) {
          for (int i = 0; i < kTvModel;) {
            int v;
            if (pos < P) {
              st = sh.draws.rst[pos];
              v = sh.draws.rii[pos];
            } else {
              v = (int)(rng_next(st) % (unsigned)n);
            }
            ++pos;
            int j = 0;
            for (; j < i; ++j)
              if (sh.subset[h][j] == v) break;
            if (j < i) continue;
            sh.subset[h][i++] = v;
          }
        }
        sh.ctl.rng = st;
      }
      wave_lds_sync();
      tv_solve_minimal(pts, sh.subset[lane], &sh.jm[0][lane], &sh.jv[0][lane], sh.hyp[lane]);
    }
    __syncthreads();
    for (int h = wave; h < kTvRound; h += 4) {
      double F[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) F[i] = sh.hyp[h][i];
      const bool ok = tv_finite9(F);
      const int c =
          wave_count_if(lane, n, 64, [&](int i) { return ok && tv_sampson(F, pts[i]) <= thr; });
      if (lane == 0) sh.count[h] = c;
    }
    __syncthreads();
    if (t == 0) {
      ransac_accept(sh.ctl, sh.count, 0, kTvRound, n, a.confidence, kTvModel, [&](int h) {
        for (int i = 0; i < 9; ++i) sh.best[i] = sh.hyp[h][i];
      });
    }
    __syncthreads();
  }

  const int it = sh.ctl.iter;
  if (sh.ctl.max_good <= 0) {
    none(2, it);
    return;
  }
  int nin = score(sh.best, true);
  for (int r = 0; r < a.refine_iters; ++r) {
    __syncthreads();   // lmask complete, sh.cand's readers done
    if (wave == 0) {
      // 1: the centroids, one serial sum per lane
      if (lane < 4) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) {
          if (!lmask[i]) continue;
          const float4 p = pts[i];
          const float c = lane == 0 ? p.x : lane == 1 ? p.y : lane == 2 ? p.z : p.w;
          s = s + (double)c;
        }
        sh.red[lane] = s / (double)nin;
      }
      wave_lds_sync();
      if (lane < 2) {
        const double cx = sh.red[2 * lane], cy = sh.red[2 * lane + 1];
        double d = 0.0;
        for (int i = 0; i < n; ++i) {
          if (!lmask[i]) continue;
          const float4 p = pts[i];
          const double dx = (double)(lane == 0 ? p.x : p.z) - cx;
          const double dy = (double)(lane == 0 ? p.y : p.w) - cy;
          d = d + sqrt(dx * dx + dy * dy);
        }
        sh.red[4 + lane] = kTvSqrt2 / (d / (double)nin);
      }
      wave_lds_sync();
      // 2: the 45 sums of A^T A into lane 0's column
      if (lane < kTvSym) {
        int ei = 0, ej = lane;
        while (ej >= 9 - ei) {
          ej -= 9 - ei;
          ++ei;
        }
        ej += ei;
        // a = (u1, v1, 1) x (u0, v0, 1): entry k is left[k / 3] * right[k % 3], and a product
        // with 1.0 is exact, so these are tv_row's values without an array indexed at run time
        const int li = ei / 3, ri = ei % 3, lj = ej / 3, rj = ej % 3;
        const double cx0 = sh.red[0], cy0 = sh.red[1], cx1 = sh.red[2], cy1 = sh.red[3];
        const double s0 = sh.red[4], s1 = sh.red[5];
        double m = 0.0;
        for (int i = 0; i < n; ++i) {
          if (!lmask[i]) continue;
          const float4 p = pts[i];
          const double u0 = ((double)p.x - cx0) * s0, v0 = ((double)p.y - cy0) * s0;
          const double u1 = ((double)p.z - cx1) * s1, v1 = ((double)p.w - cy1) * s1;
          const double ai = (li == 0 ? u1 : li == 1 ? v1 : 1.0) * (ri == 0 ? u0 : ri == 1 ? v0 : 1.0);
          const double aj = (lj == 0 ? u1 : lj == 1 ? v1 : 1.0) * (rj == 0 ? u0 : rj == 1 ? v0 : 1.0);
          m = m + ai * aj;
        }
        sh.jm[lane][0] = m;
      }
      wave_lds_sync();
      if (lane == 0) {
        double nm[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) nm[k] = sh.red[k];
        tv_finish(&sh.jm[0][0], &sh.jv[0][0], nm, sh.cand);
      }
    }
    __syncthreads();
    const int c = score(sh.cand, false);
    if (!(tv_finite9(sh.cand) && c >= nin)) break;
    __syncthreads();
    if (t < 9) sh.best[t] = sh.cand[t];
    __syncthreads();
    nin = score(sh.best, true);
  }
  __syncthreads();
  report(sh.best, nin, it);
}

}  // namespace
}  // namespace onepose

using namespace onepose;

extern "C" {

constexpr size_t kTvLdsBudget = 160 * 1024;
constexpr size_t kTvPointBytes = 17;   // a float4 and an inlier flag
constexpr size_t kTvStaticBytes = (sizeof(TvShared) + 15) / 16 * 16;   // as the kernel's metadata has it
constexpr size_t kTvDynMax = (kTvLdsBudget - kTvStaticBytes) / 16 * 16;
static_assert(4096 * kTvPointBytes <= kTvDynMax, "4096 matches (SuperPoint's max_keypoints) must fit");

int onepose_twoview_version(void) { return 1; }

int onepose_two_view_max_points(void) {
  return (int)(kTvDynMax / kTvPointBytes);
}

size_t onepose_two_view_workspace_bytes(int batch, int max_points) {
  if (batch <= 0 || max_points <= 0) return 0;
  return 256;   // reserved: every pair's state is in its workgroup's LDS
}

int onepose_two_view_verify(const float* pts0, const float* pts1, const int* counts,
                            int max_points, int batch, const double* F_in, double max_error,
                            double confidence, int max_trials, int min_num_inliers,
                            double min_inlier_ratio, int refine_iters, double* F,
                            uint8_t* inlier_mask, int* n_inliers, int* iters, int* status,
                            void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  OP_REQUIRE(pts0 && pts1 && counts, "two_view: null input");
  OP_REQUIRE(F && inlier_mask && n_inliers && iters && status, "two_view: null output");
  OP_REQUIRE(batch >= 1 && max_points >= 1, "two_view: batch=%d max_points=%d", batch, max_points);
  OP_REQUIRE(max_points <= onepose_two_view_max_points(),
             "two_view: max_points=%d above onepose_two_view_max_points() = %d (LDS)", max_points,
             onepose_two_view_max_points());
  OP_REQUIRE(min_num_inliers >= kTvModel, "two_view: min_num_inliers %d below 8", min_num_inliers);
  OP_REQUIRE(max_trials >= 1, "two_view: max_trials %d below 1", max_trials);
  OP_REQUIRE(refine_iters >= 0, "two_view: refine_iters %d negative", refine_iters);
  OP_REQUIRE(max_error >= 0.0, "two_view: max_error %f negative or NaN", max_error);
  OP_REQUIRE(confidence > 0 && confidence < 1, "two_view: confidence %f not in (0,1)", confidence);
  OP_REQUIRE(min_inlier_ratio == min_inlier_ratio, "two_view: min_inlier_ratio is NaN");
  const size_t need = onepose_two_view_workspace_bytes(batch, max_points);
  if (!workspace || workspace_bytes < need) {
    set_error("two_view: workspace %zu < %zu bytes", workspace_bytes, need);
    return ONEPOSE_ERR_WORKSPACE;
  }
  static bool attr_set = false;
  if (!attr_set) {
    OP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(two_view_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)kTvDynMax));
    attr_set = true;
  }
  const size_t lds = align_up((size_t)max_points * kTvPointBytes, 16);
  const TvArgs a{pts0, pts1, counts, max_points, F_in, max_error, confidence, max_trials,
                 min_num_inliers, min_inlier_ratio, refine_iters, F, inlier_mask, n_inliers,
                 iters, status};
  hipLaunchKernelGGL(two_view_kernel, dim3(batch), dim3(kTvThreads), lds, static_cast<hipStream_t>(stream), a);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

}  // extern "C"
