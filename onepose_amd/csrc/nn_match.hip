// NearestNeighbour 2D-2D matcher (src/models/matchers/nn/nearest_neighbour.py:5-63): mutual
// nearest neighbour with Lowe's ratio test and a distance test on sim = desc0^T desc1.
//
// The similarity matrix is never written to memory.  Launch 1 is an fp32 tile GEMM on
// v_mfma_f32_32x32x2_f32 whose epilogue reduces each wave's 64 x 64 block of accumulators to
// per-row and per-column (best value, best index, second value) partials; launch 2 merges the
// partials, applies the tests and writes matches1 / scores1 and the raw matches0 / scores0;
// launch 3 (only with do_mutual_check) clears the rows of matches0 whose column does not point
// back.  No atomics and no workgroup waits for another: the result is deterministic.
//
// Order on equal similarities (the reference's topk promises none): (value, index) is a total
// order, larger value first, then LOWER index; the best is its maximum, the second value is the
// second element of the multiset (a duplicated best value is its own runner-up).  Every merge
// below is a maximum under that order, so the grouping of partials cannot change a result.
// sim[i][j] is summed over d in the same order for every (i, j): the K loop runs k = 0, 2, 4, ...
// from LDS panels zero-padded past d, past n0 and past n1, wherever the tile lies.
#include <climits>
#include <cmath>

#include <hip/hip_fp16.h>

#include "common.h"

namespace onepose {
namespace {

constexpr int kNnMaxN = 16384, kNnMaxD = 1024, kNnMaxBatch = 65535;
constexpr int kNnTile = 128;   // workgroup tile: 128 rows x 128 columns, 4 waves of 64 x 64
constexpr int kNnPart = 64;    // partial granularity: one per wave block
constexpr int kNnKC = 32;      // K rows of both panels staged per step
constexpr int kNnThreads = 256;
constexpr int kNnLoads = kNnKC * kNnTile / kNnThreads;   // elements per thread, panel and stage

// (best value, best index, second value) of a set of (value, index) pairs
struct __attribute__((aligned(16))) Top2 {
  float bv;
  int bi;
  float sv;
  int pad;
};

__device__ __forceinline__ bool nn_better(float v, int i, float bv, int bi) {
  return v > bv || (v == bv && i < bi);
}
__device__ __forceinline__ void nn_insert(float& bv, int& bi, float& sv, float v, int i) {
  if (nn_better(v, i, bv, bi)) {
    sv = bv;
    bv = v;
    bi = i;
  } else {
    sv = fmaxf(sv, v);
  }
}
__device__ __forceinline__ void nn_merge(float& bv, int& bi, float& sv, float ov, int oi,
                                         float os) {
  if (nn_better(ov, oi, bv, bi)) {
    sv = fmaxf(os, bv);
    bv = ov;
    bi = oi;
  } else {
    sv = fmaxf(sv, ov);
  }
}

__device__ __forceinline__ float nn_ld(const float* p) { return *p; }
__device__ __forceinline__ float nn_ld(const __half* p) { return __half2float(*p); }

struct SimArgs {
  const void *d0, *d1;
  int64_t bs0, bs1;   // batch strides, elements (0: shared)
  int d, n0, n1;
  int ct, rt;         // partials per row (ceil(n1 / 64)) and per column (ceil(n0 / 64))
  Top2 *rowpart, *colpart;
};

// One workgroup per (column tile, row tile, batch entry).  Panels A = desc0[k][row0 ..] and
// B = desc1[k][col0 ..] are staged K-major, as they lie in memory; the MFMA takes A[i][k] from
// lane (i, k & 1) and B[k][j] from lane (j, k & 1), and accumulator register r of lane
// (j, hh) holds row 8 (r / 4) + 4 hh + r % 4 of column j.
template <class T>
__global__ __launch_bounds__(kNnThreads, 2) void nn_sim_top2_kernel(SimArgs P) {
  typedef float floatx16 __attribute__((ext_vector_type(16)));
  __shared__ float As[kNnKC][kNnTile];
  __shared__ float Bs[kNnKC][kNnTile];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, hh = lane >> 5, l31 = lane & 31;
  const int wr = w >> 1, wc = w & 1;
  const int bz = blockIdx.z;
  const int trow = blockIdx.y * kNnTile, tcol = blockIdx.x * kNnTile;
  const T* g0 = static_cast<const T*>(P.d0) + (int64_t)bz * P.bs0;
  const T* g1 = static_cast<const T*>(P.d1) + (int64_t)bz * P.bs1;
  const int d = P.d, n0 = P.n0, n1 = P.n1;

  // thread t stages element c of rows k = kq + 2 i of a step
  const int c = t & (kNnTile - 1), kq = t >> 7;
  const bool in0 = trow + c < n0, in1 = tcol + c < n1;
  float ra[kNnLoads], rb[kNnLoads];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < kNnLoads; ++i) {
      const int k = k0 + kq + 2 * i;
      ra[i] = (in0 && k < d) ? nn_ld(g0 + (int64_t)k * n0 + trow + c) : 0.f;
      rb[i] = (in1 && k < d) ? nn_ld(g1 + (int64_t)k * n1 + tcol + c) : 0.f;
    }
  };

  floatx16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  fetch(0);
  for (int k0 = 0; k0 < d; k0 += kNnKC) {
    __syncthreads();   // the previous step's readers are done
#pragma unroll
    for (int i = 0; i < kNnLoads; ++i) {
      As[kq + 2 * i][c] = ra[i];
      Bs[kq + 2 * i][c] = rb[i];
    }
    __syncthreads();
    if (k0 + kNnKC < d) fetch(k0 + kNnKC);
    const int kend = min(kNnKC, (d - k0 + 1) & ~1);   // an odd d is padded with one zero row
    const float* ap = &As[hh][wr * 64 + l31];
    const float* bp = &Bs[hh][wc * 64 + l31];
    auto step = [&](int kk) {
      const float a0 = ap[kk * kNnTile], a1 = ap[kk * kNnTile + 32];
      const float b0 = bp[kk * kNnTile], b1 = bp[kk * kNnTile + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    };
    if (kend == kNnKC) {   // a full stage, unrolled; the same k order as the ragged one
#pragma unroll
      for (int kk = 0; kk < kNnKC; kk += 2) step(kk);
    } else {
      for (int kk = 0; kk < kend; kk += 2) step(kk);
    }
  }

  // ---- epilogue: this wave's 64 x 64 block (no barrier below, so a wave may leave)
  const int row0 = trow + wr * 64, col0 = tcol + wc * 64;
  if (row0 >= n0 || col0 >= n1) return;
  // rows / columns past n0 / n1 hold zeros, which could beat real negatives: they enter every
  // reduction as (-inf, INT_MAX), below anything real
  const bool edge = row0 + 64 > n0 || col0 + 64 > n1;   // wave-uniform
  if (edge) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = row0 + 32 * a + 8 * (r >> 2) + 4 * hh + (r & 3);
          const int col = col0 + 32 * b + l31;
          if (row >= n0 || col >= n1) acc[a][b][r] = -INFINITY;
        }
  }

  // columns: the lane's 32 rows of column 32 b + l31, then the other half's
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int col = col0 + 32 * b + l31;
    float bv = -INFINITY, sv = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + 32 * a + 8 * (r >> 2) + 4 * hh + (r & 3);
        const float v = acc[a][b][r];
        nn_insert(bv, bi, sv, v, (row < n0 && col < n1) ? row : INT_MAX);
      }
    const float ov = __shfl_xor(bv, 32, 64), os = __shfl_xor(sv, 32, 64);
    const int oi = __shfl_xor(bi, 32, 64);
    nn_merge(bv, bi, sv, ov, oi, os);
    if (hh == b && col < n1) {
      Top2 o{bv, bi, sv, 0};
      P.colpart[((int64_t)bz * n1 + col) * P.rt + row0 / kNnPart] = o;
    }
  }

  // rows, one half (a) of the block at a time: state r is the lane's row
  // 32 a + 8 (r / 4) + 4 hh + r % 4 over its two columns.  Four steps over lane bits 0..3 fold
  // 16 states to one per lane, halving the states a lane keeps at every step (lane bit s keeps
  // the upper half, sends the lower); lane bit 4 then joins the two groups of 16 columns.
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    float bv[16], sv[16];
    int bi[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + 32 * a + 8 * (r >> 2) + 4 * hh + (r & 3);
      bv[r] = -INFINITY;
      sv[r] = -INFINITY;
      bi[r] = INT_MAX;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int col = col0 + 32 * b + l31;
        nn_insert(bv[r], bi[r], sv[r], acc[a][b][r], (row < n0 && col < n1) ? col : INT_MAX);
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int half = 8 >> s;
      const bool up = (l31 >> s) & 1;
#pragma unroll
      for (int k = 0; k < half; ++k) {
        const float mv = up ? bv[k + half] : bv[k], ms = up ? sv[k + half] : sv[k];
        const int mi = up ? bi[k + half] : bi[k];
        const float tv = up ? bv[k] : bv[k + half], ts = up ? sv[k] : sv[k + half];
        const int ti = up ? bi[k] : bi[k + half];
        const float ov = __shfl_xor(tv, 1 << s, 64), os = __shfl_xor(ts, 1 << s, 64);
        const int oi = __shfl_xor(ti, 1 << s, 64);
        bv[k] = mv;
        bi[k] = mi;
        sv[k] = ms;
        nn_merge(bv[k], bi[k], sv[k], ov, oi, os);
      }
    }
    {
      const float ov = __shfl_xor(bv[0], 16, 64), os = __shfl_xor(sv[0], 16, 64);
      const int oi = __shfl_xor(bi[0], 16, 64);
      nn_merge(bv[0], bi[0], sv[0], ov, oi, os);
    }
    // the state this lane ends with: bit s of l31 chose the half of size 8 >> s
    const int r = ((l31 & 1) << 3) | ((l31 & 2) << 1) | ((l31 & 4) >> 1) | ((l31 & 8) >> 3);
    const int row = row0 + 32 * a + 8 * (r >> 2) + 4 * hh + (r & 3);
    if ((l31 >> 4) == a && row < n0) {
      Top2 o{bv[0], bi[0], sv[0], 0};
      P.rowpart[((int64_t)bz * n0 + row) * P.ct + col0 / kNnPart] = o;
    }
  }
}

struct MergeArgs {
  const Top2 *rowpart, *colpart;
  int n0, n1, ct, rt;
  int use_ratio, use_dist;
  float ratio2, dist2;   // float32(ratio ** 2), float32(distance ** 2)
  int64_t *m0, *m1;
  float *s0, *s1;
};

// find_nn (:5-15) on the merged partials, one thread per row (x < n0) or column.  The fp32
// arithmetic is the reference's, operation by operation: dist = 2 * (1 - sim) is one
// subtraction and an exact doubling, the ratio test one multiply and a <=.
__global__ __launch_bounds__(256) void nn_merge_kernel(MergeArgs P) {
  const int x = blockIdx.x * 256 + threadIdx.x, bz = blockIdx.y;
  if (x >= P.n0 + P.n1) return;
  const bool is_row = x < P.n0;
  const int i = is_row ? x : x - P.n0;
  const int np = is_row ? P.ct : P.rt;
  const Top2* p = is_row ? P.rowpart + ((int64_t)bz * P.n0 + i) * P.ct
                         : P.colpart + ((int64_t)bz * P.n1 + i) * P.rt;
  Top2 m = p[0];
  for (int j = 1; j < np; ++j) {
    const Top2 o = p[j];
    nn_merge(m.bv, m.bi, m.sv, o.bv, o.bi, o.sv);
  }
  const float d0 = __fmul_rn(2.f, __fsub_rn(1.f, m.bv));
  // no candidate compared above -inf (NaN descriptors): unmatched, and never an index for
  // the mutual check to follow
  bool ok = (unsigned)m.bi < (unsigned)(is_row ? P.n1 : P.n0);
  if (P.use_ratio) {
    const float d1 = __fmul_rn(2.f, __fsub_rn(1.f, m.sv));
    ok = ok && d0 <= __fmul_rn(P.ratio2, d1);
  }
  if (P.use_dist) ok = ok && d0 <= P.dist2;
  const int64_t match = ok ? (int64_t)m.bi : (int64_t)-1;
  const float score = ok ? __fdiv_rn(__fadd_rn(m.bv, 1.f), 2.f) : 0.f;
  if (is_row) {
    P.m0[(int64_t)bz * P.n0 + i] = match;
    P.s0[(int64_t)bz * P.n0 + i] = score;
  } else {
    P.m1[(int64_t)bz * P.n1 + i] = match;
    P.s1[(int64_t)bz * P.n1 + i] = score;
  }
}

// mutual_check (:18-23): matches0 only; scores0 stays as find_nn left it
__global__ __launch_bounds__(256) void nn_mutual_kernel(int64_t* m0, const int64_t* m1, int n0,
                                                        int n1) {
  const int i = blockIdx.x * 256 + threadIdx.x, bz = blockIdx.y;
  if (i >= n0) return;
  int64_t* p = m0 + (int64_t)bz * n0 + i;
  const int64_t m = *p;
  if (m > -1 && m1[(int64_t)bz * n1 + m] != (int64_t)i) *p = -1;
}

bool shape_ok(int batch, int n0, int n1) {
  return batch >= 1 && batch <= kNnMaxBatch && n0 >= 1 && n0 <= kNnMaxN && n1 >= 1 &&
         n1 <= kNnMaxN;
}

struct NnPlan {
  int ct, rt;
  Top2 *rowpart, *colpart;
  size_t bytes;
};
NnPlan nn_plan(void* ws, int batch, int n0, int n1) {
  NnPlan p;
  p.ct = ceil_div(n1, kNnPart);
  p.rt = ceil_div(n0, kNnPart);
  Carve cv(ws);
  p.rowpart = cv.take<Top2>((size_t)batch * n0 * p.ct);
  p.colpart = cv.take<Top2>((size_t)batch * n1 * p.rt);
  p.bytes = align_up(cv.off, 256);
  return p;
}

// The checks every NN entry shares, in the documented order (onepose_hip.h)
int nn_check(const void* desc0, int64_t bs0, const void* desc1, int64_t bs1, int dtype, int batch,
             int d, int n0, int n1, bool outputs_ok, bool use_ratio, const void* ws,
             size_t ws_bytes, NnPlan* plan) {
  OP_REQUIRE(desc0 && desc1 && outputs_ok && ws, "nn_match: null pointer (descriptors, outputs "
             "and workspace are all required)");
  OP_REQUIRE(batch >= 1 && batch <= kNnMaxBatch, "nn_match: batch %d, need 1..%d", batch,
             kNnMaxBatch);
  OP_REQUIRE(n0 >= 1 && n0 <= kNnMaxN && n1 >= 1 && n1 <= kNnMaxN,
             "nn_match: n0 = %d, n1 = %d, need 1..%d each", n0, n1, kNnMaxN);
  OP_REQUIRE(d >= 1 && d <= kNnMaxD, "nn_match: d = %d, need 1..%d", d, kNnMaxD);
  OP_REQUIRE(dtype == ONEPOSE_DT_F32 || dtype == ONEPOSE_DT_F16,
             "nn_match: desc_dtype %d is neither ONEPOSE_DT_F32 nor ONEPOSE_DT_F16", dtype);
  OP_REQUIRE(bs0 >= 0 && bs1 >= 0, "nn_match: negative batch stride");
  OP_REQUIRE(!use_ratio || (n0 >= 2 && n1 >= 2),
             "nn_match: the ratio test needs 2 candidates on each searched side (n0 = %d, "
             "n1 = %d)", n0, n1);
  *plan = nn_plan(const_cast<void*>(ws), batch, n0, n1);
  if (ws_bytes < plan->bytes) {
    set_error("nn_match: workspace of %zu bytes, %zu needed", ws_bytes, plan->bytes);
    return ONEPOSE_ERR_WORKSPACE;
  }
  return ONEPOSE_OK;
}

int nn_launch_sim(const void* desc0, int64_t bs0, const void* desc1, int64_t bs1, int dtype,
                  int batch, int d, int n0, int n1, const NnPlan& plan, hipStream_t st) {
  SimArgs a{desc0, desc1, bs0, bs1, d, n0, n1, plan.ct, plan.rt, plan.rowpart, plan.colpart};
  const dim3 grid(ceil_div(n1, kNnTile), ceil_div(n0, kNnTile), batch);
  if (dtype == ONEPOSE_DT_F16)
    hipLaunchKernelGGL(nn_sim_top2_kernel<__half>, grid, dim3(kNnThreads), 0, st, a);
  else
    hipLaunchKernelGGL(nn_sim_top2_kernel<float>, grid, dim3(kNnThreads), 0, st, a);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

}  // namespace
}  // namespace onepose

using namespace onepose;

extern "C" {

int onepose_nn_version(void) { return 1; }

size_t onepose_nn_match_workspace_bytes(int batch, int n0, int n1) {
  if (!shape_ok(batch, n0, n1)) return 0;
  return nn_plan(nullptr, batch, n0, n1).bytes;
}

int onepose_nn_similarity_top2(const void* desc0, int64_t desc0_bstride, const void* desc1,
                               int64_t desc1_bstride, int desc_dtype, int batch, int d, int n0,
                               int n1, void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  NnPlan plan;
  const int rc = nn_check(desc0, desc0_bstride, desc1, desc1_bstride, desc_dtype, batch, d, n0,
                          n1, true, false, workspace, workspace_bytes, &plan);
  if (rc != ONEPOSE_OK) return rc;
  return nn_launch_sim(desc0, desc0_bstride, desc1, desc1_bstride, desc_dtype, batch, d, n0, n1,
                       plan, static_cast<hipStream_t>(stream));
}

int onepose_nn_match(const void* desc0, int64_t desc0_bstride, const void* desc1,
                     int64_t desc1_bstride, int desc_dtype, int batch, int d, int n0, int n1,
                     double ratio_threshold, double distance_threshold, int do_mutual_check,
                     int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                     void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  const bool use_ratio = ratio_threshold > 0.0, use_dist = distance_threshold > 0.0;   // NaN: off
  NnPlan plan;
  int rc = nn_check(desc0, desc0_bstride, desc1, desc1_bstride, desc_dtype, batch, d, n0, n1,
                    matches0 && matches1 && mscores0 && mscores1, use_ratio, workspace,
                    workspace_bytes, &plan);
  if (rc != ONEPOSE_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  rc = nn_launch_sim(desc0, desc0_bstride, desc1, desc1_bstride, desc_dtype, batch, d, n0, n1,
                     plan, st);
  if (rc != ONEPOSE_OK) return rc;
  MergeArgs m{plan.rowpart, plan.colpart, n0, n1, plan.ct, plan.rt, use_ratio ? 1 : 0,
              use_dist ? 1 : 0,
              use_ratio ? (float)std::pow(ratio_threshold, 2.0) : 0.f,   // Python's ratio ** 2,
              use_dist ? (float)std::pow(distance_threshold, 2.0) : 0.f,   // rounded to float32
              matches0, matches1, mscores0, mscores1};
  hipLaunchKernelGGL(nn_merge_kernel, dim3(ceil_div(n0 + n1, 256), batch), dim3(256), 0, st, m);
  OP_LAUNCHED();
  if (do_mutual_check) {
    hipLaunchKernelGGL(nn_mutual_kernel, dim3(ceil_div(n0, 256), batch), dim3(256), 0, st,
                       matches0, matches1, n0, n1);
    OP_LAUNCHED();
  }
  return ONEPOSE_OK;
}

}  // extern "C"
